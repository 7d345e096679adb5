"""The purple-fringe removal of include/tdk_hip_defringe.h restated in NumPy: every array below is float32, so NumPy rounds each
written operation once and contracts nothing; division and square root are correctly rounded; the frame statistic is summed in
uint64.  tests/test_defringe_spec.py holds this file to literal per-pixel loops, to the header's identities and to its purpose;
tests/test_gpu_defringe.py holds the two kernels to it bit for bit."""

import math

import numpy as np

f32 = np.float32
GLOBAL, LINEAR, STATIC = 0, 1, 2
GROUPS_SHIFT, GROUPS_MASK = 8, 0x7FF00
MAX_RADIUS, MAX_SAMPLE_RADIUS, MAX_GROUPS, TILE = 12, 8, 1024, 32
STAT_SCALE, STAT_CAP = f32(1048576.0), f32(1024.0)


def gaussian_taps(sigma):
    """The formula of tdk_defringe_weights in float64, rounded once to float32: (w0 .. wR), R = ceil(3 sigma)."""
    s = float(f32(sigma))
    radius = math.ceil(3.0 * s)
    w = [1.0] + [math.exp(-(k * k) / (2.0 * s * s)) for k in range(1, radius + 1)]
    tail = 0.0
    for v in w[1:]:
        tail += v
    return tuple(f32(v / (w[0] + 2.0 * tail)) for v in w)


def pos(v):
    return np.where(v > 0, v, f32(0)).astype(f32)


def working(x, linear=False):
    """(Y, Cb, Cr) of a (H, W, 3) frame."""
    t = pos(x.astype(f32))
    if not linear:
        t = np.sqrt(t)
    tr, tg, tb = t[..., 0], t[..., 1], t[..., 2]
    return (f32(0.25) * tr + f32(0.5) * tg) + f32(0.25) * tb, tb - tg, tr - tg


def shift(a, k, axis):
    """a[i + k] along `axis`, the index clamped to the frame (replicate)."""
    n = a.shape[axis]
    return np.take(a, np.clip(np.arange(n) + k, 0, n - 1), axis=axis)


def blur(s, taps):
    """G(s): along x, then along y."""
    for axis in (1, 0):
        h = f32(taps[0]) * s
        for k in range(1, len(taps)):
            h = h + f32(taps[k]) * (shift(s, -k, axis) + shift(s, k, axis))
        s = h
    return s


def edge_chroma(cb, cr, taps):
    """E"""
    db, dr = cb - blur(cb, taps), cr - blur(cr, taps)
    return db * db + dr * dr


def statistic(e):
    """S, an int"""
    q = np.floor(np.fmin(e, STAT_CAP) * STAT_SCALE).astype(np.uint64)
    return int(q.sum(dtype=np.uint64))


def threshold(s, n, strength, floor, static=False):
    """th as a float32"""
    if static:
        return np.fmax(f32(floor), f32(strength))
    avg = f32(np.float64(s) / (np.float64(n) * np.float64(1048576.0)))   # (np.float64(s) rounds the integer once, to nearest even)
    return np.fmax(f32(floor), f32(strength) * avg)


def disc(sample_radius):
    """The offsets (dy, dx) in visiting order."""
    r = int(sample_radius)
    return [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dx * dx + dy * dy <= r * r]


def averaged_chroma(cb, cr, e, th, sample_radius):
    """(Cb', Cr') at every pixel, as if every pixel were fringed."""
    wt = f32(1.0) / (e + th)
    pb, pr = wt * cb, wt * cr
    a, b, n = np.zeros_like(cb), np.zeros_like(cb), np.zeros_like(cb)
    for dy, dx in disc(sample_radius):
        a = a + shift(shift(pb, dy, 0), dx, 1)
        b = b + shift(shift(pr, dy, 0), dx, 1)
        n = n + shift(shift(wt, dy, 0), dx, 1)
    return a / n, b / n


def process(x, taps, sample_radius=6, strength=2.5, floor=1e-4, mode='global', domain='sqrt'):
    """(the frame in the type of x, the mask as uint8, E, S, th)."""
    assert x.ndim == 3 and x.shape[2] == 3 and x.dtype in (np.float32, np.float16)
    assert mode in ('global', 'static') and domain in ('sqrt', 'linear')
    linear = domain == 'linear'
    y, cb, cr = working(x, linear)
    with np.errstate(over='ignore', invalid='ignore'):
        e = edge_chroma(cb, cr, taps)
    s = statistic(e)
    th = threshold(s, e.size, strength, floor, mode == 'static')
    fringed = e > th
    out = x.copy()
    if fringed.any():
        cb2, cr2 = averaged_chroma(cb, cr, e, th, sample_radius)
        g = y - f32(0.25) * (cb2 + cr2)
        v = np.fmax(np.stack([g + cr2, g, g + cb2], axis=-1), f32(0))
        with np.errstate(over='ignore'):
            new = (v if linear else v * v).astype(x.dtype)
        out[fringed] = new[fringed]
    return out, fringed.astype(np.uint8), e, s, th


def workspace_bytes(width, height):
    """What tdk_defringe_workspace_bytes answers."""
    return -(-(width * height * 4) // 16) * 16 + MAX_GROUPS * 8 + 16


def lds_bytes():
    """The first launch: Cb and Cr over the tile and its apron of MAX_RADIUS, their row-blurred planes, four partial sums."""
    p = TILE + 2 * MAX_RADIUS
    return 4 * (2 * p * p + 2 * p * TILE) + 4 * 8


def lds_bytes_correct():
    """The second launch: wt, wt*Cb and wt*Cr over the tile and its apron of MAX_SAMPLE_RADIUS, the new chroma and a flag byte per pixel
    of the tile, four partial sums, four votes."""
    p = TILE + 2 * MAX_SAMPLE_RADIUS
    return 4 * 3 * p * p + (2 * 4 + 1) * TILE * TILE + 4 * 8 + 4 * 4
