"""The capture sharpening of include/tdk_hip_deconv.h restated in NumPy: every array below is float32, so NumPy rounds each written
operation once and contracts nothing; division and square root are correctly rounded.  tests/test_deconv_spec.py holds this file to
literal per-pixel loops and to its purpose; tests/test_gpu_deconv.py holds the kernel to it bit for bit."""

import math

import numpy as np

f32 = np.float32
TINY = f32(2.0 ** -20)
REC709 = (0.2126, 0.7152, 0.0722)
MAX_RADIUS, MAX_ITERATIONS, MAX_FUSED, TILE = 6, 50, 4, 32
MASK, FUSE_SHIFT, FUSE_MASK = 1, 8, 0xF00


def gaussian_taps(sigma):
    """The formula of tdk_deconv_weights in float64, rounded once to float32: (w0 .. wR), R = ceil(3 sigma)."""
    s = float(f32(sigma))
    radius = math.ceil(3.0 * s)
    w = [1.0] + [math.exp(-(k * k) / (2.0 * s * s)) for k in range(1, radius + 1)]
    tail = 0.0
    for v in w[1:]:
        tail += v
    return tuple(f32(v / (w[0] + 2.0 * tail)) for v in w)


def pos(v):
    return np.where(v > 0, v, f32(0)).astype(f32)


def luminance(x, weights=REC709):
    """o of a (H, W, 1 or 3) frame."""
    x = x.astype(f32)
    if x.shape[2] == 3:
        l0, l1, l2 = (f32(v) for v in weights)
        y = pos((l0 * x[..., 0] + l1 * x[..., 1]) + l2 * x[..., 2])
    else:
        y = pos(x[..., 0])
    return np.fmax(y, TINY)


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


def iterate(o, taps, iterations):
    u = o
    for _ in range(iterations):
        q = o / np.fmax(blur(u, taps), TINY)
        u = u * blur(q, taps)
    return u


def contrast_mask(o, threshold):
    """m; threshold None: 1 everywhere."""
    if threshold is None:
        return np.ones_like(o)
    around = [shift(shift(o, dy, 0), dx, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    hi, lo = np.maximum.reduce(around), np.minimum.reduce(around)
    t = f32(threshold)
    it = f32(1.0) / t
    d = np.sqrt(hi) - np.sqrt(lo)
    e = np.fmin(np.fmax((d - t) * it, f32(0)), f32(1))
    return (e * e) * (f32(3) - f32(2) * e)


def process(x, taps, iterations=8, threshold=0.02, max_gain=4.0, weights=REC709):
    """(the frame in the type of x, m)."""
    assert x.ndim == 3 and x.shape[2] in (1, 3) and x.dtype in (np.float32, np.float16)
    o = luminance(x, weights)
    m = contrast_mask(o, threshold)
    if iterations == 0:
        return x.copy(), m
    u = iterate(o, taps, iterations)
    gain = f32(max_gain)
    yn = o + m * (u - o)
    g = np.fmin(np.fmax(yn / o, f32(1.0) / gain), gain)
    with np.errstate(over='ignore'):
        out = (x.astype(f32) * g[..., None]).astype(x.dtype)
    return out, m


def launches(iterations, fused):
    return 1 if iterations == 0 else -(-iterations // fused)


def workspace_bytes(width, height, n_launches):
    """What tdk_deconv_workspace_bytes answers for a call of that many launches."""
    planes = min(n_launches - 1, 2)
    return 0 if planes == 0 else planes * (-(-(width * height * 4) // 16) * 16) + 16
