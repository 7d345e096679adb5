"""The haze removal of include/tdk_hip_dehaze.h restated in NumPy: steps 1 to 5 in float32 with one rounding per written operation
(every array below is float32, so NumPy rounds each operation once and contracts nothing), the sums of step 3 in int64.  The cell
grid, the tree, the box sums and the upsampling are those of the tone equalizer and come from tests/toneequal_spec.py.
tests/test_dehaze_spec.py holds this file to literal loops and to its purpose; tests/test_gpu_dehaze.py holds the kernels to it bit
for bit."""

import math

import numpy as np

from toneequal_spec import REC709, box, cell_means, inv_window, luminance, pos, tree, upsample

f32 = np.float32
MIN_AMBIENT = f32(2.0 ** -10)
MAX_DARK_RADIUS, MAX_RADIUS, MAX_CELLS, PLANES = 4, 8, 1 << 24, 10


def count_of(quantile, w, h, cell):
    """K, as the host forms it."""
    return max(1, math.floor(quantile * (-(-w // cell)) * (-(-h // cell))))


def cells(x, s, weights=REC709):
    """Step 1: (m, M, L) -- m and M are (CH, CW, 3), L is (CH, CW)."""
    p = pos(x.astype(f32))
    h, w, _ = p.shape
    ch, cw = -(-h // s), -(-w // s)
    yi, xi = np.minimum(np.arange(ch * s), h - 1), np.minimum(np.arange(cw * s), w - 1)
    blocks = p[yi][:, xi].reshape(ch, s, cw, s, 3)
    m = blocks.min(axis=(1, 3))
    mean = tree(tree(blocks, 3), 1) * f32(1.0 / (s * s))
    return m, mean, cell_means(luminance(x, weights), s)


def minwin(p, r):
    """The minimum over the (2r+1)^2 cells around a cell, indices clamped to the grid."""
    h, w = p.shape
    out = p
    for k in range(-r, r + 1):
        out = np.minimum(out, p[:, np.clip(np.arange(w) + k, 0, w - 1)])
    rows = out
    for k in range(-r, r + 1):
        out = np.minimum(out, rows[np.clip(np.arange(h) + k, 0, h - 1)])
    return out


def dark_channel(m, rd):
    """Step 2."""
    return minwin(np.minimum(np.minimum(m[..., 0], m[..., 1]), m[..., 2]), rd)


def fix(v):
    return (np.minimum(v, f32(65536.0)) * f32(1048576.0)).astype(np.int64)


def ambient(d, mean, count):
    """Step 3: the four float32 values A_r, A_g, A_b, n."""
    keys = np.ascontiguousarray(d, dtype=f32).view(np.uint32).ravel()
    threshold = np.partition(keys, keys.size - count)[keys.size - count]   # the count-th largest
    chosen = keys >= threshold
    n = int(chosen.sum())
    sums = fix(mean.reshape(-1, 3)[chosen]).sum(axis=0, dtype=np.int64)
    return np.array([f32((float(int(s)) / float(n)) * 2.0 ** -20) for s in sums] + [f32(n)], dtype=f32)


def clamp_ambient(amb):
    return np.fmax(np.asarray(amb, dtype=f32)[:3], MIN_AMBIENT)


def cell_transmission(m, amb, rd, strength):
    """Step 4, its first half: t per cell."""
    i = f32(1.0) / clamp_ambient(amb)
    q = np.fmin(np.fmin(m[..., 0] * i[0], m[..., 1] * i[1]), m[..., 2] * i[2])
    return f32(1.0) - f32(strength) * np.fmin(minwin(q, rd), f32(1.0))


def coefficients(lum, t, rg, eps):
    """Step 4, its second half: (a, b)."""
    inv, eps = inv_window(rg), f32(eps)
    ml = box(lum, rg) * inv
    mt = box(t, rg) * inv
    cov = box(lum * t, rg) * inv - ml * mt
    var = pos(box(lum * lum, rg) * inv - ml * ml)
    a = cov / (var + eps)
    return a, mt - a * ml


def estimate(x, cell=8, dark_radius=1, count=1, weights=REC709):
    """Steps 1 to 3."""
    m, mean, _ = cells(x, cell, weights)
    return ambient(dark_channel(m, dark_radius), mean, count)


def process(x, amb=None, strength=0.9, floor=0.1, cell=8, dark_radius=1, radius=4, eps=1e-3, count=1, weights=REC709, refine=True):
    """Steps 1 to 5: (the frame in the type of x, tp, the four ambient values).  amb None: estimated with `count`.  refine False
    replaces the guided refinement by plain upsampling of the cell transmission (for the purpose test only)."""
    m, mean, lum = cells(x, cell, weights)
    if amb is None:
        amb = ambient(dark_channel(m, dark_radius), mean, count)
    amb = np.asarray(amb, dtype=f32)
    t = cell_transmission(m, amb, dark_radius, strength)
    h, w, _ = x.shape
    if refine:
        a, b = coefficients(lum, t, radius, eps)
        inv = inv_window(radius)
        raw = upsample(box(a, radius) * inv, h, w, cell) * luminance(x, weights) + upsample(box(b, radius) * inv, h, w, cell)
    else:
        raw = upsample(t, h, w, cell)
    tp = np.fmin(np.fmax(raw, f32(floor)), f32(1.0))
    rt = f32(1.0) / tp
    big = clamp_ambient(amb)
    with np.errstate(over='ignore'):
        out = pos((x.astype(f32) - big) * rt[..., None] + big).astype(x.dtype)
    return out, tp, amb
