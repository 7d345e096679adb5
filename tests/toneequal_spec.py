"""The tone equalizer of include/tdk_hip_toneeq.h restated in NumPy: steps 1 to 7 in float32 with one rounding per written operation
(every array below is float32, so NumPy rounds each operation once and contracts nothing), and the host curve in float64.
tests/test_toneequal_spec.py holds this file to literal per-pixel loops; tests/test_gpu_toneequal.py holds the kernels to it bit for bit."""

import numpy as np

f32 = np.float32
EV_MIN, EV_MAX, STEPS, TABLE = -16, 4, 32, 641
CENTRES = np.arange(-8.0, 1.0)
REC709 = (0.2126, 0.7152, 0.0722)
M_LO, M_HI = f32(2.0 ** EV_MIN), np.nextafter(f32(2.0 ** EV_MAX), f32(0))


# ---- the host curve, float64
def curve(gains_ev, sigma=2 ** 0.5):
    """The weights of the nine Gaussians for which the correction passes through gains_ev at the centres."""
    a = np.exp(-(CENTRES[:, None] - CENTRES[None, :]) ** 2 / (2.0 * sigma ** 2))
    return np.linalg.solve(a, np.asarray(gains_ev, dtype=np.float64))


def correction(ev, weights, sigma=2 ** 0.5):
    ev = np.clip(np.asarray(ev, dtype=np.float64), -8.0, 0.0)
    return (np.asarray(weights) * np.exp(-(ev[..., None] - CENTRES) ** 2 / (2.0 * sigma ** 2))).sum(-1)


def nodes():
    j = np.arange(TABLE)
    return (1.0 + (j % STEPS) / STEPS) * 2.0 ** (EV_MIN + j // STEPS)


def make_table(gains_ev, mask_exposure=0.0, sigma=2 ** 0.5):
    return np.exp2(correction(np.log2(nodes()) + mask_exposure, curve(gains_ev, sigma), sigma)).astype(f32)


# ---- the device, float32
def pos(v):
    return np.where(v > 0, v, f32(0)).astype(f32)


def luminance(x, weights=REC709):
    """Step 1.  x: (H, W, 3) float32 or float16."""
    x = x.astype(f32)
    w0, w1, w2 = (f32(v) for v in weights)
    return pos((w0 * x[..., 0] + w1 * x[..., 1]) + w2 * x[..., 2])


def tree(v, axis):
    """A balanced binary tree over adjacent pairs along `axis`, whose length is a power of two."""
    v = np.moveaxis(v, axis, -1)
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def cell_means(y, s):
    """Step 2."""
    h, w = y.shape
    ch, cw = -(-h // s), -(-w // s)
    yi, xi = np.minimum(np.arange(ch * s), h - 1), np.minimum(np.arange(cw * s), w - 1)
    blocks = y[yi][:, xi].reshape(ch, s, cw, s)
    rows = tree(blocks, 3)            # (ch, s, cw): the row sums
    return tree(rows, 1) * f32(1.0 / (s * s))


def box(p, r):
    """The (2r+1)^2 window sum with clamped indices: horizontally from the lowest index up, then vertically; the first tap starts a sum."""
    h, w = p.shape
    cols = [np.clip(np.arange(w) + k, 0, w - 1) for k in range(-r, r + 1)]
    acc = p[:, cols[0]]
    for c in cols[1:]:
        acc = acc + p[:, c]
    rows = [np.clip(np.arange(h) + k, 0, h - 1) for k in range(-r, r + 1)]
    out = acc[rows[0]]
    for c in rows[1:]:
        out = out + acc[c]
    return out


def inv_window(r):
    return f32(1.0 / float((2 * r + 1) ** 2))


def coefficients(cells, r, eps):
    """Step 3: (a, b)."""
    inv, eps = inv_window(r), f32(eps)
    mean = box(cells, r) * inv
    corr = box(cells * cells, r) * inv
    var = pos(corr - mean * mean)
    a = var / (var + eps)
    return a, mean - a * mean


def taps(n, s, cells):
    """Step 5 along one axis: (first cell, second cell, weight of the second) of the pixels 0 .. n - 1."""
    q = np.maximum(2 * np.arange(n) + 1 - s, 0)
    c0 = q // (2 * s)
    return c0, np.minimum(c0 + 1, cells - 1), (q % (2 * s)).astype(f32) / f32(2 * s)


def lerp(p0, p1, f):
    return p0 + f * (p1 - p0)


def upsample(p, h, w, s):
    ch, cw = p.shape
    y0, y1, fy = taps(h, s, ch)
    x0, x1, fx = taps(w, s, cw)
    top = lerp(p[y0][:, x0], p[y0][:, x1], fx[None, :])
    bottom = lerp(p[y1][:, x0], p[y1][:, x1], fx[None, :])
    return lerp(top, bottom, fy[:, None])


def mask(x, cell=8, radius=4, eps=1e-4, weights=REC709):
    """Steps 1 to 5: the (H, W) float32 mask m."""
    y = luminance(x, weights)
    a, b = coefficients(cell_means(y, cell), radius, eps)
    inv = inv_window(radius)
    h, w = y.shape
    return upsample(box(a, radius) * inv, h, w, cell) * y + upsample(box(b, radius) * inv, h, w, cell)


def gain(m, table):
    """Step 6."""
    mc = np.minimum(np.maximum(m.astype(f32), M_LO), M_HI)
    bits = mc.view(np.uint32).astype(np.int64)
    e, mant = (bits >> 23) - 127, bits & 0x7FFFFF
    i = (e - EV_MIN) * STEPS + (mant >> 18)
    f = (mant & 0x3FFFF).astype(f32) / f32(262144.0)
    return table[i] + f * (table[i + 1] - table[i])


def process(x, table, cell=8, radius=4, eps=1e-4, weights=REC709):
    """Steps 1 to 7: (the frame in the type of x, the mask)."""
    m = mask(x, cell, radius, eps, weights)
    with np.errstate(over='ignore'):
        out = (x.astype(f32) * gain(m, table)[..., None]).astype(x.dtype)
    return out, m
