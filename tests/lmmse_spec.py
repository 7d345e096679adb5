"""NumPy float32 restatement of include/tdk_hip_lmmse.h (tdk_lmmse), whole planes at a time.

Every operation is one float32 NumPy operation in the header's order, so the result predicts the device's bits.  The frame is
extended by the apron with the folded (reflected) index once; every plane is then evaluated on the extended grid.  np.roll wraps
values around the extended grid's rim, which spoils at most TDK_LMMSE_APRON positions from the rim inwards: exactly what is cropped.
That a plane evaluated at a reflected position has the bits of its value at the folded index is the header's remark on symmetry;
tests/test_lmmse_spec.py holds this module to literal loops that take the value at the folded index instead."""
import numpy as np

F = np.float32
RGGB, BGGR, GRBG, GBRG = 0x94949494, 0x16161616, 0x61616161, 0x49494949
PATTERNS = {'RGGB': RGGB, 'BGGR': BGGR, 'GRBG': GRBG, 'GBRG': GBRG}
APRON = 11
LINEAR = 1   # TDK_LMMSE_LINEAR

_w = np.exp(-np.arange(5, dtype=np.float64) ** 2 / 8.0)
G = (_w / (_w[0] + 2.0 * _w[1:].sum())).astype(F)   # g0..g4, formed in double and rounded once
NINTH = F(1.0 / 9.0)
EPS = F(1e-7)
HALF, QUARTER = F(0.5), F(0.25)


def cfa_color(row, col, pattern: int):
    """0 = R, 1 = G, 2 = B: the pattern word of tdk_hip.h."""
    return (pattern >> ((((row << 1) & 14) + (col & 1)) << 1)) & 3


def fold(i, n: int):
    """Reflection about the edge sample without repeating it, folded until the index lies inside; n >= 2."""
    period = 2 * (n - 1)
    i = np.abs(np.asarray(i)) % period
    return np.where(i < n, i, period - i)


def flip_pattern(pattern: int, horizontal: bool, size: int) -> int:
    """The pattern of a mosaic flipped along an axis of `size` samples: the same for an odd size, rows or columns swapped otherwise."""
    if size % 2 == 1:
        return pattern
    c = [[int(cfa_color(r, k, pattern)) for k in (0, 1)] for r in (0, 1)]
    c = [row[::-1] for row in c] if horizontal else c[::-1]
    return next(p for p in PATTERNS.values() if [[int(cfa_color(r, k, p)) for k in (0, 1)] for r in (0, 1)] == c)


def _pair(a, k, axis):
    """a[-k] + a[+k] along an axis"""
    return np.roll(a, k, axis) + np.roll(a, -k, axis)


def _window(a, axis):
    s = a.copy()
    for k in range(1, 5):
        s = s + _pair(a, k, axis)
    return s


def _direction(t, green, axis):
    """(x, v) of one direction on the extended grid (meaningful at red and blue sites)."""
    e = (HALF * _pair(t, 1, axis) - QUARTER * _pair(t, 2, axis)) + HALF * t
    d = np.where(green, t - e, e - t)
    p = G[0] * d
    for k in range(1, 5):
        p = p + G[k] * _pair(d, k, axis)
    mu = _window(p, axis) * NINTH
    # mu belongs to the window's centre: a[k] = (p[k] - mu)^2 is formed per centre, so the window is summed tap by tap
    def spread(q, centre):
        s = (q - centre) * (q - centre)
        for k in range(1, 5):
            lo, hi = np.roll(q, k, axis) - centre, np.roll(q, -k, axis) - centre
            s = s + (lo * lo + hi * hi)
        return s
    vx = EPS + spread(p, mu)
    r = d - p
    vn = EPS + _window(r * r, axis)
    total = vx + vn
    return (p * vn + d * vx) / total, (vx * vn) / total


def to_float32(mosaic) -> np.ndarray:
    m = np.asarray(mosaic)
    if m.ndim == 3:
        assert m.shape[2] == 1
        m = m[:, :, 0]
    assert m.dtype in (np.float32, np.float16), m.dtype
    return m.astype(F)


def lmmse(mosaic, pattern: int, flags: int = 0, out_dtype=None) -> np.ndarray:
    """(H, W) float32 or float16 mosaic -> (H, W, 3) in out_dtype (default: the mosaic's); the bits of tdk_lmmse."""
    src = np.asarray(mosaic)
    if src.ndim == 3:
        src = src[:, :, 0]
    out_dtype = np.dtype(src.dtype if out_dtype is None else out_dtype)
    m = to_float32(src)
    h, w = m.shape
    assert h >= 2 and w >= 2
    with np.errstate(all='ignore'):
        t = m if flags & LINEAR else np.sqrt(np.maximum(m, F(0)))
        ys, xs = np.arange(-APRON, h + APRON), np.arange(-APRON, w + APRON)
        t = np.ascontiguousarray(t[np.ix_(fold(ys, h), fold(xs, w))])
        colour = cfa_color(ys[:, None] & 1, xs[None, :] & 1, pattern)   # reflection keeps the parity of an index
        green = colour == 1
        xh, vh = _direction(t, green, 1)
        xv, vv = _direction(t, green, 0)
        D = (xh * vv + xv * vh) / (vh + vv)
        G_rb = t + D
        along = t - HALF * _pair(D, 1, 1)      # at a green site: the colour that shares the row
        across = t - HALF * _pair(D, 1, 0)     # ... and the other
        up, down = np.roll(D, 1, 0), np.roll(D, -1, 0)
        other = G_rb - QUARTER * ((np.roll(up, 1, 1) + np.roll(up, -1, 1)) + (np.roll(down, 1, 1) + np.roll(down, -1, 1)))
        row_colour = np.roll(colour, -1, 1)    # the colour of the horizontal neighbours (both the same)
        row_colour[:, -1] = colour[:, -2]

        def finish(c):
            if flags & LINEAR:
                return c
            q = np.maximum(c, F(0))
            return q * q

        est = np.empty(t.shape + (3,), F)
        est[..., 1] = finish(G_rb)
        for ch in (0, 2):
            est[..., ch] = np.where(green, np.where(row_colour == ch, finish(along), finish(across)), finish(other))
    crop = (slice(APRON, APRON + h), slice(APRON, APRON + w))
    out = est[crop].astype(out_dtype)
    own = src.astype(F).astype(out_dtype) if src.dtype != out_dtype else src   # the own colour is the input sample itself
    ch = colour[crop]
    for c in range(3):
        out[..., c] = np.where(ch == c, own, out[..., c])
    return out
