"""The specification of the reduced-size demosaic (include/tdk_hip_scaled.h) as a float32 NumPy restatement: every intermediate is a
float32 value, fmaf(a, b, c) is a*b + c rounded once.  It shares no code with the product; the CPU tests hold it to literal
per-output loops (tests/test_scaled_demosaic_spec.py) and the GPU tests compare the kernel's raw bits with it
(tests/test_gpu_scaled_demosaic.py)."""

import numpy as np

f32 = np.float32
RGGB, BGGR, GRBG, GBRG = 0x94949494, 0x16161616, 0x61616161, 0x49494949
PATTERNS = {'RGGB': RGGB, 'BGGR': BGGR, 'GRBG': GRBG, 'GBRG': GBRG}
MIN_RATIO, MAX_RATIO, MAX_TAPS = 2, 16, 32
LDS_BYTES = 57600   # the static LDS of one workgroup: 8 staged rows of 136 16-byte segments, 8192 + 1024 + 512 + 128 floats, 192 ints


def cfa_color(row, col, pattern: int):
    """0 = R, 1 = G, 2 = B: the pattern word of tdk_hip.h."""
    return (pattern >> ((((row << 1) & 14) + (col & 1)) << 1)) & 3


def fmaf(a, b, c):
    """a*b + c rounded once to float32.  The product of two float32 values is exact in float64; the float64 sum is made odd where it
    is inexact (its error comes from TwoSum), so the second rounding, to 24 bits, is the rounding of the exact value."""
    with np.errstate(invalid='ignore', over='ignore'):
        p = np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64)
        c = np.asarray(c, dtype=np.float64)
        p, c = np.broadcast_arrays(p, c)
        s = p + c
        t = s - p
        err = (p - (s - t)) + (c - t)
        bits = s.copy().view(np.int64)
        inexact = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((bits & 1) == 0)
        away = (err > 0) == (s > 0)   # the exact value lies further from zero than s
        bits = np.where(inexact, bits + np.where(away, 1, -1), bits)
        return bits.view(np.float64).astype(f32)


def axis_taps(n_in: int, n_out: int):
    """For every output i: (j, w) -- the taps that take part, ascending, and their float32 weights.  Plain integers throughout."""
    assert MIN_RATIO * n_out <= n_in <= MAX_RATIO * n_out and n_out >= 1
    out = []
    for i in range(n_out):
        js, ws = [], []
        for j in range(max(0, (2 * i + 1) * n_in // (2 * n_out) - n_in // n_out - 2), n_in):
            num = 2 * n_out * j + n_out - (2 * i + 1) * n_in
            if num >= 2 * n_in:
                break
            if abs(num) < 2 * n_in:
                js.append(j)
                ws.append(f32(1) - f32(abs(num)) / f32(2 * n_in))
        out.append((np.array(js, dtype=np.int64), np.array(ws, dtype=f32)))
    return out


def max_parity_taps(n_in: int, n_out: int) -> int:
    """The largest number of taps of one parity an output has: T of the flat-frame bound."""
    return max(max(int((j & 1 == p).sum()) for p in (0, 1)) for j, _ in axis_taps(n_in, n_out))


def flat_bound(width, height, out_width, out_height) -> float:
    """The header's relative error bound of a flat frame: g(n) = n u / (1 - n u), u = 2^-24, n = 2 (Tx + Ty + 1)."""
    n = 2 * (max_parity_taps(width, out_width) + max_parity_taps(height, out_height) + 1)
    u = 2.0 ** -24
    return n * u / (1.0 - n * u)


def _chains(x, taps, n_out):
    """One pass along axis 0 of a float32 array: (acc[p] of shape (n_out, ...), sums[p] of shape (n_out,)) for the parities p."""
    acc = [np.zeros((n_out,) + x.shape[1:], f32) for _ in (0, 1)]
    sums = [np.zeros(n_out, f32) for _ in (0, 1)]
    with np.errstate(invalid='ignore', over='ignore'):
        for i, (js, ws) in enumerate(taps):
            for p in (0, 1):
                a = s = None
                for j, w in zip(js, ws):
                    if (j & 1) != p:
                        continue
                    if a is None:
                        a, s = w * x[j], w
                    else:
                        a, s = fmaf(w, x[j], a), f32(s + w)
                assert a is not None, (i, p)
                acc[p][i], sums[p][i] = a, s
    return acc, sums


def balance(x, gains, pattern: int, half: bool = False):
    """The mosaic tdk_apply_white_balance writes: fminf(fmaxf(x*g, 0), 1) per site (a NaN becomes 0), rounded to binary16 when the
    mosaic is stored as binary16."""
    x = np.asarray(x, dtype=f32)
    g = np.asarray(gains, dtype=f32)
    yy, xx = np.mgrid[0:x.shape[0], 0:x.shape[1]]
    with np.errstate(invalid='ignore', over='ignore'):
        v = np.fmin(np.fmax(x * g[cfa_color(yy, xx, pattern)], f32(0)), f32(1)).astype(f32)
    return v.astype(np.float16).astype(f32) if half else v


def decode12(packed, width, height, ids: bool):
    """The float32 mosaic tdk_decode12_f32 (scaled) writes for the packed bytes."""
    b = np.asarray(packed, dtype=np.uint8).astype(np.uint32).reshape(-1, 3)
    if ids:
        p0, p1 = (b[:, 0] << 4) | (b[:, 2] & 0xF), (b[:, 1] << 4) | (b[:, 2] >> 4)
    else:
        p0, p1 = ((b[:, 1] & 0xF) << 8) | b[:, 0], (b[:, 2] << 4) | (b[:, 1] >> 4)
    codes = np.stack([p0, p1], axis=1).reshape(height, width)
    return codes.astype(f32) * (f32(1.0) / f32(4095.0))


def encode12(codes, ids: bool):
    """Packed bytes of 12-bit codes (H, W), W even: the layout decode12 reads."""
    c = np.asarray(codes, dtype=np.uint32).reshape(-1, 2)
    p0, p1 = c[:, 0], c[:, 1]
    if ids:
        b = np.stack([p0 >> 4, p1 >> 4, ((p0 & 0xF)) | ((p1 & 0xF) << 4)], axis=1)
    else:
        b = np.stack([p0 & 0xFF, ((p1 & 0xF) << 4) | (p0 >> 8), p1 >> 4], axis=1)
    return b.astype(np.uint8).reshape(-1)


def scaled_demosaic(x, out_width: int, out_height: int, pattern: int, gains=None, out_dtype=np.float32, half_source: bool = False):
    """(H, W) samples (float32 values; binary16 or decoded sites already widened) -> (out_height, out_width, 3) of out_dtype."""
    x = np.asarray(x, dtype=f32)
    if gains is not None:
        x = balance(x, gains, pattern, half=half_source)
    h, w = x.shape
    A, Sx = _chains(np.ascontiguousarray(x.T), axis_taps(w, out_width), out_width)       # A[p]: (out_width, H)
    A = [np.ascontiguousarray(a.T) for a in A]                                           # (H, out_width)
    ytaps = axis_taps(h, out_height)
    B, Sy = {}, None
    for p in (0, 1):
        acc, Sy = _chains(A[p], ytaps, out_height)                                       # acc[q]: (out_height, out_width)
        for q in (0, 1):
            B[q, p] = acc[q]
    out = np.empty((out_height, out_width, 3), f32)
    sites = {c: [(q, p) for q in (0, 1) for p in (0, 1) if cfa_color(q, p, pattern) == c] for c in (0, 1, 2)}   # the even row first
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for c in (0, 2):
            (q, p), = sites[c]
            out[:, :, c] = B[q, p] / (Sy[q][:, None] * Sx[p][None, :])
        (q1, p1), (q2, p2) = sites[1]
        num = B[q1, p1] + B[q2, p2]
        den = Sy[q1][:, None] * Sx[p1][None, :] + Sy[q2][:, None] * Sx[p2][None, :]
        out[:, :, 1] = num / den
    return out.astype(out_dtype)


def tile(width, height, out_width, out_height):
    """The output tile (columns, rows) of one workgroup, as tdk_demosaic_scaled_tile answers: 64 columns up to 8:1 and 32 beyond; the
    most rows, up to 32, whose source rows fit the 8192-float intermediate and whose taps fit the 512-float weight table."""
    tw = 64 if width <= 8 * out_width else 32
    rows = 8192 // (2 * tw)
    ky = (2 * height + out_height - 1) // out_height
    for th in range(32, 1, -1):
        span = ((th - 1) * height + 2 * height) // out_height + 1
        if span <= rows and ky * th <= 512:
            return tw, th
    return tw, 1


def bin2x2(x, pattern: int):
    """(H, W) mosaic, both even -> (H/2, W/2, 3): the plain 2 x 2 binning (the two greens averaged), float64."""
    x = np.asarray(x, dtype=np.float64)
    out = np.zeros((x.shape[0] // 2, x.shape[1] // 2, 3))
    for q in (0, 1):
        for p in (0, 1):
            c = cfa_color(q, p, pattern)
            out[:, :, c] += x[q::2, p::2] * (0.5 if c == 1 else 1.0)
    return out
