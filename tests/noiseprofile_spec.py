"""NumPy restatement of include/tdk_hip_noise.h: what tdk_noise_profile, tdk_noise_stabilize and tdk_noise_unstabilize must compute,
to the last integer and the last float bit.  Counters are Python integers, the derived values Python floats (IEEE double, one
rounding per operation), the transform is float32 operation by operation.  Shared by test_noiseprofile_spec.py (which holds this
file to independent evaluations) and test_gpu_noiseprofile.py (which holds the kernels to this file)."""

import math

import numpy as np

LEVELS = 128
KAPPA = 0.9796   # TDK_NOISE_MEDIAN_FACTOR
RGGB, BGGR, GRBG, GBRG = 0x94949494, 0x16161616, 0x61616161, 0x49494949
F = np.float32


def level(e):
    """The level of the integer block energy e, in integers alone."""
    e = int(e)
    if e < 256:
        return 0
    lg = e.bit_length() - 1
    return min(4 * (lg - 8) + ((e >> (lg - 2)) & 3) + 1, LEVELS - 1)


def level_edge(l):
    """E_lo(l), l >= 1: the smallest energy of level l."""
    return (4 + ((l - 1) & 3)) << (((l - 1) >> 2) + 6)


def quantise(frame, white):
    """(q as int64, NaN mask) of a frame of float32, float16 or uint16."""
    x = np.asarray(frame).astype(F)
    scale = F(65535.0) / F(white)
    with np.errstate(invalid='ignore'):
        q = np.rint(np.fmin(np.fmax(x * scale, F(0.0)), F(65535.0)))
    return q.astype(np.int64), np.isnan(x)


def block_statistics(frames, pattern, bins=32, white=1.0, clip=(1, 64224)):
    """{'hist': [3][bins][128], 'sum': [3][bins], 'blocks', 'nan', 'clipped': [3]} as nested lists of Python integers."""
    hist = [[[0] * LEVELS for _ in range(bins)] for _ in range(3)]
    sums = [[0] * bins for _ in range(3)]
    blocks, nan, clipped = [0] * 3, [0] * 3, [0] * 3
    for frame in frames:
        q, isnan = quantise(frame, white)
        for p in range(4):
            k = (pattern >> (2 * p)) & 3
            plane, bad = q[p >> 1::2, p & 1::2], isnan[p >> 1::2, p & 1::2]
            nby, nbx = plane.shape[0] // 8, plane.shape[1] // 8
            if nby == 0 or nbx == 0:
                continue
            b = plane[:nby * 8, :nbx * 8].reshape(nby, 8, nbx, 8).transpose(0, 2, 1, 3)
            bad = bad[:nby * 8, :nbx * 8].reshape(nby, 8, nbx, 8).transpose(0, 2, 1, 3).any(axis=(2, 3))
            s = b.sum(axis=(2, 3))
            h = 2 * b[:, :, :, 1:7] - b[:, :, :, 0:6] - b[:, :, :, 2:8]
            v = 2 * b[:, :, 1:7, :] - b[:, :, 0:6, :] - b[:, :, 2:8, :]
            e = (h * h).sum(axis=(2, 3)) + (v * v).sum(axis=(2, 3))
            out = (b.min(axis=(2, 3)) < clip[0]) | (b.max(axis=(2, 3)) > clip[1])
            for by in range(nby):
                for bx in range(nbx):
                    blocks[k] += 1
                    if bad[by, bx]:
                        nan[k] += 1
                    elif out[by, bx]:
                        clipped[k] += 1
                    else:
                        total = int(s[by, bx])
                        i = ((total >> 6) * bins) >> 16
                        hist[k][i][level(e[by, bx])] += 1
                        sums[k][i] += total
    return {'hist': hist, 'sum': sums, 'blocks': blocks, 'nan': nan, 'clipped': clipped}


def counts_vector(stats):
    """The statistics in the order of the `counts` block of the header, int64."""
    flat = [n for per in stats['hist'] for row in per for n in row] + [n for per in stats['sum'] for n in per]
    return np.array(flat + stats['blocks'] + stats['nan'] + stats['clipped'], dtype=np.int64)


def bin_point(h, total, white, min_count):
    """(x, v, w) of one intensity bin as Python floats, or None when the bin is unusable."""
    n = sum(h)
    if n < min_count:
        return None
    r = min(max(int(math.ceil(0.5 * float(n))), 1), n)
    cum = 0
    for at in range(LEVELS):
        if cum + h[at] >= r:
            break
        cum += h[at]
    if at == 0 or at == LEVELS - 1:
        return None
    frac = float(r - cum) / float(h[at])
    lo, hi = float(level_edge(at)), float(level_edge(at + 1))
    e_med = lo + frac * (hi - lo)
    ws = float(F(white)) / 65535.0
    v = (e_med / (576.0 * KAPPA)) * (ws * ws)
    x = ((float(total) / (64.0 * float(n))) / 65535.0) * float(F(white))
    return x, v, float(n) / (v * v)


def fit(points):
    """(a, b, valid) of the weighted line through [(x, v, w), ...], i ascending, as the header writes it."""
    sw = swx = swxx = swv = swxv = 0.0
    for x, v, w in points:
        wx = w * x
        sw += w
        swx += wx
        swxx += wx * x
        swv += w * v
        swxv += wx * v
    det = sw * swxx - swx * swx
    if len(points) < 2 or not det > 0.0:
        return 0.0, 0.0, 0
    a = (sw * swxv - swx * swv) / det
    b = (swxx * swv - swx * swxv) / det
    if a < 0.0:
        a, b = 0.0, swv / sw
    elif b < 0.0:
        b, a = 0.0, swxv / swxx
    return a, b, 1


def derive(stats, bins=32, white=1.0, min_count=32):
    """(model (3, 4) float32, curve (2, 3, bins) float32) from the statistics."""
    model, curve = np.zeros((3, 4), F), np.zeros((2, 3, bins), F)
    for k in range(3):
        points = []
        for i in range(bins):
            pt = bin_point(stats['hist'][k][i], stats['sum'][k][i], white, min_count)
            if pt is not None:
                points.append(pt)
                curve[0, k, i], curve[1, k, i] = F(pt[0]), F(pt[1])
        a, b, valid = fit(points)
        model[k] = (F(a), F(b), F(valid), F(len(points)))
    return model, curve


def estimate(frames, pattern, bins=32, white=1.0, clip=(1, 64224), min_count=32):
    """(counts int64 vector, model, curve) of a list of mosaics."""
    stats = block_statistics(frames, pattern, bins, white, clip)
    model, curve = derive(stats, bins, white, min_count)
    return counts_vector(stats), model, curve


# ---- the transform
def rows_of(shape, pattern=None):
    """The model row of every element of a mosaic (pattern given) or of a (..., C) image."""
    if pattern is not None:
        i, j = np.indices(shape)
        return ((pattern >> (2 * (2 * (i & 1) + (j & 1)))) & 3).astype(np.int64)
    if shape[-1] == 1:
        return np.zeros(shape, np.int64)
    return np.broadcast_to(np.arange(3), shape).astype(np.int64)


def _constants(model, gains, sigma_out):
    model = np.asarray(model, F)
    g = np.ones(3, F) if gains is None else np.asarray(gains, F)
    s = F(sigma_out)
    with np.errstate(all='ignore'):
        a = g * model[:, 0]
        b = (g * g) * model[:, 1]
        c = F(0.375) * (a * a) + b
        k = (F(2.0) * s) / a
        sb = np.sqrt(b)
        coa = c / a
        sn2 = b / (a * a)
    identity = (model[:, 2] == 0) | ((a == 0) & (b == 0))
    gauss = ~identity & (a == 0)
    return s, a, c, k, sb, coa, sn2, identity, gauss


def _store(values, out_dtype):
    return values.astype(out_dtype)   # float32 -> float16 rounds to nearest even, once


def stabilize(x, model, pattern=None, gains=None, sigma_out=1.0, out_dtype=np.float32):
    x = np.asarray(x)
    row = rows_of(x.shape, pattern)
    x = x.astype(F)
    s, a, c, k, sb, _, _, identity, gauss = _constants(model, gains, sigma_out)
    with np.errstate(all='ignore'):
        y = k[row] * np.sqrt(np.fmax(a[row] * x + c[row], F(0.0)))
        y = np.where(gauss[row], (s * x) / sb[row], y)
    return _store(np.where(identity[row], x, y).astype(F), out_dtype)


def unstabilize(y, model, pattern=None, gains=None, sigma_out=1.0, inverse='unbiased', out_dtype=None):
    y = np.asarray(y)
    out_dtype = y.dtype if out_dtype is None else out_dtype
    row = rows_of(y.shape, pattern)
    y = y.astype(F)
    s, a, c, _, sb, coa, sn2, identity, gauss = _constants(model, gains, sigma_out)
    with np.errstate(all='ignore'):
        d = y / s
        if inverse == 'algebraic':
            x = ((a[row] * (d * d)) * F(0.25)) - coa[row]
        else:
            assert inverse == 'unbiased', inverse
            big = np.fmax(d, F(1.2247449))
            d2 = big * big
            i = (((((d2 * F(0.25)) + (F(0.30618622) / big)) - (F(1.375) / d2)) + (F(0.76546554) / (d2 * big))) - F(0.125)) - sn2[row]
            x = a[row] * np.fmax(i, F(0.0))
        x = np.where(gauss[row], d * sb[row], x)
    return _store(np.where(identity[row], y, x).astype(F), out_dtype)
