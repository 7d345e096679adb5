"""NumPy restatement of include/tdk_hip_ca.h: `correct` in float32, one rounding per written operation; `estimate` in integers (the
block sums) and float64 (the fits, as Python floats: IEEE double, one rounding per operation).  What the GPU tests hold the kernels to,
bit for bit, and what tests/test_chromatic_spec.py holds to literal loops and to its purpose."""

import math

import numpy as np

F32 = np.float32
MAX_SHIFT = 8
TILE = (64, 32)
QSCALE, QMAX = F32(65535.0), 65535
SUMS, MIN_SITES, MAX_FRAMES = 17, 16, 16
BILINEAR, BICUBIC = 0, 1
LINEAR, POLY3 = 0, 1
PATTERNS = {'RGGB': 0x94949494, 'BGGR': 0x16161616, 'GRBG': 0x61616161, 'GBRG': 0x49494949}


def lds_bytes(interp):
    lo, hi = (12, 12) if interp == BICUBIC else (8, 12)
    return 4 * (TILE[0] + lo + hi) * (TILE[1] + lo + hi)


def colour_offset(pattern, colour):
    """(row, column) of the colour in a CFA cell."""
    for p in range(4):
        if (pattern >> (2 * p)) & 3 == colour:
            return p >> 1, p & 1
    raise ValueError(hex(pattern))


def default_geometry(width, height):
    """(x0, y0, rn) as float32 values: the frame centre and the distance to the farthest corner."""
    x0, y0 = F32((width - 1) / 2), F32((height - 1) / 2)
    return x0, y0, F32(math.hypot(max(x0, width - 1 - x0), max(y0, height - 1 - y0)))


def identity_model():
    return np.array([[1, 0, 0, 1], [1, 0, 0, 1]], dtype=F32)


def _c1(t):
    return ((F32(1.25) * t - F32(2.25)) * t) * t + F32(1.0)


def _c2(t):
    return ((F32(-0.75) * t + F32(3.75)) * t - F32(6.0)) * t + F32(3.0)


def weights(a, interp):
    if interp == BICUBIC:
        return [_c2(a + F32(1.0)), _c1(a), _c1(F32(1.0) - a), _c2(F32(2.0) - a)]
    return [F32(1.0) - a, a]


def displacement(i, j, row, x0, y0, rn):
    """(dx, dy) of the sites (i, j) (integer arrays) under the model row (v, c, b), float32, clamped."""
    v, c, b = (F32(x) for x in row[:3])
    px, py = j.astype(F32) - F32(x0), i.astype(F32) - F32(y0)
    r2 = px * px + py * py
    rho = np.sqrt(r2) / F32(rn)
    s = (b * rho + c) * rho + v
    t = s - F32(1.0)
    dx, dy = px * t, py * t
    bad = ~(np.isfinite(dx) & np.isfinite(dy))
    dx, dy = np.where(bad, F32(0), dx), np.where(bad, F32(0), dy)
    d = F32(MAX_SHIFT)
    return np.minimum(np.maximum(dx, -d), d), np.minimum(np.maximum(dy, -d), d)


def correct(mosaic, pattern, model, x0, y0, rn, interp=BICUBIC, out_dtype=None):
    out_dtype = mosaic.dtype if out_dtype is None else out_dtype
    x = mosaic.astype(F32)
    out = x.copy()
    h, w = x.shape
    ph, pw = h // 2, w // 2
    lo = -1 if interp == BICUBIC else 0
    with np.errstate(all='ignore'):
        for k, colour in enumerate((0, 2)):
            if model[k, 3] == 0:
                continue
            oy, ox = colour_offset(pattern, colour)
            plane = x[oy::2, ox::2]
            i, j = np.meshgrid(np.arange(oy, h, 2), np.arange(ox, w, 2), indexing='ij')
            dx, dy = displacement(i, j, model[k], x0, y0, rn)
            moved = ~((dx == 0) & (dy == 0))
            pj, pi = j >> 1, i >> 1
            u, v = pj.astype(F32) + dx * F32(0.5), pi.astype(F32) + dy * F32(0.5)
            xf, yf = np.floor(u), np.floor(v)
            ax, ay = u - xf, v - yf
            ix, iy = xf.astype(np.int64), yf.astype(np.int64)
            wx, wy = weights(ax, interp), weights(ay, interp)
            cols = [np.clip(ix + lo + n, 0, pw - 1) for n in range(len(wx))]
            acc = None
            for m in range(len(wy)):
                rows = np.clip(iy + lo + m, 0, ph - 1)
                r = plane[rows, cols[0]] * wx[0] + plane[rows, cols[1]] * wx[1]
                if interp == BICUBIC:
                    r = (r + plane[rows, cols[2]] * wx[2]) + plane[rows, cols[3]] * wx[3]
                acc = r * wy[0] if m == 0 else acc + r * wy[m]
            out[oy::2, ox::2] = np.where(moved, acc, plane)
    return out.astype(out_dtype)


def quantise(x):
    with np.errstate(all='ignore'):
        q = np.minimum(np.maximum(np.rint(x * QSCALE), F32(0)), F32(QMAX))
    return np.where(np.isfinite(q), q, 0).astype(np.int64)


def block_sums(mosaics, pattern, clip=0.95, block=64):
    """(nby, nbx, 2, 17) int64: step 1 over all frames."""
    h, w = mosaics[0].shape
    nby, nbx = h // block, w // block
    sums = np.zeros((nby, nbx, 2, SUMS), dtype=np.int64)
    for mosaic in mosaics:
        x = mosaic.astype(F32)
        with np.errstate(all='ignore'):
            usable = np.isfinite(x) & (x < F32(clip))
        q = quantise(np.where(usable, x, F32(0)))
        for k, colour in enumerate((0, 2)):
            oy, ox = colour_offset(pattern, colour)
            i, j = np.meshgrid(np.arange(oy, h, 2), np.arange(ox, w, 2), indexing='ij')
            inside = (i >= 1) & (i <= h - 2) & (j >= 1) & (j <= w - 2) & (i < nby * block) & (j < nbx * block)
            i, j = i[inside], j[inside]
            used = usable[i, j] & usable[i, j - 1] & usable[i, j + 1] & usable[i - 1, j] & usable[i + 1, j]
            i, j = i[used], j[used]
            gl, gr, gu, gd, c = q[i, j - 1], q[i, j + 1], q[i - 1, j], q[i + 1, j], q[i, j]
            g4, gx, gy = gl + gr + gu + gd, gr - gl, gd - gu
            terms = [np.ones_like(c), j, i, g4, gx, gy, c, g4 * g4, g4 * gx, g4 * gy, g4 * c, gx * gx, gx * gy, gx * c, gy * gy, gy * c, c * c]
            for n, term in enumerate(terms):
                np.add.at(sums[:, :, k, n], (i // block, j // block), term.astype(np.int64))
    return sums


def solve3(n00, n01, n02, n11, n12, n22, r0, r1, r2):
    """(det, x0, x1, x2, C11, C22) by the cofactor formulas of the header."""
    c00, c01, c02 = n11 * n22 - n12 * n12, n02 * n12 - n01 * n22, n01 * n12 - n02 * n11
    c11, c12, c22 = n00 * n22 - n02 * n02, n01 * n02 - n00 * n12, n00 * n11 - n01 * n01
    det = (n00 * c00 + n01 * c01) + n02 * c02
    return det, _div((c00 * r0 + c01 * r1) + c02 * r2, det), _div((c01 * r0 + c11 * r1) + c12 * r2, det), _div((c02 * r0 + c12 * r1) + c22 * r2, det), c11, c22


def _div(a, b):
    """a / b as IEEE does it where Python raises."""
    if b != 0:
        return a / b
    if a == 0 or math.isnan(a):
        return math.nan
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


def block_fit(rec, noise, max_shift, x0, y0, rn):
    """Step 2 and the terms of step 3 for one record: None (dropped) or (g, h, rho, dx, dy)."""
    n = float(rec[0])
    if rec[0] < MIN_SITES:
        return None
    s1, s2, s3, s4 = (float(rec[k]) for k in (3, 4, 5, 6))
    m = [float(v) for v in rec]
    c11, c12, c13 = m[7] - (s1 * s1) / n, m[8] - (s1 * s2) / n, m[9] - (s1 * s3) / n
    c14, c22, c23 = m[10] - (s1 * s4) / n, m[11] - (s2 * s2) / n, m[12] - (s2 * s3) / n
    c24, c33, c34 = m[13] - (s2 * s4) / n, m[14] - (s3 * s3) / n, m[15] - (s3 * s4) / n
    n00, n01, n02, n11, n12, n22 = c11 / 16.0, c12 / 8.0, c13 / 8.0, c22 / 4.0, c23 / 4.0, c33 / 4.0
    r0, r1, r2 = c14 / 4.0, c24 / 2.0, c34 / 2.0
    if noise is not None:
        na, nb = noise
        q = float(QSCALE)
        nv = (q * q) * ((na * ((s1 / 4.0) / q)) + nb * n)
        n00, n11, n22 = n00 - nv / 4.0, n11 - nv / 2.0, n22 - nv / 2.0
    det, kappa, mx, my, c11_, c22_ = solve3(n00, n01, n02, n11, n12, n22, r0, r1, r2)
    dx, dy = _div(mx, kappa), _div(my, kappa)
    if not (n00 > 0 and n11 > 0 and n22 > 0 and det > 0 and c11_ > 0 and c22_ > 0 and kappa > 0 and abs(dx) <= max_shift and abs(dy) <= max_shift):
        return None
    wx, wy = det / c11_, det / c22_
    cx, cy = float(rec[1]) / n - x0, float(rec[2]) / n - y0
    rho = math.sqrt(cx * cx + cy * cy) / rn
    g = (wx * cx) * cx + (wy * cy) * cy
    hh = -((wx * cx) * dx + (wy * cy) * dy)
    return g, hh, rho, dx, dy


def fit_model(sums, x0, y0, rn, noise_model=None, fit=LINEAR, max_shift=2.0):
    """(2, 4) float32 from the block sums; noise_model: a (3, 4) array (row 1 = green: a, b, valid) or None."""
    noise = None
    if noise_model is not None and noise_model[1][2] != 0:
        noise = (float(F32(noise_model[1][0])), float(F32(noise_model[1][1])))
    x0, y0, rn, max_shift = float(F32(x0)), float(F32(y0)), float(F32(rn)), float(F32(max_shift))
    model = np.zeros((2, 4), dtype=F32)
    records = sums.reshape(-1, 2, SUMS)
    for k in range(2):
        a = [0.0] * 9
        count = 0
        for rec in records[:, k]:
            kept = block_fit(rec, noise, max_shift, x0, y0, rn)
            if kept is None:
                continue
            g, h, rho = kept[:3]
            phi = (1.0, rho, rho * rho)
            for e, (pa, pb) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
                a[e] += (g * phi[pa]) * phi[pb]
            for e in range(3):
                a[6 + e] += h * phi[e]
            count += 1
        if fit == LINEAR:
            e, c, b = _div(a[6], a[0]), 0.0, 0.0
            ok = count >= 1 and a[0] > 0
        else:
            det, e, c, b, _, _ = solve3(*a)
            ok = count >= 3 and det > 0
        with np.errstate(all='ignore'):
            row = np.array([1.0 + e, c, b], dtype=np.float64).astype(F32)
        ok = ok and bool(np.all(np.isfinite(row)))
        model[k] = (*row, 1) if ok else (1, 0, 0, 0)
    return model


def estimate(mosaics, pattern, x0, y0, rn, noise_model=None, fit=LINEAR, clip=0.95, block=64, max_shift=2.0):
    """(model, sums)"""
    sums = block_sums(mosaics, pattern, clip, block)
    return fit_model(sums, x0, y0, rn, noise_model, fit, max_shift), sums


def corner_shift(row, x0, y0, rn, width, height):
    """(s - 1) * the distance from the centre to the farthest corner, in sites, float64."""
    r = math.hypot(max(float(x0), width - 1 - float(x0)), max(float(y0), height - 1 - float(y0)))
    rho = r / float(rn)
    return r * ((float(row[0]) - 1.0) + float(row[1]) * rho + float(row[2]) * rho * rho)
