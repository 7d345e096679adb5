"""NumPy restatement of include/tdk_hip_hdr.h: what tdk_hdr_merge must compute, to the last bit of the output and the last byte of the
mask.  float32 operation by operation, one rounding each.  Shared by test_hdrmerge_spec.py (which holds this file to literal per-site
loops and to the algorithm's purpose) and test_gpu_hdrmerge.py (which holds the kernel to this file)."""

import numpy as np

from temporal_spec import BGGR, GBRG, GRBG, RGGB, rows_of, window_sums  # noqa: F401  (the same colours and the same window rule)

F = np.float32
MAX_FRAMES = 8
TILE = (32, 32)   # TDK_HDR_TILE_W, TDK_HDR_TILE_H


def lds_bytes(r):
    """Two staged planes with four columns either side, two planes of row sums, the clip bytes with a row more either side, 96 bytes of
    addresses and ratios."""
    tw, th = TILE
    return 4 * (2 * (th + 2 * r) * (tw + 8) + 2 * (th + 2 * r) * tw) + (th + 2 * r + 2) * (tw + 8) + 96


def parameters(clip=0.95, thresholds=(1.5, 3.0), pixel_threshold=4.0, variance_floor=1e-12):
    """(clip, t_hi, inv, c2, v_min) as the float32 numbers the kernel is given."""
    t_lo, t_hi = F(thresholds[0]), F(thresholds[1])
    inv = F(1.0) / (t_hi - t_lo)
    c2 = F(np.inf) if pixel_threshold is None else F(pixel_threshold) * F(pixel_threshold)
    return F(clip), t_hi, inv, c2, F(variance_floor)


def ratios(exposures, ref=-1):
    """(k, lo, ref): the exposure ratios, the shortest frame and the resolved reference frame."""
    e = np.asarray(exposures, F)
    lo = hi = 0
    for f in range(1, e.size):
        if e[f] < e[lo]:
            lo = f
        if e[f] > e[hi]:
            hi = f
    with np.errstate(all='ignore'):
        k = (e / e[lo]).astype(F)
    return k, lo, (hi if ref is None or ref < 0 else int(ref))


def saturated(x, clip):
    """sat_f(q) of one frame: the OR of !(x < clip) over the in-frame sites of the 3 x 3."""
    with np.errstate(invalid='ignore'):
        c = ~(x < clip)
    h, w = c.shape
    pad = np.zeros((h + 2, w + 2), bool)
    pad[1:-1, 1:-1] = c
    out = np.zeros((h, w), bool)
    for di in range(3):
        for dj in range(3):
            out |= pad[di:di + h, dj:dj + w]
    return out


def merge(frames, exposures, model, pattern, ref=-1, radius=2, clip=0.95, thresholds=(1.5, 3.0), pixel_threshold=4.0, variance_floor=1e-12, out_dtype=None):
    """One call of tdk_hdr_merge: (out, mask)."""
    frames = [np.asarray(x) for x in frames]
    nf = len(frames)
    assert 2 <= nf <= MAX_FRAMES
    out_dtype = frames[0].dtype if out_dtype is None else out_dtype
    clip, t_hi, inv, c2, v_min = parameters(clip, thresholds, pixel_threshold, variance_floor)
    k, lo, ref = ratios(exposures, ref)
    x = [f.astype(F) for f in frames]
    shape = x[0].shape
    model = np.asarray(model, F)
    row = rows_of(shape, pattern)
    valid = (model[:, 2] != 0)[row]
    a = np.where(valid, model[:, 0][row], F(1.0)).astype(F)
    b = np.where(valid, model[:, 1][row], F(0.0)).astype(F)
    with np.errstate(all='ignore'):
        sat = [saturated(xf, clip) for xf in x]
        # the anchor
        best = np.full(shape, -1, np.int64)
        bk = np.zeros(shape, F)
        for f in range(nf):
            take = ~sat[f] & ((best < 0) | (k[f] > bk))
            best = np.where(take, f, best)
            bk = np.where(take, k[f], bk).astype(F)
        g = np.where(~sat[ref], ref, best)
        blown = g < 0
        g = np.where(blown, lo, g)
        kg = k[g]
        xg = np.choose(g, x).astype(F)
        R = xg / kg
        Rp = np.fmax(R, F(0.0))

        def u_of(kf):
            var = np.fmax(a * (Rp * kf) + b, v_min)
            return var / (kf * kf)

        ug = u_of(kg)
        num, den = np.zeros(shape, F), np.zeros(shape, F)
        count = np.zeros(shape, np.int64)
        for f in range(nf):
            r = x[f] / k[f]
            u = u_of(k[f])
            d = r - R
            out_of_it = sat[f] | blown | (g == f)
            eps = np.where(out_of_it, F(0.0), d * d).astype(F)
            v = np.where(out_of_it, F(0.0), u + ug).astype(F)
            t = window_sums(eps, radius) / window_sums(v, radius)
            s = np.fmin(np.fmax((t_hi - t) * inv, F(0.0)), F(1.0))
            s = np.where(eps > c2 * v, F(0.0), s)
            s = np.where(~valid | (g == f), F(1.0), s).astype(F)
            w = np.where(sat[f], F(0.0), s / u).astype(F)
            on = w > 0
            num = np.where(on, num + w * r, num).astype(F)
            den = np.where(on, den + w, den).astype(F)
            count += on
        out = np.where(den > 0, num / den, R).astype(F)
        mask = (g | np.where(blown, 8, 0) | (count << 4)).astype(np.uint8)
        return out.astype(out_dtype), mask
