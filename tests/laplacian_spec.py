"""The local Laplacian filter as a specification: float64 arithmetic, explicit binary16 rounding at every store, whole-array
numpy operations.  Plain numpy: nothing of the product, no torch.

Written from the reference's formulas (csrc/local_contrast/laplacian.cu:50-66 sizes and boundary clamp, :111-141 expand,
:177-207 reduce, :221-252 assemble, :266-290 curve, :482-592 sequencing): coordinate arrays and gathers
instead of per-pixel loops, float64 instead of float32.  It shares no code with the C oracle (oracle/src/laplacian.c); on finite
data the two can differ only where the oracle's fp32 rounding moves a value across a binary16 rounding boundary.

Non-finite values travel as in the reference:
  * a store rounds to binary16, so a value beyond 65504 becomes +-inf there (`astype(float16)`);
  * `expand` sums only the taps the reference's loops visit -- three (1 6 1) at an even coordinate, two (4 4) at an odd one, per
    axis -- so a NaN or an infinity in a cell that is not visited does not reach the result;
  * the curve always adds clarity * c * exp(...), also when clarity is 0: 0 * inf and 0 * NaN are NaN, so a non-finite input
    sample is a NaN in all six gamma pyramids whatever the settings;
  * the blend weight a = fmin(fmax(., 0), 1) maps NaN to 0 as C's fmaxf does.

`laplacian_spec` also returns a per-pixel scale s: the largest magnitude among the five terms the level-0 assemble sums for that
pixel -- expand(output level 1), the two bracketing gamma pyramids' level-0 values and their level-1 expansions.  Where the result
is a small difference of large pyramid values (inputs far outside [0, 1], sigma far above the data's range), one binary16 ulp of
the RESULT says nothing about the rounding that went into it; one binary16 ulp of s does."""

import numpy as np

NG = 6
K5 = np.array([1, 4, 6, 4, 1], np.float64) / 16


def h16(a):
    with np.errstate(over='ignore', invalid='ignore'):
        return np.asarray(a).astype(np.float16).astype(np.float64)  # write_imagef_half: every stored value is binary16


def dl(x, level):
    return (x + (1 << level) - 1) >> level


def gamma_centre(k):
    return np.float64((np.float32(k) + np.float32(0.5)) / np.float32(NG))  # the reference forms g in fp32


def reduce_half(fine, cw, ch):
    """5x5 binomial at 2c with c = the coarse position clamped to [1, size - 2] (laplacian.cu:177-207).  All 25 taps are read."""
    cx = np.clip(np.arange(cw), 1, cw - 2)
    cy = np.clip(np.arange(ch), 1, ch - 2)
    acc = np.zeros((ch, cw))
    with np.errstate(invalid='ignore'):
        for j in range(-2, 3):
            for i in range(-2, 3):
                acc += fine[(2 * cy + j)[:, None], (2 * cx + i)[None, :]] * (K5[i + 2] * K5[j + 2])
    return h16(acc)


def expand(coarse, qx, qy):
    """4 x (binomial taps of the zero-stuffed coarse level): 3 taps (1, 6, 1)/16 at an even coordinate, 2 taps (4, 4)/16 at
    an odd one (laplacian.cu:111-141); qx / qy are coordinate arrays.  A tap the reference's loops skip is not summed."""
    def taps(q):
        odd = (q & 1) == 1
        w = np.where(odd[None, :], np.array([0.0, 4.0, 4.0])[:, None], np.array([1.0, 6.0, 1.0])[:, None]) / 16  # offsets -1, 0, +1
        used = np.stack([~odd, np.ones_like(odd), np.ones_like(odd)])
        return q // 2, w, used
    cx, wx, ux = taps(qx)
    cy, wy, uy = taps(qy)
    out = np.zeros((qy.size, qx.size))
    with np.errstate(invalid='ignore'):
        for j in (-1, 0, 1):
            for i in (-1, 0, 1):
                wgt = wy[j + 1][:, None] * wx[i + 1][None, :]
                # a skipped tap may point outside the level (offset -1 at coordinate 0 is never visited: q >= 1); the clip keeps the gather legal
                cell = coarse[np.clip(cy + j, 0, coarse.shape[0] - 1)[:, None], np.clip(cx + i, 0, coarse.shape[1] - 1)[None, :]]
                out += np.where(uy[j + 1][:, None] & ux[i + 1][None, :], wgt * cell, 0.0)
    return 4.0 * out


def clamp_boundary(n):
    """The fine coordinate an expand is evaluated at (laplacian.cu:53-65): [1, n - 2] for odd n, [1, n - 3] for even n."""
    q = np.arange(n)
    q = np.minimum(q, n - 2 if n & 1 else n - 3)
    return np.maximum(q, 1)


def curve(x, g, sigma, shadows, highlights, clarity):
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        c = x - g
        pos = c > 0
        ssigma = np.where(pos, sigma, -sigma)
        shadhi = np.where(pos, shadows, highlights)
        lin = g + ssigma + shadhi * (c - ssigma)
        t = np.clip(c / (2.0 * ssigma), 0.0, 1.0)
        bez = g + ssigma * 2.0 * (1.0 - t) * t + t * t * (ssigma + ssigma * shadhi)
        val = np.where(np.abs(c) > 2 * sigma, lin, bez)
        return val + clarity * c * np.exp(-c * c / (2.0 * sigma * sigma / 3.0))  # added for every clarity: 0 * inf is NaN


def laplacian_spec(lum, sigma, shadows, highlights, clarity):
    """(result, s): the filter's result as float64 holding binary16 values, and the scale of the level-0 sum (module docstring)."""
    H, W = lum.shape
    L = min(30, int(np.floor(np.log2(min(W, H)))))
    pad = 1 << (L - 1)
    bw, bh = W + 2 * pad, H + 2 * pad
    size = [(dl(bh, l), dl(bw, l)) for l in range(L)]
    ys, xs = np.clip(np.arange(bh) - pad, 0, H - 1), np.clip(np.arange(bw) - pad, 0, W - 1)
    padded = [h16(lum.astype(np.float64)[ys[:, None], xs[None, :]])]
    for l in range(1, L):
        padded.append(reduce_half(padded[l - 1], size[l][1], size[l][0]))
    proc = []
    for k in range(NG):
        p = [h16(curve(padded[0], gamma_centre(k), sigma, shadows, highlights, clarity))]
        for l in range(1, L):
            p.append(reduce_half(p[l - 1], size[l][1], size[l][0]))
        proc.append(p)
    out = [None] * L
    out[L - 1] = padded[L - 1]                      # the coarsest gaussian level lives in the output pyramid (:526)
    s = None
    with np.errstate(invalid='ignore', over='ignore'):
        for l in range(L - 2, -1, -1):
            ph, pw = size[l]
            qx, qy = clamp_boundary(pw), clamp_boundary(ph)
            v = padded[l]
            hi = np.ones(v.shape, int)
            for h in range(1, NG - 1):                  # hi advances while (hi + .5) / NG <= v; a NaN fails the first compare
                hi += (hi == h) & (gamma_centre(h) <= v)
            lo = hi - 1
            a = np.fmin(np.fmax(v * NG - (lo + 0.5), 0.0), 1.0)
            fine = np.stack([proc[k][l] for k in range(NG)])
            up = np.stack([expand(proc[k][l + 1], qx, qy) for k in range(NG)])
            yy, xx = np.mgrid[0:ph, 0:pw]
            f0, f1, u0, u1 = fine[lo, yy, xx], fine[lo + 1, yy, xx], up[lo, yy, xx], up[lo + 1, yy, xx]
            e = expand(out[l + 1], qx, qy)
            out[l] = h16(e + (f0 - u0) * (1.0 - a) + (f1 - u1) * a)
            if l == 0:
                s = np.max(np.abs(np.stack([e, f0, u0, f1, u1])), axis=0)
    return out[0][pad:pad + H, pad:pad + W], s[pad:pad + H, pad:pad + W]


def laplacian_fp64(lum, sigma, shadows, highlights, clarity):
    return laplacian_spec(lum, sigma, shadows, highlights, clarity)[0]


def half_ulp_of(v):
    """One binary16 ulp of |v| (the subnormal spacing 2^-24 below 2^-14)."""
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -14)))
    return 2.0 ** (e - 10)
