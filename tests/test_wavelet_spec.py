"""CPU-only: the specification of the wavelet denoiser (head comment of include/tdk_hip_wavelet.h) restated in NumPy float32,
`wavelet_ref`, which tests/test_gpu_wavelet.py holds the kernels to bit for bit -- and what pins the restatement itself: an
independent float64 computation, a frame on which every intermediate is exact, the band norms, a noise calibration, and the rule
that indices are clamped at every scale."""

import ctypes

import numpy as np
import pytest

F = np.float32
TAPS = (0.0625, 0.25, 0.375, 0.25, 0.0625)
RADIUS = 62   # 2 * (1 + 2 + 4 + 8 + 16): the support of five scales on each side


def _blur_axis(c, p, axis, f):
    """h = (0.0625*(c[-2p] + c[+2p]) + 0.25*(c[-p] + c[+p])) + 0.375*c[0] along one axis, indices clamped to the frame."""
    n = c.shape[axis]
    idx = np.arange(n)

    def tap(k):
        return np.take(c, np.clip(idx + k * p, 0, n - 1), axis=axis)

    outer = tap(-2) + tap(2)
    inner = tap(-1) + tap(1)
    a = f(0.0625) * outer
    b = f(0.25) * inner
    s = a + b
    m = f(0.375) * c
    return s + m


def bands(v, scales, f=F):
    """([d_0 .. d_{S-1}], c_S) of a working-space frame (H, W, K); every temporary has the type f."""
    c = v.astype(f)
    d = []
    for s in range(scales):
        h = _blur_axis(c, 1 << s, 1, f)       # horizontal
        n = _blur_axis(h, 1 << s, 0, f)       # vertical
        d.append(c - n)
        c = n
    return d, c


def shrink(d, t):
    ad = np.abs(d)
    return np.where(ad > t, np.copysign(ad - t, d), d.dtype.type(0))


def forward(x, ycc, f=F):
    x = x.astype(f)
    if not ycc:
        return x
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    y = (f(0.25) * r + f(0.5) * g) + f(0.25) * b
    return np.stack([y, b - g, r - g], axis=-1)


def inverse(v, ycc, f=F):
    if not ycc:
        return v
    y, cb, cr = v[..., 0], v[..., 1], v[..., 2]
    g = y - f(0.25) * (cb + cr)
    return np.stack([cr + g, g, cb + g], axis=-1)


def wavelet_ref(x, thresholds, ycc=False, f=F):
    """x: (H, W, C) float32 or float16; thresholds: (S, C) -> the result in x's type.  With f = float64 the same expression tree
    without the float32 roundings (and the float64 result)."""
    t = np.asarray(thresholds, dtype=F).astype(f)
    assert t.ndim == 2 and t.shape[1] == x.shape[2]
    d, c = bands(forward(x, ycc, f), t.shape[0], f)
    acc = shrink(d[0], t[0])
    for s in range(1, t.shape[0]):
        acc = acc + shrink(d[s], t[s])
    y = inverse(acc + c, ycc, f)
    assert y.dtype == f
    return y if f is not F else y.astype(x.dtype)   # binary16: round to nearest even, no clamp


# ------------------------------------------------------------------ an independent float64 computation
def _operator(n, p):
    """The clamped 5-tap filter at step p as an n x n matrix."""
    m = np.zeros((n, n))
    for i in range(n):
        for k, w in zip((-2, -1, 0, 1, 2), TAPS):
            m[i, min(max(i + k * p, 0), n - 1)] += w
    return m


def float64_wavelet(x, thresholds, ycc):
    """Matrix form: c_{s+1} = V_p c_s H_p^T per channel.  Returns (result, the largest |intermediate|)."""
    x = x.astype(np.float64)
    if ycc:
        r, g, b = x[..., 0], x[..., 1], x[..., 2]
        v = np.stack([0.25 * r + 0.5 * g + 0.25 * b, b - g, r - g], axis=-1)
    else:
        v = x
    t = np.asarray(thresholds, dtype=F).astype(np.float64)
    height, width = x.shape[:2]
    c, acc, big = v, np.zeros_like(v), np.abs(v).max()
    for s in range(t.shape[0]):
        hm, vm = _operator(width, 1 << s), _operator(height, 1 << s)
        n = np.einsum('ij,jkc->ikc', vm, np.einsum('ijc,kj->ikc', c, hm))
        d = c - n
        acc = acc + np.sign(d) * np.maximum(np.abs(d) - t[s], 0.0)
        big = max(big, np.abs(d).max(), np.abs(acc).max(), np.abs(n).max())
        c = n
    y = acc + c
    if ycc:
        g = y[..., 0] - 0.25 * (y[..., 1] + y[..., 2])
        y = np.stack([y[..., 2] + g, g, y[..., 1] + g], axis=-1)
    return y, max(big, np.abs(y).max())


@pytest.mark.parametrize('ycc', [False, True])
@pytest.mark.parametrize('scales', [1, 3, 5])
def test_restatement_against_float64(scales, ycc):
    rng = np.random.default_rng(10 * scales + ycc)
    x = rng.random((45, 70, 3), dtype=F)
    t = (rng.random((scales, 3)) * 0.02).astype(F)
    got = wavelet_ref(x, t, ycc).astype(np.float64)
    want, big = float64_wavelet(x, t, ycc)
    # Roundings on the path to one output.  A pass is 3 products and 4 sums = 7, a scale 14, and the filter is a convex combination, so
    # c_s carries at most 14 s roundings of its inputs' range.  d_s = c_s - c_{s+1} carries those of both plus its own; the shrinkage
    # is 1-Lipschitz and adds one subtraction; the sum adds one per band: band s gives 14 s + 14 (s + 1) + 3.  y adds c_S (14 S) and one
    # sum; the colour transform 4 roundings in and 4 out, each of which a filter or the inverse passes on at most twice.
    # Every rounding is at most 2^-24 of the value it rounds, and no intermediate exceeds R = 2 (asserted on the float64 run).
    ops = sum(14 * s + 14 * (s + 1) + 3 for s in range(scales)) + 14 * scales + 1 + (16 if ycc else 0)
    R = 2.0
    assert big <= R
    tol = ops * 2.0 ** -24 * R
    err = np.abs(got - want).max()
    print(f'S={scales} ycc={ycc}: max error {err:.3e}, tolerance {tol:.3e} ({ops} roundings)')
    assert err <= tol


def test_exact_on_a_dyadic_frame():
    """Integers 0..15 times 2^-4 through two scales: a pass divides the resolution by at most 16 (the tap 0.0625), so after four
    passes every value is a multiple of 2^-20 below 1 in magnitude -- 20 bits, and every sum and difference of two of them has 21:
    float32 holds each intermediate exactly and agrees with float64 to the bit.  (Without the colour transform, and no more scales:
    either would need more bits than float32 has.)"""
    rng = np.random.default_rng(3)
    x = (rng.integers(0, 16, (40, 37, 1)) / 16.0).astype(F)
    d, _ = bands(x, 2)
    d64, _ = bands(x, 2, np.float64)
    for a, b in zip(d, d64):
        assert np.array_equal(a.astype(np.float64), b)
    # a sample of each band whose magnitude becomes the band's threshold: |d| == t gives 0 there
    spots = []
    for s in range(2):
        ys, xs, _ = np.nonzero(d[s][8:-8, 8:-8])
        spots.append((ys[s] + 8, xs[s] + 8))
    at = np.array([[abs(d[s][spots[s]][0])] for s in range(2)], dtype=F)
    below = at - F(2.0 ** -20)                # |d| is one step of the frame's 2^-20 lattice above this threshold (a finer step leaves the lattice)
    assert (below > 0).all() and np.array_equal(below.astype(np.float64), at.astype(np.float64) - 2.0 ** -20)
    for t, name in ((at, 'equal'), (below, 'one step above')):
        got = wavelet_ref(x, t)
        want = wavelet_ref(x, t, f=np.float64)
        assert got.dtype == F and np.array_equal(got.astype(np.float64), want), name
        for s in range(2):
            v = d[s][spots[s]][0]
            kept = shrink(d[s], t[s])[spots[s]][0]
            if name == 'equal':
                assert kept == 0 and v != 0
            else:
                assert abs(kept) == F(2.0 ** -20) and np.signbit(kept) == np.signbit(v)
    # and the thresholds change the result: the two runs differ where a coefficient survives
    assert not np.array_equal(wavelet_ref(x, at), wavelet_ref(x, below))


def test_band_norms(td):
    from torch_darktable._native import lib

    x = np.zeros((129, 129, 1))
    x[64, 64, 0] = 1.0
    d, _ = bands(x, 5, np.float64)            # the restatement in float64: the impulse response of each band, clear of the borders
    want = [F(np.sqrt((b * b).sum())) for b in d]
    for scales in range(1, 6):
        buf = (ctypes.c_float * 5)(*([7.0] * 5))
        assert lib.tdk_wavelet_band_norms(scales, buf) == 0
        assert [F(v) for v in buf[:scales]] == want[:scales], (scales, list(buf), want)
        assert all(v == 0.0 for v in buf[scales:])
    assert lib.tdk_wavelet_band_norms(0, buf) == 1 and lib.tdk_wavelet_band_norms(6, buf) == 1 and b'scales' in lib.tdk_last_error()
    assert lib.tdk_wavelet_band_norms(3, None) == 1 and b'null pointer' in lib.tdk_last_error()
    from torch_darktable.wavelet import band_norms
    assert band_norms(5) == tuple(float(v) for v in want)
    print('band norms', [float(v) for v in want])


def test_noise_calibration():
    """White noise of sigma in c_0 leaves sigma * n_s in d_s."""
    sigma, size, scales = 0.01, 1024, 5
    rng = np.random.default_rng(5)
    x = (0.5 + sigma * rng.standard_normal((size, size, 1))).astype(F)
    d, _ = bands(x, scales)
    imp = np.zeros((129, 129, 1))
    imp[64, 64, 0] = 1.0
    norms = [np.sqrt((b * b).sum()) for b in bands(imp, scales, np.float64)[0]]
    for s in range(scales):
        inner = d[s][RADIUS:-RADIUS, RADIUS:-RADIUS, 0].astype(np.float64)
        got = inner.std()
        # The standard deviation of N independent Gaussian samples has the relative standard error 1 / sqrt(2 N).  The coefficients
        # of band s are correlated over the band's support, about 4 * 2^s pixels on each axis, so N counts one sample per (4 * 2^s)^2
        # pixels; five standard errors.  (The float32 roundings, 2^-24 * 0.5, are far below sigma * n_s >= 1e-4.)
        n_eff = inner.size / (4 << s) ** 2
        tol = 5.0 / np.sqrt(2.0 * n_eff)
        print(f'band {s}: std {got:.4e}, sigma * n_s {sigma * norms[s]:.4e}, relative tolerance {tol:.3f}')
        assert abs(got / (sigma * norms[s]) - 1.0) <= tol


def test_indices_are_clamped_at_every_scale():
    """The trap: c_{s+1} at a clamped index is the value at the edge pixel.  Replicating the frame once by the whole support,
    filtering and cropping computes a filter of replicated c_s beyond the edge instead: the same at scale 0, different from scale 1 on."""
    rng = np.random.default_rng(7)
    x = rng.random((150, 140, 1), dtype=F)
    d, c = bands(x, 3)
    padded = np.pad(x, ((RADIUS, RADIUS), (RADIUS, RADIUS), (0, 0)), mode='edge')
    dp, cp = bands(padded, 3)
    crop = (slice(RADIUS, -RADIUS), slice(RADIUS, -RADIUS))
    assert np.array_equal(d[0], dp[0][crop])                       # c_1: one filter of replicated c_0 is the rule itself
    for s in (1, 2):
        assert not np.array_equal(d[s], dp[s][crop]), s
        far = 2 * ((2 << s) - 1)                                   # the support of scales 0..s: beyond it no edge is seen
        assert np.array_equal(d[s][far:-far, far:-far], dp[s][crop][far:-far, far:-far]), s
        assert not np.array_equal(d[s][:far], dp[s][crop][:far]), s
    assert not np.array_equal(c, cp[crop])
