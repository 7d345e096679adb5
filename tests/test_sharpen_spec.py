"""CPU-only: the specification of the sharpener (head comment of include/tdk_hip_sharpen.h) as a NumPy float32 restatement,
`sharpen_ref`, which tests/test_gpu_sharpen.py holds the kernel to bit for bit.

NumPy's float32 element-wise + - * are single correctly rounded IEEE operations and are never fused, so writing the header's
formulas operation by operation reproduces the kernel's arithmetic (the library is built with -ffp-contract=off).

Second source.  `sharpen_ref` is checked against an independent float64 computation: torch's CPU conv2d on the replicate-padded
frame for the two blur passes, float64 for everything after.  Both use the same float32 tap values, inputs and threshold, so the
difference is the float32 rounding of the restatement alone.  With u = 2^-24, M = max|x|, a = amount:
  signal   the channel itself: exact.  Luminance: 3 products and 2 sums of magnitude <= M:               E_s  = 5 u M  (else 0)
  blur     per pass, the R + 1 products, R pair sums and R accumulations are counted as (2 R + 4) roundings of the largest
           magnitude M (the taps sum to 1, so every partial sum is <= M); the second pass hands the first one's error on with
           weights that sum to 1:                                                                          E_b  = 2 (2 R + 4) u M + E_s
  detail   d = s - b, |d| <= 2 M, one rounding:                                                            E_d  = E_s + E_b + 2 u M
  shrink   |d| - t is one more rounding, the rule is 1-Lipschitz:                                          E_d' = E_d + 2 u M
  result   a * d' rounds once (<= 2 a M), x + a d' once (<= (1 + 2 a) M):                                   E_y  = a E_d' + 2 a u M + (1 + 2 a) u M
Terms of order u^2 are left out (below 1e-5 of the bound).  Measured on the cases below: at most 0.14 of E_y."""
import ctypes
import math
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
F = np.float32
U = 2.0 ** -24
LUMA_WEIGHTS = (F(0.2126729), F(0.7151522), F(0.0721750))


def gaussian_weights(sigma):
    """The formula of tdk_sharpen_weights in NumPy float64, rounded once to float32: (w0 .. wR), R = ceil(3 sigma)."""
    s = float(F(sigma))
    radius = math.ceil(3.0 * s)
    w = np.exp(-np.arange(radius + 1, dtype=np.float64) ** 2 / (2.0 * s * s))
    return tuple((w / (w[0] + 2.0 * w[1:].sum())).astype(F))


def _shift(a, k, axis):
    """a[i + k] along `axis`, the index clamped to the frame (replicate)."""
    n = a.shape[axis]
    return np.take(a, np.clip(np.arange(n) + k, 0, n - 1), axis=axis)


def blur_ref(s, w, axis):
    h = w[0] * s
    for k in range(1, len(w)):
        h = h + w[k] * (_shift(s, -k, axis) + _shift(s, k, axis))
    return h


def extrema3x3(xf):
    shifted = [_shift(_shift(xf, dy, 0), dx, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    return np.minimum.reduce(shifted), np.maximum.reduce(shifted)


def sharpen_ref(x, weights, amount=0.5, threshold=0.0, luma=False, overshoot=None):
    """x: (H, W, C) float32, float16 or uint8; the same type out.  `luma` must be False for C = 1 (the C entry point rejects it)."""
    assert x.ndim == 3 and x.dtype in (np.float32, np.float16, np.uint8) and not (luma and x.shape[2] != 3)
    if amount == 0:
        return x.copy()
    w = [F(v) for v in weights]
    scale = F(255.0) if x.dtype == np.uint8 else F(1.0)
    xf = x.astype(F)
    if luma:
        s = ((LUMA_WEIGHTS[0] * xf[:, :, 0] + LUMA_WEIGHTS[1] * xf[:, :, 1]) + LUMA_WEIGHTS[2] * xf[:, :, 2])[:, :, None]
    else:
        s = xf
    b = blur_ref(blur_ref(s, w, 1), w, 0)
    d = s - b
    t = F(threshold) * scale
    ad = np.abs(d)
    dp = np.where(ad > t, np.copysign(ad - t, d), F(0.0)).astype(F)
    y = xf + F(amount) * dp
    if overshoot is not None:
        lo, hi = extrema3x3(xf)
        o = F(overshoot) * scale
        y = np.minimum(np.maximum(y, lo - o), hi + o)
    assert y.dtype == F and s.dtype == F and b.dtype == F
    if x.dtype == np.uint8:
        return np.rint(np.clip(y, F(0.0), F(255.0))).astype(np.uint8)
    return y.astype(x.dtype)


def sharpen_f64(x, weights, amount, threshold, luma):
    """The independent computation: float64, the blur by torch's conv2d on a replicate-padded frame.  float32 input."""
    import torch
    import torch.nn.functional as nnf

    xd = torch.from_numpy(x.astype(np.float64))
    if luma:
        s = (float(LUMA_WEIGHTS[0]) * xd[:, :, 0] + float(LUMA_WEIGHTS[1]) * xd[:, :, 1] + float(LUMA_WEIGHTS[2]) * xd[:, :, 2])[:, :, None]
    else:
        s = xd
    radius = len(weights) - 1
    taps = torch.tensor([float(F(v)) for v in weights], dtype=torch.float64)
    kernel = torch.cat([taps.flip(0)[:-1], taps])
    planes = s.permute(2, 0, 1)[:, None]                                     # (signals, 1, H, W)
    padded = nnf.pad(planes, (radius, radius, radius, radius), mode='replicate')
    b = nnf.conv2d(nnf.conv2d(padded, kernel.view(1, 1, 1, -1)), kernel.view(1, 1, -1, 1))[:, 0].permute(1, 2, 0)
    d = s - b
    t = float(F(threshold))
    dp = torch.where(d.abs() > t, torch.sign(d) * (d.abs() - t), torch.zeros_like(d))
    return (xd + float(F(amount)) * dp).numpy()


def bound_f32(radius, amount, xmax, luma):
    e_s = 5 * U * xmax if luma else 0.0
    e_b = 2 * (2 * radius + 4) * U * xmax + e_s
    e_d = e_s + e_b + 2 * U * xmax
    e_dp = e_d + 2 * U * xmax
    return amount * e_dp + 2 * amount * U * xmax + (1 + 2 * amount) * U * xmax


def rand_f(shape, seed):
    return np.random.default_rng(seed).random(shape, dtype=F)


def rand_u8(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


# ------------------------------------------------------------------ second source
@pytest.mark.parametrize('sigma', [0.25, 1.0, 4.0])
@pytest.mark.parametrize('c,luma', [(1, False), (3, False), (3, True)])
def test_restatement_agrees_with_float64_conv2d(sigma, c, luma):
    w = gaussian_weights(sigma)
    for xscale, amount, threshold, seed in ((1.0, 0.5, 0.0, 1), (1.0, 4.0, 0.02, 2), (255.0, 1.5, 3.0, 3)):
        x = (rand_f((61, 83, c), seed + c) * F(xscale)).astype(F)
        got = sharpen_ref(x, w, amount, threshold, luma).astype(np.float64)
        want = sharpen_f64(x, w, amount, threshold, luma)
        tol = bound_f32(len(w) - 1, amount, float(np.abs(x).max()), luma)
        err = float(np.abs(got - want).max())
        print(f'sharpen_ref vs float64: sigma {sigma} C {c} luma {luma} amount {amount}: err {err:.3e} bound {tol:.3e} ({err / tol:.3f} of it)')
        assert err <= tol, (sigma, c, luma, amount, err, tol)


def test_threshold_and_limit_follow_their_formulas_in_float64():
    """The two branches the conv2d comparison leaves alone: pixels on both sides of the threshold exist in its cases, and the
    halo limit is exact arithmetic on the result (minimum, maximum, one rounding each for lo - o and hi + o)."""
    x = rand_f((40, 50, 3), 9)
    w = gaussian_weights(1.0)
    d = x - blur_ref(blur_ref(x, w, 1), w, 0)
    assert (np.abs(d) > 0.02).any() and (np.abs(d) <= 0.02).any()
    free = sharpen_ref(x, w, 4.0, 0.02, False)
    held = sharpen_ref(x, w, 4.0, 0.02, False, overshoot=0.05)
    lo, hi = extrema3x3(x)
    assert np.array_equal(held, np.minimum(np.maximum(free, lo - F(0.05)), hi + F(0.05)))
    assert (held != free).any()


# ------------------------------------------------------------------ weights
@pytest.mark.parametrize('sigma', [0.25, 1.0 / 3.0, 0.5, 1.0, 1.7, 2.0, 3.999, 4.0])
def test_weights_equal_the_numpy_formula(td, sigma):
    from torch_darktable._native import lib

    buf, radius = (ctypes.c_float * 13)(*([7.0] * 13)), ctypes.c_int(-1)
    assert lib.tdk_sharpen_weights(sigma, buf, ctypes.byref(radius)) == 0, lib.tdk_last_error()
    want = gaussian_weights(sigma)
    r = radius.value
    assert r == len(want) - 1 == math.ceil(3.0 * float(F(sigma))) and 1 <= r <= 12
    got = np.array(buf[: r + 1], dtype=F)
    assert (np.abs(got.astype(np.float64) - np.array(want, np.float64)) <= np.spacing(np.array(want, F))).all(), (got, want)   # one ulp per weight
    assert all(v == 0.0 for v in buf[r + 1:])
    total = float(got[0]) + 2.0 * float(got[1:].astype(np.float64).sum())
    assert abs(total - 1.0) <= (r + 1) * 2.0 ** -23, total
    assert (np.diff(got) < 0).all() and got[-1] >= 0


def test_radius_is_ceil_3_sigma(td):
    """sigma is a float32: 1/3 rounds up to 0.33333334, so 3 sigma > 1 and R = 2."""
    assert [len(gaussian_weights(s)) - 1 for s in (0.25, 1.0 / 3.0, 1.0, 4.0)] == [1, 2, 3, 12]
    cuda = __import__('torch').device('cuda', 0)
    for sigma, radius in ((0.25, 1), (1.0 / 3.0, 2), (1.0, 3), (4.0, 12)):
        s = td.Sharpen(cuda, sigma=sigma)
        assert s.radius == radius and s.weights == tuple(float(v) for v in gaussian_weights(sigma))


def test_weights_argument_errors(td):
    from torch_darktable._native import lib

    buf, radius = (ctypes.c_float * 13)(), ctypes.c_int(0)
    for sigma in (0.2499, 4.001, 0.0, -1.0, float('nan'), float('inf')):
        assert lib.tdk_sharpen_weights(sigma, buf, ctypes.byref(radius)) == 1 and b'sigma' in lib.tdk_last_error(), sigma
    assert lib.tdk_sharpen_weights(1.0, None, ctypes.byref(radius)) == 1 and b'null pointer' in lib.tdk_last_error()
    assert lib.tdk_sharpen_weights(1.0, buf, None) == 1 and b'null pointer' in lib.tdk_last_error()


def test_tile_matches_the_kernel_source(td):
    text = (ROOT / 'torch-darktable_amd' / 'csrc' / 'sharpen.hip').read_text()
    tw, th = re.search(r'constexpr int SH_TW = (\d+), SH_TH = (\d+)', text).groups()
    assert td.Sharpen.TILE == (int(tw), int(th))


# ------------------------------------------------------------------ properties of the operator
FRAMES = {np.float32: lambda shape, seed: rand_f(shape, seed), np.float16: lambda shape, seed: rand_f(shape, seed).astype(np.float16),
          np.uint8: rand_u8}


@pytest.mark.parametrize('dtype', [np.float32, np.float16, np.uint8])
def test_amount_zero_returns_the_bits(dtype):
    x = FRAMES[dtype]((23, 31, 3), 5)
    if dtype != np.uint8:
        x.flat[0], x.flat[1] = -0.0, np.finfo(dtype).max
    for luma, overshoot in ((False, None), (True, 0.0)):
        y = sharpen_ref(x, gaussian_weights(1.0), 0.0, 0.0, luma, overshoot)
        assert y.dtype == x.dtype and np.array_equal(y.view(np.uint8), x.view(np.uint8))


@pytest.mark.parametrize('sigma', [0.25, 1.0, 4.0])
def test_constant_frame_stays_constant(sigma):
    """The taps sum to 1 within (R + 1) ulp, so the blur of a constant v is v within (2 R + 4) u v per pass; the detail is that
    small, and amount <= 16 keeps the result within 16 * 2 (2 R + 4) u v + u v of v.  uint8 and binary16: unchanged."""
    w = gaussian_weights(sigma)
    radius = len(w) - 1
    for value in (0.7, 1.0, 123.456):
        x = np.full((20, 30, 3), value, F)
        for luma in (False, True):
            y = sharpen_ref(x, w, 16.0, 0.0, luma)
            e_s = 5 * U * value if luma else 0.0
            tol = 16 * (2 * (2 * radius + 4) * U * value + 2 * e_s + 4 * U * value) + 33 * 2 * U * value
            assert np.abs(y.astype(np.float64) - float(F(value))).max() <= tol, (sigma, value, luma)
    for value in (0, 1, 77, 255):
        x = np.full((20, 30, 3), value, np.uint8)
        assert np.array_equal(sharpen_ref(x, w, 2.0, 0.0, True, 0.0), x) and np.array_equal(sharpen_ref(x, w, 2.0, 0.0, False), x)
    x = np.full((20, 30, 1), 0.3, np.float16)
    assert np.array_equal(sharpen_ref(x, w, 2.0, 0.0, False), x)


def test_noise_below_the_threshold_leaves_the_frame_untouched():
    """|d| = |s - b| <= max s - min s <= 2 * 0.004 (the blur is a convex combination, up to rounding far below the margin):
    with threshold 0.01 every d' is 0 and y = x + amount * 0 = x."""
    w = gaussian_weights(1.5)
    x = (F(0.5) + (rand_f((40, 50, 3), 6) - F(0.5)) * F(0.008)).astype(F)
    for luma in (False, True):
        assert np.array_equal(sharpen_ref(x, w, 8.0, 0.01, luma, None), x)
    u = (128 + rand_u8((40, 50, 3), 7) % 3).astype(np.uint8)       # 128..130: |d| <= 2 codes, threshold 0.01 * 255 = 2.55
    assert np.array_equal(sharpen_ref(u, w, 8.0, 0.01, True, 0.1), u)
    assert not np.array_equal(sharpen_ref(u, w, 8.0, 0.0, True), u)    # and without the threshold it does change


def test_step_edge_overshoots_without_the_limit_and_not_with_it():
    w = gaussian_weights(2.0)
    x = np.full((24, 64, 3), 0.25, F)
    x[:, 32:] = 0.75
    free = sharpen_ref(x, w, 2.0, 0.0, True)
    assert free.max() > 0.8 and free.min() < 0.2                      # halos on both sides of the edge
    for o in (0.0, 0.03):
        held = sharpen_ref(x, w, 2.0, 0.0, True, o)
        lo, hi = extrema3x3(x)
        assert (held >= lo - F(o)).all() and (held <= hi + F(o)).all()
        assert held.max() <= F(0.75) + F(o) and held.min() >= F(0.25) - F(o)
    assert np.array_equal(sharpen_ref(x, w, 2.0, 0.0, True, 0.0)[:, :30], x[:, :30])   # away from the edge's 3x3 reach: the flat value
    u = (x * 255).astype(np.uint8)
    assert sharpen_ref(u, w, 2.0, 0.0, True).max() > 191 + 10
    held = sharpen_ref(u, w, 2.0, 0.0, True, 4.0 / 255.0).astype(int)
    assert held.max() <= 191 + 4 + 1 and held.min() >= 63 - 4 - 1    # (4/255 * 255 carries one float32 rounding, rint another half)


def test_luma_mode_keeps_a_grey_frame_grey():
    g = rand_f((33, 47, 1), 8)
    x = np.repeat(g, 3, axis=2)
    for overshoot in (None, 0.02):
        y = sharpen_ref(x, gaussian_weights(1.0), 3.0, 0.01, True, overshoot)
        assert np.array_equal(y[:, :, 0], y[:, :, 1]) and np.array_equal(y[:, :, 1], y[:, :, 2])
        assert not np.array_equal(y, x)
    u = np.repeat(rand_u8((33, 47, 1), 9), 3, axis=2)
    y = sharpen_ref(u, gaussian_weights(1.0), 3.0, 0.01, True, 0.02)
    assert np.array_equal(y[:, :, 0], y[:, :, 1]) and np.array_equal(y[:, :, 1], y[:, :, 2])
