"""CPU-only: the NumPy restatement of include/tdk_hip_ca.h (tests/chromatic_spec.py) against literal per-site loops on small frames,
and against its purpose on a synthetic chart: 384 x 512 RGGB, the sum of 40 sinusoids of random orientation (frequencies N(0, 0.12) rad
per site, amplitudes 1/sqrt(f^2 + 0.01), scaled into 0.05 .. 0.75), raw gains 0.5 / 1 / 0.7 (the regression must not need a white
balance).  Red and blue are the scene evaluated analytically at c0 + (x - c0) / s_k: the exact inverse of the model's
q = c0 + (p - c0) * s_k for a constant s_k, so that the model with v = s_k is the truth.  Nothing is read from the reference.

Measured on the restatement (corner displacement in sites, the corner is 319.3 sites from the centre):
  noise-free, fit='linear':  red +0.639 -> +0.630, +1.277 -> +1.259, +2.554 -> +2.511;  blue -0.639 -> -0.633, -0.958 -> -0.951,
      -1.916 -> -1.907: worst error 0.043 (the first-order remainder d^2 / radius is 0.020 of it); one round of refine: 0.022
  noise var = 1e-4 + 1e-4 x, three seeds, shifts 0.639 / 1.277 / 1.916: worst error with the noise model 0.0780, without it
      0.35 .. 1.12 (4.5 to 100 times the error with it); a frame without aberration: up to 0.088 with, 0.035 without
  correct with the true model at a 1.3-site corner shift, mean |difference| to the scene without aberration, after / before:
      bilinear 0.140 (red) 0.120 (blue), bicubic 0.166 / 0.149; estimate on the corrected frame: bilinear +0.017 / -0.006,
      bicubic -0.133 / +0.136.  The bicubic residual is the Keys kernel with A = -0.75 (tdk_hip_warp.h, OpenCV): it does not
      reproduce a linear ramp, its position error reaches 0.048 plane samples = 0.096 site (test_bicubic_position_error), and the
      estimator finds it.  Bilinear has none, and is the default of the front-end for that reason."""

import math

import numpy as np
import pytest

import chromatic_spec as spec

H, W = 384, 512
RGGB = spec.PATTERNS['RGGB']
X0, Y0, RN = spec.default_geometry(W, H)
CORNER = float(RN)
NOISE_FREE_BOUND = 0.05          # the issue's bound
NOISY_MEASURED = 0.0780          # the worst error with the noise model, measured on the restatement (the docstring)
SHIFTS = ((0.002, -0.002), (0.004, -0.003), (0.008, -0.006))   # s - 1 of (red, blue): corner shifts 0.639 / 1.277 / 2.554 and -0.639 / -0.958 / -1.916


@pytest.fixture(scope='module')
def scene():
    rng = np.random.default_rng(7)
    fx, fy = rng.normal(0, 0.12, 40), rng.normal(0, 0.12, 40)
    amp = 1 / np.sqrt(fx * fx + fy * fy + 0.01)
    phase = rng.uniform(0, 2 * np.pi, 40)

    def raw(x, y):
        out = np.zeros(np.broadcast(x, y).shape)
        for k in range(40):
            out += amp[k] * np.sin(fx[k] * x + fy[k] * y + phase[k])
        return out

    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    base = raw(xx, yy)
    lo, hi = base.min(), base.max()
    return lambda x, y: 0.05 + 0.7 * (raw(x, y) - lo) / (hi - lo)


def chart(scene, s_red, s_blue, gains=(0.5, 1.0, 0.7)):
    """float64 mosaic: colour k is gains[k] * scene(c0 + (x - c0) / s_k)."""
    x0, y0 = (W - 1) / 2, (H - 1) / 2
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    m = np.zeros((H, W))
    for colour, s, (oy, ox) in ((0, s_red, (0, 0)), (1, 1.0, (0, 1)), (1, 1.0, (1, 0)), (2, s_blue, (1, 1))):
        x, y = xx[oy::2, ox::2], yy[oy::2, ox::2]
        m[oy::2, ox::2] = gains[colour] * scene(x0 + (x - x0) / s, y0 + (y - y0) / s)
    return m


def corner(model):
    return [spec.corner_shift(model[k], X0, Y0, RN, W, H) for k in range(2)]


def refine(mosaic, model, interp=spec.BILINEAR, **kw):
    """ChromaticAberration.refine on the restatement: model + estimate(correct(mosaic, model)) - identity."""
    residual, _ = spec.estimate([spec.correct(mosaic, RGGB, model, X0, Y0, RN, interp)], RGGB, X0, Y0, RN, **kw)
    out = model.copy()
    out[:, :3] += (residual[:, :3] - np.array([1, 0, 0], dtype=np.float32)) * residual[:, 3:4]
    return out


# ---------------------------------------------------------------- literal loops
def literal_correct(mosaic, pattern, model, x0, y0, rn, interp, out_dtype):
    f = np.float32
    x = mosaic.astype(f)
    h, w = x.shape
    out = x.copy()
    c1 = lambda t: ((f(1.25) * t - f(2.25)) * t) * t + f(1.0)
    c2 = lambda t: ((f(-0.75) * t + f(3.75)) * t - f(6.0)) * t + f(3.0)
    with np.errstate(all='ignore'):
        for i in range(h):
            for j in range(w):
                k = (pattern >> (2 * (2 * (i & 1) + (j & 1)))) & 3
                if k == 1 or model[k // 2, 3] == 0:
                    continue
                v, c, b = (f(t) for t in model[k // 2, :3])
                px, py = f(j) - f(x0), f(i) - f(y0)
                rho = np.sqrt(px * px + py * py) / f(rn)
                t = ((b * rho + c) * rho + v) - f(1.0)
                dx, dy = px * t, py * t
                if not (np.isfinite(dx) and np.isfinite(dy)):
                    dx = dy = f(0)
                dx, dy = min(max(dx, f(-8)), f(8)), min(max(dy, f(-8)), f(8))
                if dx == 0 and dy == 0:
                    continue
                u, vv = f(j >> 1) + dx * f(0.5), f(i >> 1) + dy * f(0.5)
                xf, yf = np.floor(u), np.floor(vv)
                ax, ay = u - xf, vv - yf
                if interp == spec.BICUBIC:
                    wx, wy, lo = [c2(ax + f(1)), c1(ax), c1(f(1) - ax), c2(f(2) - ax)], [c2(ay + f(1)), c1(ay), c1(f(1) - ay), c2(f(2) - ay)], -1
                else:
                    wx, wy, lo = [f(1) - ax, ax], [f(1) - ay, ay], 0
                tap = lambda m, n: x[2 * min(max(int(yf) + lo + m, 0), h // 2 - 1) + (i & 1), 2 * min(max(int(xf) + lo + n, 0), w // 2 - 1) + (j & 1)]
                acc = None
                for m in range(len(wy)):
                    r = tap(m, 0) * wx[0] + tap(m, 1) * wx[1]
                    for n in range(2, len(wx)):
                        r = r + tap(m, n) * wx[n]
                    acc = r * wy[0] if m == 0 else acc + r * wy[m]
                out[i, j] = acc
    return out.astype(out_dtype)


@pytest.mark.parametrize('name', sorted(spec.PATTERNS))
@pytest.mark.parametrize('interp', (spec.BILINEAR, spec.BICUBIC))
def test_correct_is_the_literal_loop(name, interp):
    rng = np.random.default_rng(11)
    for (h, w), dtype, out_dtype in (((2, 2), np.float32, np.float32), ((6, 4), np.float16, np.float32), ((14, 18), np.float32, np.float16)):
        mosaic = rng.uniform(0, 1, (h, w)).astype(dtype)
        if h > 2:
            mosaic[3, 2] = np.nan
        x0, y0, rn = spec.default_geometry(w, h)
        for model in (np.array([[1.3, 0.2, -0.1, 1], [0.6, 0.0, 0.3, 1]], np.float32), np.array([[1.01, 0, 0, 0], [3.0, 0, 0, 1]], np.float32),   # the clamp at D acts
                      spec.identity_model()):
            want = literal_correct(mosaic, spec.PATTERNS[name], model, x0, y0, rn, interp, out_dtype)
            got = spec.correct(mosaic, spec.PATTERNS[name], model, x0, y0, rn, interp, out_dtype)
            assert got.dtype == out_dtype and np.array_equal(got.view(np.uint16 if out_dtype == np.float16 else np.uint32),
                                                              want.view(np.uint16 if out_dtype == np.float16 else np.uint32))


def literal_sums(mosaics, pattern, clip, block):
    h, w = mosaics[0].shape
    sums = np.zeros((h // block, w // block, 2, spec.SUMS), dtype=np.int64)
    q = lambda v: int(min(max(np.rint(np.float32(v) * np.float32(65535.0)), 0), 65535))
    ok = lambda v: bool(np.isfinite(v)) and np.float32(v) < np.float32(clip)
    for mosaic in mosaics:
        x = mosaic.astype(np.float32)
        for i in range(1, h - 1):
            for j in range(1, w - 1):
                k = (pattern >> (2 * (2 * (i & 1) + (j & 1)))) & 3
                if k == 1 or i // block >= h // block or j // block >= w // block:
                    continue
                five = (x[i, j], x[i, j - 1], x[i, j + 1], x[i - 1, j], x[i + 1, j])
                if not all(ok(v) for v in five):
                    continue
                c, gl, gr, gu, gd = (q(v) for v in five)
                t = (gl + gr + gu + gd, gr - gl, gd - gu, c)
                rec = sums[i // block, j // block, k // 2]
                rec[:7] += (1, j, i, *t)
                rec[7:] += [t[a] * t[b] for a in range(4) for b in range(a, 4)]
    return sums


@pytest.mark.parametrize('name', sorted(spec.PATTERNS))
def test_block_sums_are_the_literal_loop(name):
    rng = np.random.default_rng(5)
    frames = [rng.uniform(-0.05, 1.1, (40, 54)).astype(dtype) for dtype in (np.float32, np.float32)]
    frames[0][7, 9] = np.nan
    frames[1][20, 30] = np.inf
    got = spec.block_sums(frames, spec.PATTERNS[name], 0.95, 16)
    assert got.shape == (2, 3, 2, 17) and np.array_equal(got, literal_sums(frames, spec.PATTERNS[name], 0.95, 16))
    assert got[..., 0].min() > 0


def test_bicubic_position_error():
    """The Keys kernel with A = -0.75 does not reproduce a ramp: interpolating f(k) = k at offset a gives a + e(a), |e| up to 0.048
    samples; bilinear is exact.  It is why `estimate` finds a residual behind a bicubic `correct`."""
    a = np.linspace(0, 1, 1001, dtype=np.float32)
    w = spec.weights(a, spec.BICUBIC)
    e = (-w[0] + w[2] + 2 * w[3]) - a
    assert 0.047 < np.abs(e).max() < 0.049
    assert np.abs(w[0] + w[1] + w[2] + w[3] - 1).max() < 4e-6   # float32: the Horner steps of c2 pass through 6, half an ulp there is 2.4e-7
    w = spec.weights(a, spec.BILINEAR)
    assert np.abs(w[1] - a).max() == 0


# ---------------------------------------------------------------- purpose
@pytest.fixture(scope='module')
def noise_free(scene):
    """[(mosaic, linear model)] of the three pairs."""
    out = []
    for red, blue in SHIFTS:
        mosaic = chart(scene, 1 + red, 1 + blue).astype(np.float32)
        out.append((mosaic, spec.estimate([mosaic], RGGB, X0, Y0, RN)[0]))
    return out


def test_noise_free_recovery(noise_free):
    for (red, blue), (_, model) in zip(SHIFTS, noise_free):
        got, want = corner(model), (red * CORNER, blue * CORNER)
        print(f'true {want[0]:+.3f} {want[1]:+.3f}  estimated {got[0]:+.3f} {got[1]:+.3f}')
        assert model[0, 3] == 1 and model[1, 3] == 1 and model[:, 1:3].max() == 0
        assert abs(got[0] - want[0]) <= NOISE_FREE_BOUND and abs(got[1] - want[1]) <= NOISE_FREE_BOUND


def test_poly3_recovers_a_radial_polynomial(scene, noise_free):
    mosaic = noise_free[1][0]
    model, _ = spec.estimate([mosaic], RGGB, X0, Y0, RN, fit=spec.POLY3)
    got = corner(model)
    print(model, got)
    assert model[:, 3].min() == 1
    assert abs(got[0] - 0.004 * CORNER) <= NOISE_FREE_BOUND and abs(got[1] + 0.003 * CORNER) <= NOISE_FREE_BOUND


def test_refine_does_not_increase_the_noise_free_error(noise_free):
    """The noise-free error is the worst over the three pairs and both colours: 0.043 before, 0.022 after one round (bilinear).  Per
    case the round removes the first-order remainder and leaves what the interpolator adds, +1 to +2 % of the shift (a two-tap
    interpolation is exact in its centroid, not in its group delay): 0.043 -> 0.022, 0.018 -> 0.017, 0.009 -> 0.001, 0.007 -> 0.007,
    and the two smallest rise, 0.008 -> 0.012 and 0.006 -> 0.007.  Behind a bicubic `correct` a round makes things worse
    (0.630 -> 0.475 for a true 0.639: test_bicubic_position_error); refine is for the bilinear default."""
    before = after = 0.0
    for (red, blue), (mosaic, model) in zip(SHIFTS, noise_free):
        want = (red * CORNER, blue * CORNER)
        first, second = corner(model), corner(refine(mosaic, model))
        print(f'true {want[0]:+.3f} {want[1]:+.3f}  first {first[0]:+.4f} {first[1]:+.4f}  refined {second[0]:+.4f} {second[1]:+.4f}')
        for k in range(2):
            before, after = max(before, abs(first[k] - want[k])), max(after, abs(second[k] - want[k]))
            assert abs(second[k] - want[k]) <= NOISE_FREE_BOUND
    print('worst error', before, '->', after)
    assert after <= before


def test_noisy_recovery_needs_the_noise_model(scene):
    """var = 1e-4 + 1e-4 x: the gradient SNR is about 1.  With the model the worst error stays within 1.25 times what was measured
    (the margin is for the seeds); wherever the true shift is 0.6 site or more it is below half the error without the model."""
    noise_model = np.array([[1e-4, 1e-4, 1, 0]] * 3, dtype=np.float32)
    worst = 0.0
    for seed in (1, 2, 3):
        for shift in (0.002, 0.004, 0.006):
            clean = chart(scene, 1 + shift, 1 - shift)
            rng = np.random.default_rng(seed)
            mosaic = (clean + rng.normal(size=clean.shape) * np.sqrt(1e-4 + 1e-4 * clean)).astype(np.float32)
            sums = spec.block_sums([mosaic], RGGB)
            with_model = corner(spec.fit_model(sums, X0, Y0, RN, noise_model))
            without = corner(spec.fit_model(sums, X0, Y0, RN))
            for k, want in enumerate((shift * CORNER, -shift * CORNER)):
                e_with, e_without = abs(with_model[k] - want), abs(without[k] - want)
                print(f'seed {seed} true {want:+.3f}  with {with_model[k]:+.3f}  without {without[k]:+.3f}')
                worst = max(worst, e_with)
                assert abs(want) >= 0.6 and e_with < 0.5 * e_without
    print('worst error with the noise model', worst)
    assert worst <= 1.25 * NOISY_MEASURED


@pytest.mark.parametrize('interp', (spec.BILINEAR, spec.BICUBIC))
def test_correct_with_the_true_model_aligns_the_planes(scene, interp):
    red, blue = 1 + 1.3 / CORNER, 1 - 1.3 / CORNER
    mosaic = chart(scene, red, blue).astype(np.float32)
    clean = chart(scene, 1.0, 1.0)
    model = np.array([[red, 0, 0, 1], [blue, 0, 0, 1]], dtype=np.float32)
    fixed = spec.correct(mosaic, RGGB, model, X0, Y0, RN, interp)
    assert np.array_equal(fixed[0::2, 1::2], mosaic[0::2, 1::2]) and np.array_equal(fixed[1::2, 0::2], mosaic[1::2, 0::2])
    for oy, ox in ((0, 0), (1, 1)):
        before = np.abs(mosaic[oy::2, ox::2] - clean[oy::2, ox::2]).mean()
        after = np.abs(fixed[oy::2, ox::2] - clean[oy::2, ox::2]).mean()
        print('interp', interp, 'plane', (oy, ox), 'after / before', after / before)
        assert after <= 0.5 * before
    residual = corner(spec.estimate([fixed], RGGB, X0, Y0, RN)[0])
    print('interp', interp, 'estimate on the corrected frame', residual)
    if interp == spec.BILINEAR:   # (bicubic: the position error of its kernel, -0.133 / +0.136: the docstring and test_bicubic_position_error)
        assert max(abs(r) for r in residual) <= NOISE_FREE_BOUND


def test_degenerate_frames_give_no_model():
    flat = np.full((H, W), 0.3, dtype=np.float32)
    small = np.random.default_rng(3).uniform(0, 0.9, (62, 126)).astype(np.float32)
    clipped = np.random.default_rng(4).uniform(0.96, 1.0, (H, W)).astype(np.float32)
    for mosaic in (flat, small, clipped):
        for fit in (spec.LINEAR, spec.POLY3):
            x0, y0, rn = spec.default_geometry(mosaic.shape[1], mosaic.shape[0])
            model, sums = spec.estimate([mosaic], RGGB, x0, y0, rn, fit=fit)
            assert np.array_equal(model, np.array([[1, 0, 0, 0], [1, 0, 0, 0]], dtype=np.float32))
    assert spec.block_sums([small], RGGB).size == 0 and spec.block_sums([clipped], RGGB).max() == 0
    # and the identity model changes nothing, NaNs included
    small[5, 7] = np.nan
    out = spec.correct(small, RGGB, spec.identity_model(), *spec.default_geometry(126, 62))
    assert np.array_equal(out.view(np.uint32), small.view(np.uint32))
    assert math.isclose(spec.lds_bytes(spec.BICUBIC), 19712) and spec.lds_bytes(spec.BILINEAR) == 17472
