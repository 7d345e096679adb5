"""CPU-only: the fp32 C oracle against the NaN-faithful float64 specification (tests/color_domain_spec.py) on exactly the pixel
sets tests/test_gpu_color_domain.py runs the kernels on: in-gamut, [-0.25, 1.6], a dense set in [-0.02, 0.02], greys, pixels a
few ulps on either side of every branch constant, Lab with L outside [0, 1]; float32 storage and float16 storage (the
specification sees the rounded input).

Per case: the oracle's NaN positions are the specification's; every non-excluded value is within `(A_op + K_op * s_i) * scale`;
at most 1 % of the values are excluded (their GPU bound, 8x the oracle's, exceeds 1e-3).  For the tone mappers the oracle's
uint8 is floor(clip(spec) * 255 + 0.5), one step off only where spec * 255 lies within 255x the value's bound of a rounding tie.
The constants of color_domain_spec.CONSTANTS are minimal: halving either makes the oracle fail."""

import numpy as np
import pytest

import color_domain_spec as S

CASES = S.COLOR_CASES + S.TONEMAP_CASES


def compare(oracle, case, dtype, special=False, ak=None):
    x, r, s, sc, pre = S.case_spec(case, dtype, special)
    of, ou8 = S.oracle_run(oracle, case, x)
    d = S._absdiff(of.astype(np.float64), r)
    return x, r, of, ou8, d, S.bound(case[0], s, sc, pre, 1.0, ak), S.excluded(case[0], s, sc, pre, ak), sc


@pytest.mark.parametrize('dtype', ['f32', 'f16'])
@pytest.mark.parametrize('case', CASES, ids=S.case_id)
def test_oracle_meets_the_specification(oracle, case, dtype):
    x, r, of, ou8, d, b, ex, sc = compare(oracle, case, dtype)
    assert np.array_equal(np.isnan(of), np.isnan(r)), 'NaN positions differ'
    assert ex.mean() <= S.EXCLUDE_CAP, f'{ex.mean():.4f} of the values are ill-conditioned: the pixel sets must keep this below 1 %'
    bad = ~ex & (d > b)
    assert not bad.any(), (f'{bad.sum()} values beyond the bound; first pixel {x[np.argwhere(bad)[0][0]]}: oracle '
                           f'{of[np.argwhere(bad)[0][0]]}, specification {r[np.argwhere(bad)[0][0]]}')
    if ou8 is not None:
        dq = np.abs(ou8.astype(np.float64) - S.quantise(r))
        assert (dq[~ex] <= 1).all()
        off = ~ex & (dq > 0)
        assert (S.tie_distance(r)[off] <= 255.0 * b[off]).all(), 'a uint8 step away from the specification, and not on a rounding tie'
        assert (dq > 0).sum() <= S.CONSTANTS[case[0]][3], (dq > 0).sum()


@pytest.mark.parametrize('key', sorted(S.CONSTANTS))
def test_constants_are_minimal(oracle, key):
    """CONSTANTS is filled from a run of color_domain_spec.measure_constants: with half the A or half the K the oracle misses."""
    a, k = S.CONSTANTS[key][:2]
    cases = [c for c in CASES if c[0] == key]
    assert cases

    def worst(ak):
        w = 0.0
        for case in cases:
            for dtype in ('f32', 'f16'):
                x, r, of, ou8, d, b, ex, sc = compare(oracle, case, dtype, ak=ak)
                with np.errstate(all='ignore'):
                    w = max(w, float(np.where(ex | (d == 0.0), 0.0, d / b).max()))
        return w

    w = worst((a, k))
    assert w <= 1.0, w
    if a > 2.0 ** -30:
        assert worst((a / 2.0, k)) > 1.0
    if k > 1:
        assert worst((a, k / 2.0)) > 1.0


@pytest.mark.parametrize('case', CASES, ids=S.case_id)
def test_special_pixels(oracle, case):
    """0, -0, 1, the metrics' means, -1, +-inf and NaN in every channel position: the oracle's NaN positions are the specification's
    and its finite values are inside the bound the kernels get on these pixels (8x: the constants were not measured here).  Pixels whose intermediates exceed 2^30 are left to the GPU test, which holds the
    kernels to the oracle itself: float64 does not overflow where float32 does (65504^2.4 is finite in both, its cube is not)."""
    x, r, of, ou8, d, b, ex, sc = compare(oracle, case, 'f32', special=True)
    ok = (sc <= 2.0 ** 30)[:, 0] & ~(np.abs(np.where(np.isfinite(x), x, 0.0)) >= 65504.0).any(1)
    assert ok.sum() >= 28
    assert np.array_equal(np.isnan(of)[ok], np.isnan(r)[ok])
    with np.errstate(all='ignore'):
        bad = ok[:, None] & ~(d <= S.GPU_FACTOR * b)
    assert not bad.any(), (x[np.argwhere(bad)[0][0]], of[np.argwhere(bad)[0][0]], r[np.argwhere(bad)[0][0]])
    if ou8 is not None:
        sure = ok[:, None] & (S.tie_distance(r) > 255.0 * S.GPU_FACTOR * b)
        assert np.array_equal(ou8[sure].astype(np.float64), S.quantise(r)[sure])


@pytest.mark.parametrize('case', CASES, ids=S.case_id)
def test_special_pixel_classes(oracle, case):
    """What tests/test_gpu_color_domain.py compares each special value with is fixed by the oracle and the specification alone:
    the class sizes are the recorded ones and every value is in exactly one class."""
    x, r, b, o, exact, tied, loose = S.special_classes(oracle, case)
    assert (exact.astype(int) + tied + loose == 1).all()
    assert (int(exact.sum()), int(tied.sum()), int(loose.sum())) == S.SPECIAL_COUNTS[S.case_id(case)]


def test_pixel_sets_cover_the_domain():
    """Every set the module docstring lists is there, and no value is a float32 denormal (outside the tested domain)."""
    px = S.pixels('rgb')
    assert px.shape == (S.N_PIXELS, 3) and S.N_PIXELS % 4 == 3
    tiny = np.finfo(np.float32).tiny
    for kind in ('rgb', 'xyz', 'lab'):
        p = S.pixels(kind)
        assert np.isfinite(p).all() and not ((p != 0) & (np.abs(p) < tiny)).any()
    assert (px < 0).any() and (px > 1).any() and (px == 0).any() and px.min() >= -0.25 and px.max() <= 1.6
    assert ((np.abs(px) <= 0.02).all(1)).sum() >= 1000                        # the dense set around 0
    assert ((px[:, 0] == px[:, 1]) & (px[:, 1] == px[:, 2])).sum() >= 2000   # greys
    for k in (0.04045, 0.0031308, 0.5, 1.0):                                 # both sides of the branch constants on the input itself
        k32 = np.float32(k)
        assert (px == k32).any() and (px == np.nextafter(k32, np.float32(2))).any() and (px == np.nextafter(k32, np.float32(-1))).any()
    d = px.max(1) - px.min(1)
    assert ((d > 0) & (d <= np.float32(1e-6))).any() and ((d > np.float32(1e-6)) & (d < 1.5e-6)).any()  # HSL's delta threshold
    lab = S.pixels('lab')
    assert (lab[:, 0] < 0).any() and (lab[:, 0] > 1).any()
    # both sides of lab_f's and lab_f_inv's thresholds are reached through the arithmetic
    with np.errstate(all='ignore'):
        y = S.A.rgb_to_xyz(px.astype(np.float64))[:, 1]
        for t in (S.A.T_LAB, S.B.DELTA3):
            assert ((y > t) & (y < t * 1.001)).any() and ((y <= t) & (y > t * 0.999)).any()
        fy = lab[:, 0].astype(np.float64) * S.c32(100.0 / 116.0) + S.A.OFF
        assert ((fy ** 3 > S.A.T_LAB) & (fy ** 3 < S.A.T_LAB * 1.001)).any() and ((fy ** 3 <= S.A.T_LAB) & (fy ** 3 > S.A.T_LAB * 0.999)).any()
        hsl = S.A.rgb_to_hsl(px.astype(np.float64))
    for k in range(1, 6):   # hue sector borders
        assert (np.abs(hsl[:, 0] - k / 6.0) < 1e-6).any()
    assert ((hsl[:, 2] < 0.5) & (hsl[:, 2] > 0.4999999)).any() and (hsl[:, 2] == 0.5).any()


def test_semantics_nan_pow_clip():
    """The three rules the in-gamut restatement does not have."""
    with np.errstate(all='ignore'):
        assert np.isnan(S.cpow(np.array([-0.5]), 1 / 2.4)[0]) and S.cpow(np.array([np.nan]), 0.0)[0] == 1.0
        assert S.clip01(np.array([np.nan, -1.0, 2.0, np.inf, -np.inf])).tolist() == [0.0, 0.0, 1.0, 1.0, 0.0]
    m = S.METRICS
    # Reinhard at light_adapt 1: the adaptation of a negative channel is NaN, c / (NaN + c) is NaN, fmax drops it, 0^(1 / gamma) = 0
    r, _, _ = S.evaluate('tonemap_reinhard', np.array([[-0.1, 0.5, np.nan]]), (m, 0.75, 2.0, 1.0, 0.0))
    assert r[0, 0] < 1e-6 and 0.01 < r[0, 1] < 0.99 and r[0, 2] < 1e-6   # (the Lab round trip of 0 leaves ~2e-7)
    # gamma = inf: pow(x, 0) == 1 also for the dropped NaN
    r, _, _ = S.evaluate('tonemap_reinhard', np.array([[-0.1, 0.5, np.nan]]), (m, np.inf, 2.0, 1.0, 0.0))
    assert np.allclose(r, 1.0, atol=1e-6)
    # modify_hsl: a negative lightness gives pow(l, y) = NaN, the clip turns the pixel to 0
    r, _, _ = S.evaluate('modify_hsl', np.array([[-0.2, -0.1, -0.3]]), (0.1, 0.3, -0.2))
    assert (r == 0.0).all()
