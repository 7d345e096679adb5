"""CPU-only: every claim tests/test_gpu_denoise_domain.py relies on, checked against the references alone (oracle.wiener,
oracle.bilateral, nlm_ref, wavelet_ref and the float64 restatements) -- the footprints of tests/denoise_cases.py equal the
references' changed sets, which classes keep a reference finite and which make it NaN, the references' own distance from float64 on
the finite classes, and that a reference's result is bit-identical to the clean frame's outside a sample's footprint."""

from pathlib import Path

import numpy as np
import pytest

import color_domain_spec as S
import denoise_cases as dc
from test_gpu_nlmeans import nlm_ref
from test_oracle_second_source import wiener_fp64
from test_wavelet_spec import wavelet_ref

PAIRS = list(dc.WIENER_FRAMES)
NONFINITE = [dc.NAN, dc.INF, -dc.INF]


def changed(a, b):
    return ~((a == b) | (np.isnan(a) & np.isnan(b)))


def plane(scene, h, w, seed=7):
    return np.ascontiguousarray(scene(h, w, seed)[:, :, 1])


def wiener(oracle, x, sigma, K, ov):
    return oracle.wiener(np.ascontiguousarray(x[:, :, None]), sigma, K, ov)[:, :, 0]


# ------------------------------------------------------------------ the tables themselves
def test_special14_is_the_list_of_the_parity_tests():
    line = 'special = np.array([0.0, -0.0, 1e-45, 1e-39, 2.0 ** -41, 2.0 ** -40, 2.0 ** 40, 2.0 ** 41, 1e30, -0.3, -1e30, np.inf, -np.inf, np.nan], np.float32)'
    assert line in (Path(__file__).parent / 'test_gpu_parity.py').read_text()
    assert len(dc.SPECIAL14) == 14 and eval(line.split(' = ')[1], {'np': np}).tobytes() == dc.SPECIAL14.tobytes()
    assert [dc.is_tame(v) for v in dc.SPECIAL14] == [True] * 8 + [False, True] + [False] * 4
    assert all(0 < abs(float(v)) < 1.1754944e-38 for v in dc.SUBNORMALS)


def test_wiener_frames_come_from_the_geometry_tables_and_have_3x3_workgroups():
    import wiener_cases as wc

    w, h = dc.WIENER_FRAMES[(32, 4)]
    assert (w, h) in wc.STRIP_SHAPES
    g = wc.strip_geometry(w, h)
    assert (g.strips, g.segments) == (4, 3) and g.last_strip_tiles == 1 and g.last_segment_rows == 1
    assert not [s for s in wc.STRIP_SHAPES if s[0] * s[1] < w * h and wc.strip_geometry(*s).strips >= 3 and wc.strip_geometry(*s).segments >= 3]
    for K, ov in ((16, 4), (32, 2)):
        w, h = dc.WIENER_FRAMES[(K, ov)]
        assert (w, h) in wc.GROUP_SHAPES[(K, ov)]
        g = wc.group_geometry(w, h, K, ov)
        assert (g.groups_x, g.groups_y, g.last_group_tiles, g.last_group_rows) == (3, 3, 1, 1) and (g.G, g.TR) == dc.WIENER_GROUP[(K, ov)]
        assert not [s for s in wc.GROUP_SHAPES[(K, ov)] if s[0] * s[1] < w * h and wc.group_geometry(*s, K, ov).groups_x >= 3 and wc.group_geometry(*s, K, ov).groups_y >= 3]
    assert all(w * h <= 100_000 for w, h in dc.WIENER_FRAMES.values())
    assert dc.wiener_seam(32, 4) == (40, 104)   # tile 16 / tile row 8 start at (16 - 3) * 8 and (8 - 3) * 8


def test_wiener_footprint_on_hand_computed_samples():
    """The interior case of the issue (96 x 128, sample at (50, 70), K = 32, ov = 4): origins 24 .. 48 / 40 .. 64, so rows
    24 .. 79 and columns 40 .. 95.  Column 70 is read by tile columns 8 .. 11 counted from the first tile (origin -24): 8 and 11
    have their partners 9 and 10 inside the set, so the kernels' footprint is the same box; column 74 is read by tiles 9 .. 12,
    whose partners 8 and 13 add the columns 40 .. 47 and 104 .. 111."""
    m = dc.wiener_footprint2d(50, 70, 96, 128, 32, 4)
    assert m.sum() == 3136 and m[24:80, 40:96].all()
    assert np.array_equal(m, dc.wiener_footprint2d(50, 70, 96, 128, 32, 4, pairs=True))
    assert np.flatnonzero(dc.wiener_footprint(74, 128, 32, 4)).tolist() == list(range(48, 104))
    assert np.flatnonzero(dc.wiener_footprint(74, 128, 32, 4, pairs=True)).tolist() == list(range(40, 112))
    # near a border the mirrored readers (reflect(-10) = 10: the tiles at -24 and -16 read sample 10 twice) hang over that border
    # and write columns the direct readers write anyway: the reference's footprint is that of the direct readers, cut to the frame
    assert np.flatnonzero(dc.wiener_footprint(10, 128, 32, 4)).tolist() == list(range(0, 40))      # origins -16 .. 8
    assert np.flatnonzero(dc.wiener_footprint(110, 128, 32, 4)).tolist() == list(range(80, 128))   # origins 80 .. 104, and 120 mirrored (reflect(145))
    assert np.flatnonzero(dc.wiener_footprint(90, 128, 32, 4)).tolist() == list(range(64, 120))    # origins 64 .. 88; 120 reads no further back than 104
    # the kernels' footprint follows from WHICH tiles read: sample 30 is read by origins 0 .. 24 = tiles 3 .. 6 counted from the
    # first (origin -24), whose partners are tiles 2 and 7: columns 0 .. 63 instead of 0 .. 55
    assert np.flatnonzero(dc.wiener_footprint(30, 128, 32, 4)).tolist() == list(range(0, 56))
    assert np.flatnonzero(dc.wiener_footprint(30, 128, 32, 4, pairs=True)).tolist() == list(range(0, 64))


def test_sum_overflow_set_on_hand_computed_samples():
    """361 x 105, K = 32, ov = 4, a sample of 3e38 at (2, 120): the tile rows at -24, -16 and -8 read row 2 twice (reflect(-2) = 2),
    the one at 0 once; 2 * 3e38 > FLT_MAX, so rows 0 .. 23 of the kernels' footprint (columns 88 .. 159: readers 96 .. 120 =
    tiles 15 .. 18, partners 14 and 19).  Row and column 0 are read once by every tile (reflect(0) = 0 has no mirror image); 1e30
    never overflows a sum."""
    m = dc.wiener_sum_overflow2d(2, 120, 3e38, 105, 361, 32, 4)
    assert m.sum() == 24 * 72 and m[:24, 88:160].all()
    assert not dc.wiener_sum_overflow2d(53, 183, 3e38, 105, 361, 32, 4).any() and not dc.wiener_sum_overflow2d(0, 0, 3e38, 105, 361, 32, 4).any()
    assert not dc.wiener_sum_overflow2d(2, 120, 1e30, 105, 361, 32, 4).any()
    m = dc.wiener_sum_overflow2d(104, 360, 3e38, 105, 361, 32, 4)   # the bottom right sample: every tile that reads it reads it twice or four times
    assert np.array_equal(m, dc.wiener_footprint2d(104, 360, 105, 361, 32, 4, pairs=True))


def test_interior_frame_has_an_interior_workgroup_around_its_samples(td):
    """include/tdk_hip_wiener.h: workgroup (strip, segment) covers columns 8 (16 strip - 3) .. + 151 and rows 8 (8 segment - 3) .. + 87."""
    from torch_darktable import _native

    w, h = dc.WIENER_INTERIOR_FRAME
    q = _native.lib.tdk_wiener_strip_interior
    assert w % 4 == 0 and w * h <= 100_000 and q(w, h, 8, 1, 1) == 1 and q(w, h, 8, 2, 2) == 1
    assert all(q(*dc.WIENER_FRAMES[(32, 4)], 8, st, sg) == 0 for st in range(4) for sg in range(3))
    y, x = dc.WIENER_INTERIOR_POSITIONS['interior-body']
    assert 104 + 32 <= x < 256 - 32 and 40 + 32 <= y < 128 - 32   # every tile that reads it belongs to workgroup (1, 1)
    assert dc.WIENER_INTERIOR_POSITIONS['interior-body-seam'] == (8 * (8 * 2 - 3), 8 * (16 * 2 - 3))


@pytest.mark.parametrize('K,ov', PAIRS)
def test_pair_footprint_widens_columns_only_by_at_most_one_tile_step(K, ov):
    w, h = dc.WIENER_FRAMES[(K, ov)]
    s = K // ov
    wider = 0
    for y, x in dc.wiener_positions(K, ov).values():
        a, b = dc.wiener_footprint2d(y, x, h, w, K, ov), dc.wiener_footprint2d(y, x, h, w, K, ov, pairs=True)
        assert (b | a).sum() == b.sum() and np.array_equal(a.any(1), b.any(1))
        ca, cb = np.flatnonzero(a.any(0)), np.flatnonzero(b.any(0))
        assert ca.min() - cb.min() in (0, s) and cb.max() - ca.max() in (0, s)
        wider += b.sum() > a.sum()
    assert wider >= 2   # the sweep has samples whose partner tiles lie outside the reference's footprint


# ------------------------------------------------------------------ Wiener: footprints, finiteness, outside-footprint identity
@pytest.fixture(scope='module')
def wiener_clean(scene, oracle):
    out = {}
    for (K, ov), (w, h) in dc.WIENER_FRAMES.items():
        base = plane(scene, h, w)
        out[K, ov] = (base, wiener(oracle, base, 0.05, K, ov))
    return out


@pytest.mark.parametrize('K,ov', PAIRS)
def test_wiener_footprints_are_the_oracles_changed_sets(oracle, wiener_clean, K, ov):
    """Every single_* case: the result is bit-identical to the clean frame's outside the footprint; NaN, +-inf, 1e30 and 3e38
    change -- and make NaN -- exactly the footprint (reflected reads near the borders included); +-1e18 stay finite everywhere."""
    base, clean = wiener_clean[K, ov]
    h, w = base.shape
    for case in dc.classes(base, dc.wiener_positions(K, ov), only=dc.SINGLE):
        (y, x, v), = case.samples
        got = wiener(oracle, case.frame, 0.05, K, ov)
        fp = dc.wiener_footprint2d(y, x, h, w, K, ov)
        ch = changed(got, clean)
        assert not (ch & ~fp).any(), case.name
        if case.kind == 'finite':
            assert np.isfinite(got).all() and ch.sum() > 0.9 * fp.sum(), case.name
        else:
            assert np.array_equal(ch, fp) and np.array_equal(np.isnan(got), fp) and not np.isinf(got).any(), case.name


def test_wiener_small_sample_leaves_every_pixel_finite(oracle, wiener_clean):
    base, _ = wiener_clean[32, 4]
    f = base.copy()
    f[50, 70] = 1e-40
    assert np.isfinite(wiener(oracle, f, 0.05, 32, 4)).all()


@pytest.mark.parametrize('K,ov', PAIRS)
def test_wiener_oracle_vs_fp64_on_the_finite_classes(oracle, wiener_clean, K, ov):
    """The reference's own error: within 2e-6 of the float64 restatement relative to the per-pixel scale of
    denoise_cases.wiener_scale (the reference shares no transform between tiles: pairs=False), a tenth of what the kernels are
    held to.  A constant frame comes back within 5e-7 |c|; scene * s with sigma * s is s times the s = 1 result within 5e-7 s."""
    base, clean = wiener_clean[K, ov]
    worst = 0.0
    for case in dc.classes(base, dc.wiener_positions(K, ov)):
        if case.kind != 'finite':
            continue
        sigma = 0.05 * case.sigma_scale
        got = wiener(oracle, case.frame, sigma, K, ov)
        assert np.isfinite(got).all(), case.name
        ratio = float((np.abs(got - wiener_fp64(case.frame, sigma, K, ov)) / dc.wiener_scale(case, K, ov, pairs=False)).max())
        worst = max(worst, ratio)
        assert ratio <= 2e-6, (case.name, ratio)
        if case.name.startswith('flat'):
            c = float(case.frame[0, 0])
            assert np.abs(got - c).max() <= 5e-7 * abs(c), case.name
        if case.name.startswith('scaled'):
            assert np.abs(got - np.float32(case.sigma_scale) * clean).max() <= 5e-7 * case.sigma_scale, case.name
    print(f'K={K} ov={ov}: oracle within {worst:.2e} of float64, relative to the per-pixel scale')


@pytest.mark.parametrize('K,ov', PAIRS)
def test_wiener_fp64_restatement_digests_the_overflowing_samples(oracle, wiener_clean, K, ov):
    """What the kernels are held to inside the footprint of a single_overflowing sample: the float64 restatement, where
    |X|^2 ~ 1e60 is an ordinary number and the gain is 1 - sigma^2 / |X|^2 = 1 to the last bit -- the tiles pass their samples
    through, so the result is the input wherever the tiles that cover a pixel all hold the sample."""
    base, clean = wiener_clean[K, ov]
    y, x = dc.wiener_positions(K, ov)['interior']
    for v in dc.OVERFLOWING:
        f = base.copy()
        f[y, x] = v
        r = wiener_fp64(f, 0.05, K, ov)
        assert np.isfinite(r).all() and abs(r[y, x] - v) <= 1e-6 * v
        fp = dc.wiener_footprint2d(y, x, *f.shape, K, ov)
        assert np.abs(r - clean)[~fp].max() <= 2e-6


# ------------------------------------------------------------------ bilateral
@pytest.mark.parametrize('path', list(dc.BILATERAL_PATHS))
def test_bilateral_oracle_box_and_finiteness(scene, oracle, path):
    """A single sample changes at most the box of BILATERAL_RADIUS = 4 sigma_s - 1 (the sample's cell pair, blurred by two cells
    either way, is read by the pixels whose own cell pair meets those six cells), and reaches within one pixel of that radius for
    some sample; the result is finite except for +inf at the pixel of a +inf sample (L + norm * Ldiff); a NaN lightness lands in
    cell 0 (fminf / fmaxf drop it) and comes out as fmaxf(0, NaN + ...) = 0."""
    ss, sr = dc.BILATERAL_PATHS[path]
    R = dc.BILATERAL_RADIUS[(ss, path)]
    assert R == 4 * ss - 1
    reach = 0
    for h, w in dc.BILATERAL_SHAPES:
        base = oracle.compute_luminance(scene(h, w, 25))
        clean = oracle.bilateral(base, ss, sr, 0.4)
        for case in dc.classes(base, dc.sample_positions(h, w), only=dc.SINGLE):
            (y, x, v), = case.samples
            got = oracle.bilateral(case.frame, ss, sr, 0.4)
            ch = changed(got, clean)
            assert not (ch & ~dc.bilateral_footprint2d(y, x, h, w, ss, path)).any(), case.name
            ys, xs = np.nonzero(ch)
            reach = max(reach, int(np.abs(ys - y).max()), int(np.abs(xs - x).max()))
            bad = ~np.isfinite(got)
            if v == np.inf:
                assert bad.sum() == 1 and got[y, x] == np.inf, case.name
            else:
                assert not bad.any(), case.name
            if np.isnan(v):
                assert got[y, x] == 0.0
        for case in dc.classes(base, {}, only=['negative', 'flat', 'scattered_special']):
            got = oracle.bilateral(case.frame, ss, sr, 0.4)
            assert not np.isnan(got).any() and np.array_equal(np.isinf(got), case.frame == np.inf), case.name
    assert reach >= R - 1, reach


# ------------------------------------------------------------------ NLMeans
def nlm_frame(scene):
    h, w = dc.NLM_SHAPE
    return np.ascontiguousarray(scene(h, w, 1234, 0.03))


@pytest.mark.parametrize('cw', [None, [1.0, 0.25, 0.0]], ids=['weights-1', 'weight-0-on-the-channel'])
def test_nlm_footprint_is_the_references_nan_mask(scene, cw):
    """A NaN in one channel -- the blue one, whose weight is 1 or 0 -- makes every channel of the (2 (S + P) + 1)^2 pixels around it NaN
    and nothing else: cw * d^2 is NaN for cw = 0 as well, so a zero weight does not shield the distance.  An infinity stays inside
    the same box, as NaN (never as an infinity): inf - inf in the patches that hold it (every channel of the (2 P + 1)^2 pixels
    around it), w * inf = 0 * inf where it is a candidate (its own channel, radius S); the float32 and the float64 restatement
    give the same mask, and the same bits as the clean frame outside the box."""
    x = nlm_frame(scene)
    h, w, _ = x.shape
    S_, P_ = dc.NLM_S, dc.NLM_P
    clean32 = nlm_ref(x, S_, P_, 0.1, cw, np.float32)
    for (y, xx) in [(20, 30), (0, 0), (h - 1, w - 2)]:
        fp = dc.nlm_footprint2d(y, xx, h, w, S_, P_)
        for v in NONFINITE:
            f = x.copy()
            f[y, xx, 2] = v
            with np.errstate(all='ignore'):
                got64, got32 = nlm_ref(f, S_, P_, 0.1, cw), nlm_ref(f, S_, P_, 0.1, cw, np.float32)
            bad = np.isnan(got64)
            assert np.array_equal(bad, np.isnan(got32)) and not np.isinf(got64).any() and not np.isinf(got32).any(), (y, xx, v)
            assert not (bad & ~fp[:, :, None]).any(), (y, xx, v)
            if np.isnan(v):
                assert bad[fp].all(), (y, xx)
            else:
                assert bad[dc.box_footprint2d(y, xx, h, w, P_)].all() and bad[dc.box_footprint2d(y, xx, h, w, S_)][:, 2].all(), (y, xx, v)
            assert np.array_equal(got32[~fp], clean32[~fp])
    assert dc.nlm_footprint2d(20, 30, h, w, 3, 1).sum() == 81 and np.isfinite(clean32).all()


def test_nlm_scaled_frames_stay_finite(scene):
    x = nlm_frame(scene)
    for s in (1e3, 1e20):
        for dtype in (np.float64, np.float32):
            with np.errstate(all='ignore'):
                assert np.isfinite(nlm_ref(x * np.float32(s), dc.NLM_S, dc.NLM_P, 0.1 * s, None, dtype)).all(), (s, dtype)


# ------------------------------------------------------------------ wavelet
@pytest.mark.parametrize('scales', [1, 3, 5])
def test_wavelet_footprint_is_the_restatements_changed_set(scales):
    """Radius 2 (2^scales - 1), cut to the frame: the restatement changes nothing outside it, and a NaN makes exactly that box NaN (c_S carries it;
    the shrinkage drops a NaN detail, `|d| > t` being false), an infinity exactly that box non-finite (infinities where c_S carries
    one alone, NaN where inf - inf met)."""
    h, w = dc.WAVELET_SHAPE
    x = np.random.default_rng(50).random((h, w, 1), dtype=np.float32)
    t = np.full((scales, 1), 0.02, np.float32)
    clean = wavelet_ref(x, t)
    assert dc.wavelet_radius(5) == 62
    for y, xx in [(h // 2, w // 2), (0, 0), (h - 1, 3)]:
        fp = dc.wavelet_footprint2d(y, xx, h, w, scales)[:, :, None]
        for v in NONFINITE + dc.HUGE:
            f = x.copy()
            f[y, xx, 0] = v
            with np.errstate(all='ignore'):
                got = wavelet_ref(f, t)
            assert not (changed(got, clean) & ~fp).any(), (scales, y, xx, v)
            if not np.isfinite(v):
                assert np.array_equal(~np.isfinite(got), fp) and (np.isnan(got).sum() == fp.sum() or not np.isnan(v)), (scales, y, xx, v)
            else:
                assert np.isfinite(got).all()


# ------------------------------------------------------------------ the RGB frames of the fused entry points
def test_special_rgb_frame_and_its_lightness(scene, oracle):
    """Every row of color_domain_spec.special_pixels() occurs, at about 1 % of the pixels; the lightness the chain extracts
    (clip to [0, 1] first, fmaxf drops a NaN; log of at least eps) is finite on every pixel, so a special pixel changes the
    denoisers' input at its own place only and by a finite amount."""
    h, w = 96, 128
    rgb = scene(h, w, 5)
    frame, mask, idx = dc.special_rgb_frame(rgb, S.special_pixels())
    assert 0.009 <= mask.mean() <= 0.011 and set(idx[mask]) == set(range(len(S.special_pixels())))
    assert np.array_equal(frame[~mask], rgb[~mask]) and np.isnan(frame).any() and np.isinf(frame).any() and (frame < 0).any() and (frame > 1e30).any()
    for log in (False, True):
        lum = oracle.compute_luminance(frame, log, 1e-4)
        assert np.isfinite(lum).all() and np.array_equal(lum[~mask], oracle.compute_luminance(rgb, log, 1e-4)[~mask])
        assert lum.min() >= (np.float32(np.log(np.float32(1e-4))) if log else 0.0) and lum.max() <= (1e-6 if log else 1.0 + 1e-6)


def test_lab_of_a_clipped_pixel_is_lipschitz_in_its_channels():
    """|d(L, a, b)| <= LAB_LIPSCHITZ * sum_c |d rgb_c| on [0, 1]^3: the bound of the replace step (an RGB pixel, clipped) carries over
    to the (L, a, b) the Lab hand-over returns for it with this factor.  Finite differences of the float64 specification on a
    dense grid, the steepest part (channels below the sRGB knee, t below the Lab knee) resolved: measured 4.5."""
    g = np.concatenate([np.linspace(0, 0.05, 26), np.linspace(0.06, 1.0, 20)])
    px = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3)
    lab = S.A.rgb_to_lab(px)
    worst = 0.0
    for c in range(3):
        q = px.copy()
        q[:, c] = np.minimum(q[:, c] + 1e-4, 1.0)
        step = (q - px)[:, c]
        ok = step > 0
        worst = max(worst, float((np.abs(S.A.rgb_to_lab(q) - lab)[ok] / step[ok, None]).max()))
    print(f'Lab Lipschitz constant over [0, 1]^3: {worst:.3f}')
    assert worst <= dc.LAB_LIPSCHITZ
