"""CPU-only: the input classes of tests/demosaic_cases.py are what their names say, the oracle alone leaves the comparison of
tests/test_gpu_demosaic_domain.py discriminating on them, a second source agrees with the oracle on the finite classes, and two
hand-worked windows pin the oracle where the kernels once differed from it.

Why the second source (the numpy restatements of tests/test_second_source_ppg_postprocess.py) is consulted on the finite classes
only: it takes its medians with `numpy.sort`, which puts NaNs last, whereas the reference's exchange network never moves a NaN -- on
`nonfinite`, and on `overflow` and `half_extremes` (whose sums and differences reach inf - inf), it is a different function.  There
the oracle is pinned by the hand-worked windows below instead."""

import numpy as np
import pytest

import demosaic_cases as C
import test_second_source_ppg_postprocess as S

STORAGES = ['f32', 'f16']
CASES = C.cases()


def all_sites(op, frame):
    return C.sites(*frame, C.TILES[op])


# ------------------------------------------------------------------ the classes hold what their names say
@pytest.mark.parametrize('op', list(C.FRAMES))
def test_special_sites_cover_corner_edge_seams_and_site_classes(op):
    th, tw = C.TILES[op]
    for h, w in C.FRAMES[op]:
        s = all_sites(op, (h, w))
        pos = list(s.values())
        assert len(set(pos)) == len(pos) and all(0 <= y < h and 0 <= x < w for y, x in pos)
        assert s['corner00'] == (0, 0)
        if h * w < 200:   # the frame smaller than one tile: a corner and an edge, no seam
            assert h <= th and w <= tw and s['edge_bottom'][0] == h - 1 and 0 < s['edge_bottom'][1] < w - 1
            continue
        assert s['corner11'] == (h - 1, w - 1) and s['edge_top'][0] == 0 and s['edge_left'][1] == 0
        assert w > tw and s['seam_left'][1] == tw - 1 and s['seam_right'][1] == tw          # every such frame has a vertical seam
        assert h > th and s['seam_above'][0] == th - 1 and s['seam_below'][0] == th         # ... and a horizontal one
        assert {(y & 1, x & 1) for y, x in (s[k] for k in ('site00', 'site01', 'site10', 'site11'))} == {(0, 0), (0, 1), (1, 0), (1, 1)}
        r, cols = C.seam_run(h, w, (th, tw))
        assert cols.start == tw - 2 and cols.stop == tw + 2 and all((r, x) not in pos for x in range(cols.start, cols.stop))


@pytest.mark.parametrize('op', list(C.FRAMES))
def test_classes_contain_what_their_names_say(op):
    tile = C.TILES[op]
    form = C.mosaic if op in ('bilinear', 'ppg') else C.rgb
    for h, w in C.FRAMES[op]:
        big = h * w >= 200
        where = list(all_sites(op, (h, w)).values())
        at = lambda a: np.array([np.ravel(a[p])[0] for p in where])   # noqa: E731  (first channel of each special)
        scene, neg, ties = form('scene', h, w, tile), form('negative', h, w, tile), form('ties', h, w, tile)
        assert np.isfinite(scene).all() and -0.2 < scene.min() and scene.max() < 1.6
        assert np.array_equal(neg, scene - np.float32(0.3)) and ((neg < 0).mean() > 0.1 or not big)
        if big:
            assert (ties == 0).sum() >= 30 and np.signbit(ties[ties == 0]).any() and (ties[2:8, 4:14] == 0.25).all()
            assert (ties[h - 5] == 0.5).mean() > 0.95 and (ties[h - 4] == 0.5).mean() > 0.95   # (a special may sit in the row)
            if ties.ndim == 3:
                assert (ties[9:13, 20:30, 0] == ties[9:13, 20:30, 1]).all() and (ties[9:13, 20:30, 2] == ties[9:13, 20:30, 1]).all()
        ex = form('exponents', h, w, tile)
        mag = np.abs(ex[ex != 0])
        assert np.isfinite(ex).all() and 0.05 < (ex == 0).mean() < 0.2 or not big
        assert (np.abs(at(ex))[:2] == np.float32(1e-41)).all() and np.float32(1e-41) > 0
        if big:
            assert mag.max() >= 2.0 ** 29 and mag[mag > 1e-30].min() <= 2.0 ** -29 and (mag < 1e-35).sum() > w
        ov = form('overflow', h, w, tile)
        assert np.isfinite(ov).all() and np.abs(at(ov)).max() >= np.float32(3e38)
        if big:
            assert (ov >= 2e38).sum() >= 48
        hx = form('half_extremes', h, w, tile)
        assert np.isfinite(hx).all() and at(hx)[0] == 2.0 ** -24 and at(hx)[1] == 65504.0
        assert np.isfinite(C.as_stored(hx, 'f16')).all() != big   # 65520 and beyond: infinities in binary16 storage
        nf = form('nonfinite', h, w, tile)
        assert np.isnan(nf).any() and np.isposinf(nf).any() and (np.isneginf(nf).any() or not big)
        assert np.isfinite(nf).mean() > 0.9
        if big:
            r, cols = C.seam_run(h, w, tile)
            assert np.isnan(nf[r, cols]).all() and np.isfinite(nf[r, cols.start - 1]).all() and np.isfinite(nf[r, cols.stop]).all()
            if nf.ndim == 3:
                px = nf.reshape(-1, 3)
                assert (np.isposinf(px[:, 0]) & np.isposinf(px[:, 1]) & np.isfinite(px[:, 2])).any()      # inf - inf in R - G
                assert (np.isfinite(px[:, 0]) & np.isnan(px[:, 1]) & np.isfinite(px[:, 2])).any()         # a NaN in G alone


def test_pre_median_counts_on_the_scene_and_the_nonfinite_class():
    """The PPG pre-median case (threshold 1.5 / 100) meets a lone in-threshold tap (cnt == 1) on the scene, and a NaN centre
    (cnt == 0) and a NaN neighbour at green sites of the nonfinite class."""
    thr = np.float32(1.5) / np.float32(100)
    for h, w in C.FRAMES['ppg']:
        for name in ('scene', 'nonfinite'):
            raw = C.mosaic(name, h, w, C.TILES['ppg'])
            p = S.padded(raw, 2)
            taps = [(-2, 0), (-1, -1), (-1, 1), (0, -2), (0, 0), (0, 2), (1, -1), (1, 1), (2, 0)]
            vals = np.stack([S.tap(p, 2, dr, dc, h, w) for dr, dc in taps], -1)
            with np.errstate(invalid='ignore'):
                cnt = (np.abs(vals - raw[:, :, None]) < thr).sum(-1)
            for pattern in C.PATTERNS:
                green = C.fc_map(h, w, pattern) == 1
                if name == 'scene':
                    assert (cnt[green] == 1).any() and (cnt[green] > 2).any()
                else:
                    assert (np.isnan(raw) & green & (cnt == 0)).any()
                    assert (~np.isnan(raw) & green & np.isnan(vals).any(-1)).any()


# ------------------------------------------------------------------ the oracle alone: the comparison is discriminating
@pytest.mark.parametrize('op,frame,cfg', CASES, ids=[C.case_id(*c) for c in CASES])
def test_oracle_shares(oracle, op, frame, cfg):
    """At least half of the oracle's result is finite in every class and storage type, and the nonfinite class leaves at least one
    NaN where the operator's last step lets one through (demosaic_cases.NAN_REACHES_THE_RESULT): a condition on the inputs -- a kernel that wiped the
    frame, or one that never produced a NaN, would not pass for free."""
    for name in C.CLASSES:
        for storage in STORAGES:
            ref = C.round_once(C.run_oracle(oracle, op, cfg, C.as_stored(C.input_frame(op, name, frame), storage)), storage)
            finite = np.isfinite(ref).mean()
            assert finite >= 0.5, f'{name} {storage}: finite share {finite:.2f}'
            if name in C.FINITE_CLASSES and storage == 'f32':
                assert finite == 1.0, f'{name}: {finite:.3f}'
            if name == 'nonfinite':   # a NaN where the operator can return one; elsewhere fmaxf(NaN, 0) == 0 and an infinity passes
                assert np.isnan(ref).any() == (op in C.NAN_REACHES_THE_RESULT) and np.isposinf(ref).any(), f'{name} {storage}'


@pytest.mark.parametrize('frame', C.FRAMES['smoothing'], ids=lambda s: f'{s[0]}x{s[1]}')
def test_oracle_shares_combined(oracle, frame):
    for name in C.COMBINED_CLASSES:
        for storage in STORAGES:
            x = C.as_stored(C.input_frame('combined', name, frame), storage)
            for pattern in C.PATTERNS:
                ref = C.round_once(oracle.postprocess(x, oracle.PATTERNS[pattern], **C.COMBINED), storage)
                assert np.isfinite(ref).mean() >= 0.5, (name, storage, pattern)
                # behind the smoothing a green sum is inf or NaN: the ratio is no ordinary quotient, no sum-order bound applies
                s32, _ = oracle.green_eq_sums(oracle.postprocess(x, oracle.PATTERNS[pattern], color_smoothing_passes=5), oracle.PATTERNS[pattern])
                assert not (np.isfinite(s32).all() and (s32 > 0).all()), (name, storage, pattern, s32)


def test_global_green_special_ratios(oracle):
    """The three ratios the global equilibration must share with the oracle: both sums inf (ratio NaN: every G1 site becomes
    max(NaN, 0) = 0), sum1 == 0 and a NaN sum (ratio 1: the greens pass through)."""
    for h, w in C.FRAMES['green_global']:
        for pattern in C.PATTERNS:
            pat = oracle.PATTERNS[pattern]
            g1 = (C.fc_map(h, w, pattern) == 1) & ((np.mgrid[0:h, 0:w][0] & 1) == 0)
            ov = C.rgb('overflow', h, w, C.TILES['green_global'])
            s32, _ = oracle.green_eq_sums(ov, pat)
            assert np.isposinf(s32).all()
            ref = oracle.postprocess(ov, pat, green_eq_global=True)
            assert np.isfinite(ref).all() and (ref[g1][:, 1] == 0).all()
            z = C.green_sum_zero(h, w, pattern)
            assert oracle.green_eq_sums(z, pat)[0][0] == 0.0
            assert np.array_equal(oracle.postprocess(z, pat, green_eq_global=True), np.maximum(z, np.float32(0)))
            for phase in (0, 1):
                n = C.one_nan_green(h, w, pattern, phase)
                assert np.isnan(oracle.green_eq_sums(n, pat)[0][phase]) and np.isnan(n).sum() == 1
                ref = oracle.postprocess(n, pat, green_eq_global=True)
                assert np.array_equal(ref, np.where(np.isnan(n), np.float32(0), np.maximum(n, np.float32(0))))   # fmaxf(NaN, 0) == 0


# ------------------------------------------------------------------ the second source, on the finite classes
@pytest.mark.parametrize('name', C.FINITE_CLASSES)
@pytest.mark.parametrize('frame', C.FRAMES['ppg'], ids=lambda s: f'{s[0]}x{s[1]}')
def test_ppg_second_source_on_the_finite_classes(oracle, name, frame):
    raw = C.mosaic(name, *frame, C.TILES['ppg'])
    for pattern in C.PATTERNS:
        for median in (0.0, 1.5):
            got = S.ppg_2d(raw, pattern, median)
            ref = oracle.ppg(raw, oracle.PATTERNS[pattern], median)
            bad = np.argwhere(got != ref)
            assert bad.size == 0, f'{pattern} median {median}: {len(bad)} mismatches, first at {bad[:5].tolist()}'


@pytest.mark.parametrize('name', C.FINITE_CLASSES)
@pytest.mark.parametrize('frame', C.FRAMES['smoothing'], ids=lambda s: f'{s[0]}x{s[1]}')
def test_postprocess_second_source_on_the_finite_classes(oracle, name, frame):
    h, w = frame
    x = C.rgb(name, h, w, C.TILES['smoothing'])
    y = x
    for passes in range(1, 6):
        y = S.color_smoothing(y)
        if passes in (1, 4, 5):
            assert np.array_equal(y, oracle.postprocess(x, oracle.RGGB, color_smoothing_passes=passes)), f'{passes} passes'
    for pattern in C.PATTERNS:
        color = S.fc_map(h, w, S.WORDS[pattern])
        for thr in (0.04, 4.0):
            got = S.green_eq_local(x, color, np.float32(thr / 100.0))
            assert np.array_equal(got, oracle.postprocess(x, oracle.PATTERNS[pattern], green_eq_local=True, green_eq_threshold=thr)), (pattern, thr)


# ------------------------------------------------------------------ two hand-worked windows
def cswap_network(s):
    """the 19 exchanges of the reference's median of nine (csrc/reduction.h:93-116), in Python floats"""
    s = list(s)
    for a, b in [(1, 2), (4, 5), (7, 8), (0, 1), (3, 4), (6, 7), (1, 2), (4, 5), (7, 8), (0, 3), (5, 8), (4, 7), (3, 6), (1, 4), (2, 5),
                 (4, 7), (4, 2), (6, 4), (4, 2)]:
        if s[a] > s[b]:
            s[a], s[b] = s[b], s[a]
    return s[4]


def test_median_window_with_one_nan(oracle):
    """A 3 x 3 frame, G = 0.5 and B = 0.5 everywhere, R - G = the window in raster order: the centre pixel's red is
    max(median9(window) + 0.5, 0).

    Window A = [1, 2, 3, 4, NaN, 6, 7, 8, 9], the NaN in slot 4 (the centre).  An exchange (a, b) swaps only if s[a] > s[b]; every
    pair of finite slots is already in order and a comparison with the NaN is false, so NONE of the 19 exchanges swaps: s[4] stays
    NaN, NaN + 0.5 = NaN, fmaxf(NaN, 0) = 0.  Any selection by min / max that drops the NaN returns one of 4 .. 6 instead.

    Window B = [9, NaN, 1, 8, 2, 7, 3, 6, 4], the NaN in slot 1.  Exchanges that swap, in order: (7,8) 6<>4; (3,4) 8<>2; (4,5) 8<>7;
    (0,3) 9<>2; (5,8) 8<>6; (4,7) 7<>4; (3,6) 9<>3; then (1,4) compares the NaN: no swap; (2,5) 1 < 6, (4,7) 4 < 7: none; (4,2) 4 > 1
    swaps, (6,4) 9 > 1 swaps, (4,2) 9 > 4 swaps: s[4] = 4 -> red 4.5.  The NaN blocks slot 1 -- exchange (1,4) would have moved the
    column minimum there -- and 4 comes out, the fourth of the eight finite values."""
    nan = float('nan')
    for window, want in (([1, 2, 3, 4, nan, 6, 7, 8, 9], 0.0), ([9, nan, 1, 8, 2, 7, 3, 6, 4], 4.5)):
        m = cswap_network(window)
        assert (np.isnan(m) and want == 0.0) or m + 0.5 == want
        x = np.full((3, 3, 3), 0.5, np.float32)
        x[:, :, 0] = np.array(window, np.float32).reshape(3, 3) + np.float32(0.5)
        got = oracle.postprocess(x, oracle.RGGB, color_smoothing_passes=1)
        assert got[1, 1, 0] == np.float32(want) and got[1, 1, 1] == 0.5 and got[1, 1, 2] == 0.5


def test_bilinear_zero_weight_tap_is_not_dropped(oracle):
    """A 5 x 5 RGGB mosaic of ones; the centre (2, 2) is a red site: R = 16 c / 16, G = (4 (l + r + t + b) + 8 c - 2 (the four at
    distance 2)) / 16, B = (4 (the four diagonals) + 12 c - 3 (the four at distance 2)) / 16 -- and every other tap enters with
    weight 0, as a product.

    +inf on the diagonal (1, 1): R = 16 + 0 * inf = NaN, G = .. + 0 * inf = NaN, B = 4 * inf + finite = +inf.
    +inf on the diagonal (1, 1) AND on the axial neighbour (2, 3): B = 4 * inf + 0 * inf = NaN too -- every channel is NaN.
    A NaN anywhere in the diamond is NaN in every channel; a sample outside the diamond, (0, 0), is not read at all."""
    for specials, want_nan, want_inf in (([(1, 1)], [True, True, False], [False, False, True]), ([(1, 1), (2, 3)], [True] * 3, [False] * 3)):
        m = np.ones((5, 5), np.float32)
        for p in specials:
            m[p] = np.inf
        got = oracle.bilinear5x5(m, oracle.RGGB)[2, 2]
        assert np.isnan(got).tolist() == want_nan and np.isposinf(got).tolist() == want_inf, got
    m = np.ones((5, 5), np.float32)
    m[3, 2] = np.nan
    assert np.isnan(oracle.bilinear5x5(m, oracle.RGGB)[2, 2]).all()
    m = np.ones((5, 5), np.float32)
    m[0, 0] = np.inf
    assert np.array_equal(oracle.bilinear5x5(m, oracle.RGGB)[2, 2], np.ones(3, np.float32))


def test_white_balance_oracle_is_finite_everywhere(oracle):
    """clamp(x * gain, 0, 1) = fminf(fmaxf(.., 0), 1): a NaN product (0 * inf, NaN) is 0, every other one lands in [0, 1]."""
    h, w = C.WB_FRAME
    for name in C.CLASSES:
        for storage in STORAGES:
            x = C.as_stored(C.mosaic(name, h, w, (h, w)), storage)
            for gains in C.WB_GAINS:
                assert {0.0, 3e38} <= set(gains) and min(gains) < 0
                for pattern in C.PATTERNS:
                    ref = oracle.apply_white_balance(x, np.array(gains, np.float32), oracle.PATTERNS[pattern])
                    assert np.isfinite(ref).all() and ref.min() >= 0 and ref.max() <= 1
