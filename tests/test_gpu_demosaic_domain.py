"""GPU: bilinear, PPG, the PostProcess stages and the per-site white balance over their whole input domain.

The other tests of these kernels run the synthetic scene and uniform noise in [0, 1): finite, no ties.  Here they run the classes of
tests/demosaic_cases.py -- negative frames, ties, exponents from 2^-30 to 2^30 and subnormals, finite samples whose sums overflow
inside the operator, the binary16 extremes, NaN and +-inf -- on the smallest frames that take each path of each kernel, under the
four patterns, in float32 and binary16 storage, through the drop-in surface.  The contract is T0 of tests/test_gpu_parity.py:

  values    equal to the C oracle's on the same input, every value that is not a NaN (an infinity equals itself; the sign of a zero
            is not compared: the outputs end in max(x, 0), whose zero C leaves open);
  NaN       at exactly the oracle's positions (all NaNs are one pattern);
  binary16  the oracle sees the rounded input, and its float32 result is rounded once;
  global green equilibration: the sum-order bound of test_gpu_parity.py::test_postprocess_global_green_eq where the oracle's ratio
            is finite and not the fall-back, the oracle's values otherwise.

tests/test_demosaic_cases.py holds the classes to their names, checks on the CPU that at least half of every oracle result is
finite, and pins the oracle on two hand-worked windows.  A failure reports the class, the count, the first five positions and
whether values or the NaN mask differ."""

import numpy as np
import pytest
import torch

import demosaic_cases as C

pytestmark = pytest.mark.gpu

DTYPES = {'f32': torch.float32, 'f16': torch.float16}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a visible MI355X'
    return torch.device('cuda', 0)


def gpu(a, dev, storage='f32'):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(DTYPES[storage])


def npf(t):
    return t.detach().float().cpu().numpy()


_references = {}


def reference(key, compute):
    """an oracle result, computed once per module, shared by the tests, never modified"""
    if key not in _references:
        ref = compute()
        ref.setflags(write=False)
        _references[key] = ref
    return _references[key]


def differences(got, ref):
    """(kind, positions) of the first kind of difference, or None"""
    gn, rn = np.isnan(got), np.isnan(ref)
    if not np.array_equal(gn, rn):
        return 'NaN mask', np.argwhere(gn != rn)
    with np.errstate(invalid='ignore'):
        bad = ~rn & (got != ref)
    return ('value', np.argwhere(bad)) if bad.any() else None


def hold(got, ref, what):
    d = differences(got, ref)
    if d is not None:
        kind, pos = d
        first = [(p.tolist(), float(got[tuple(p)]), float(ref[tuple(p)])) for p in pos[:5]]
        pytest.fail(f'{what}: {kind} differs at {len(pos)} of {ref.size} values; first (position, got, oracle): {first}')


def stored_input(op, name, frame, storage):
    return C.as_stored(C.input_frame(op, name, frame), storage)


def oracle_result(oracle, op, frame, cfg, name, storage):
    return reference((op, frame, tuple(cfg.items()), name, storage),
                     lambda: C.round_once(C.run_oracle(oracle, op, cfg, stored_input(op, name, frame, storage)), storage))


def classes_and_storages(fn):
    fn = pytest.mark.parametrize('storage', list(DTYPES))(fn)
    return pytest.mark.parametrize('name', C.CLASSES)(fn)


# ------------------------------------------------------------------ bilinear
# tile 128 x 16, 4 x 2 pixels per thread; vec_ok = width % 4 == 0 and a 16-byte aligned output.
#   20 x 136: grid 2 x 2 (136 > 128, 20 > 16), 136 % 4 == 0 -> the 16-byte stores
#   19 x 131: grid 2 x 2, 131 % 4 != 0 -> scalar stores; odd width and height: the last thread's `x + k < width` and `y + r >= height`
#   5 x 6:    smaller than one tile: every tap clamps
@pytest.mark.parametrize('frame', C.FRAMES['bilinear'], ids=lambda s: f'{s[0]}x{s[1]}')
@classes_and_storages
def test_bilinear(td, oracle, dev, name, storage, frame):
    h, w = frame
    assert (w % 4 == 0) == (frame == (20, 136)) and ((w > 128 and h > 16) or frame == (5, 6))
    x = gpu(stored_input('bilinear', name, frame, storage)[:, :, None], dev, storage)
    for pattern in C.PATTERNS:
        ref = oracle_result(oracle, 'bilinear', frame, dict(pattern=pattern), name, storage)
        got = td.bilinear5x5_demosaic(x, td.BayerPattern[pattern])
        assert got.dtype == DTYPES[storage]
        hold(npf(got), ref, f'bilinear {name} {storage} {h}x{w} {pattern}')


# ------------------------------------------------------------------ PPG
# tile 64 x 32, 4-pixel raw halo; INTERIOR = x0 >= 8 and y0 >= 8 and x0 + 72 <= width and y0 + 40 <= height.
#   100 x 200: 4 x 4 tiles; (tx, ty) = (1, 1) and (2, 1) are INTERIOR (64 + 72 <= 200, 128 + 72 <= 200, 32 + 40 <= 100), the ring
#              variant runs on all four sides; 200 % 4 == 0 -> 16-byte stores
#   33 x 70:   2 x 2 tiles (<= 2 tile columns: the row-major tile order), no INTERIOR tile, 70 % 4 != 0 -> scalar stores
# median_threshold 1.5 runs the pre-median kernel first: tests/test_demosaic_cases.py shows that the nonfinite class holds a NaN
# centre (cnt == 0) and a NaN neighbour at green sites, and the scene a lone in-threshold tap (cnt == 1).
def ppg_interior_tiles(h, w):
    return [(tx, ty) for ty in range(-(-h // 32)) for tx in range(-(-w // 64))
            if tx * 64 >= 8 and ty * 32 >= 8 and tx * 64 + 72 <= w and ty * 32 + 40 <= h]


@pytest.mark.parametrize('median', [0.0, 1.5])
@pytest.mark.parametrize('frame', C.FRAMES['ppg'], ids=lambda s: f'{s[0]}x{s[1]}')
@classes_and_storages
def test_ppg(td, oracle, dev, name, storage, frame, median):
    h, w = frame
    assert ppg_interior_tiles(h, w) == ([(1, 1), (2, 1)] if frame == (100, 200) else []) and (w % 4 == 0) == (frame == (100, 200))
    x = gpu(stored_input('ppg', name, frame, storage)[:, :, None], dev, storage)
    for pattern in C.PATTERNS:
        ref = oracle_result(oracle, 'ppg', frame, dict(pattern=pattern, median=median), name, storage)
        got = td.PPG(dev, (w, h), td.BayerPattern[pattern], median_threshold=median).process(x)
        assert got.dtype == DTYPES[storage]
        hold(npf(got), ref, f'PPG {name} {storage} {h}x{w} {pattern} median {median}')


# ------------------------------------------------------------------ PostProcess
# colour smoothing: tile 64 x 16, at most four passes per launch -> passes 1 (one launch), 4 (a full launch), 5 (two launches);
# local equilibration: tile 64 x 16, the 4-pixel vector form or the scalar form.  Both choose by width % 4 and alignment:
#   40 x 136: 136 % 4 == 0 -> 16-byte staging and stores; 3 x 3 tiles, the last column 8 wide (cols != 64: its scalar store loop)
#   37 x 70:  70 % 4 != 0 -> the scalar paths; 2 x 3 tiles
# The specials on both sides of the seams (columns 63 | 64, rows 15 | 16) and the NaN run across column 64 lie within 4 pixels of a
# seam: their footprint, one pixel wider per pass, crosses it inside a fused launch.
def postprocess(td, dev, frame, pattern, x, **kw):
    h, w = frame
    got = td.PostProcess(dev, (w, h), td.BayerPattern[pattern], **kw).process(x)
    assert got.dtype == x.dtype and got.shape == x.shape
    return npf(got)


@pytest.mark.parametrize('passes', [1, 4, 5])
@pytest.mark.parametrize('frame', C.FRAMES['smoothing'], ids=lambda s: f'{s[0]}x{s[1]}')
@classes_and_storages
def test_colour_smoothing(td, oracle, dev, name, storage, frame, passes):
    assert (frame[1] % 4 == 0) == (frame == (40, 136)) and frame[1] > 64 and frame[0] > 16
    cfg = dict(pattern='RGGB', passes=passes)
    x = gpu(stored_input('smoothing', name, frame, storage), dev, storage)
    ref = oracle_result(oracle, 'smoothing', frame, cfg, name, storage)
    hold(postprocess(td, dev, frame, 'RGGB', x, **C.postprocess_args('smoothing', cfg)), ref, f'smoothing {name} {storage} {frame} passes {passes}')


@pytest.mark.parametrize('threshold', [0.04, 4.0])
@pytest.mark.parametrize('frame', C.FRAMES['green_local'], ids=lambda s: f'{s[0]}x{s[1]}')
@classes_and_storages
def test_local_green_equilibration(td, oracle, dev, name, storage, frame, threshold):
    """The specials sit on all four (row, column) parities, so under the four patterns on G2 sites, on their diagonal (G1) and
    same-phase neighbours, and -- the corner and edge samples -- in the 2-pixel ring whose taps leave the frame."""
    x = gpu(stored_input('green_local', name, frame, storage), dev, storage)
    for pattern in C.PATTERNS:
        cfg = dict(pattern=pattern, threshold=threshold)
        ref = oracle_result(oracle, 'green_local', frame, cfg, name, storage)
        hold(postprocess(td, dev, frame, pattern, x, **C.postprocess_args('green_local', cfg)), ref,
             f'local green eq {name} {storage} {frame} {pattern} threshold {threshold}')


def hold_global(oracle, got, x, pattern, storage, what):
    """R, B and the G2 sites: the oracle's values.  G1 sites: the oracle's values where its ratio is not an ordinary quotient (a sum
    that is not positive or not finite: the fall-back 1, NaN, inf or 0); otherwise within the sum-order bound.  Each fp32 sum carries
    an absolute error of at most (tree depth + chain length) * 2^-24 * sum |g| -- the oracle's 16 x 16 block trees (depth 8) then B
    block sums in sequence, the kernel's 8 + 12 -- that is a relative error of that times kappa = sum |g| / |sum g| (1 for the positive
    frames of test_postprocess_global_green_eq, more where signs mix); the ratio doubles it, and the quotient's and the product's own
    roundings (2^-24 each, and one binary16 rounding of a value that differs by that much: half a binary16 ulp) come on top."""
    h, w, _ = x.shape
    pat = oracle.PATTERNS[pattern]
    ref = oracle.postprocess(x, pat, green_eq_global=True)
    s32, _ = oracle.green_eq_sums(x, pat)
    ordinary = bool(np.isfinite(s32).all() and (s32 > 0).all())
    g1 = np.zeros((h, w, 3), bool)
    g1[:, :, 1] = (C.fc_map(h, w, pattern) == 1) & ((np.mgrid[0:h, 0:w][0] & 1) == 0)
    if not ordinary:
        hold(got, C.round_once(ref, storage), what + ' (ratio not an ordinary quotient)')
        return
    hold(np.where(g1, 0, got), np.where(g1, 0, C.round_once(ref, storage)), what + ' (R, B, G2)')
    green = x[:, :, 1].astype(np.float64)
    rows = np.mgrid[0:h, 0:w][0]
    inimg = (np.mgrid[0:h, 0:w][1] < 2 * (w // 2)) & (rows < 2 * (h // 2)) & (C.fc_map(h, w, pattern) == 1)
    kappa = max(np.abs(green[inimg & ((rows & 1) == p)]).sum() / abs(green[inimg & ((rows & 1) == p)].sum()) for p in (0, 1))
    blocks = ((h + 15) // 16) * ((w + 15) // 16)
    bound = 2.0 * ((8 + blocks) + (8 + 12)) * 2.0 ** -24 * kappa + 2.0 ** -22
    a, b = got[g1], ref[g1]
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b)), what + ': non-finite G1 positions differ'
    fin = np.isfinite(b)
    tol = bound * np.abs(b[fin]) + (2.0 ** -11 * np.abs(b[fin]) + 2.0 ** -25 if storage == 'f16' else 0.0)
    over = np.abs(a[fin].astype(np.float64) - b[fin]) > tol
    assert not over.any(), f'{what}: {over.sum()} G1 values beyond the sum-order bound {bound:.2e} (kappa {kappa:.2f})'


@pytest.mark.parametrize('frame', C.FRAMES['green_global'], ids=lambda s: f'{s[0]}x{s[1]}')
@classes_and_storages
def test_global_green_equilibration(td, oracle, dev, name, storage, frame):
    xs = stored_input('green_global', name, frame, storage)
    x = gpu(xs, dev, storage)
    for pattern in C.PATTERNS:
        hold_global(oracle, postprocess(td, dev, frame, pattern, x, green_eq_global=True), xs, pattern, storage,
                    f'global green eq {name} {storage} {frame} {pattern}')


@pytest.mark.parametrize('storage', list(DTYPES))
@pytest.mark.parametrize('frame', C.FRAMES['green_global'], ids=lambda s: f'{s[0]}x{s[1]}')
def test_global_green_equilibration_special_ratios(td, oracle, dev, frame, storage):
    """Both sums inf (the overflow class: ratio NaN, every G1 site max(NaN, 0) = 0), sum1 == 0 and a NaN in either sum (ratio 1):
    tests/test_demosaic_cases.py::test_global_green_special_ratios shows the oracle's side; the kernel's must be the same values."""
    h, w = frame
    for pattern in C.PATTERNS:
        pat = oracle.PATTERNS[pattern]
        frames = {'both sums inf': C.rgb('overflow', h, w, C.TILES['green_global']), 'sum1 == 0': C.green_sum_zero(h, w, pattern),
                  'NaN in sum1': C.one_nan_green(h, w, pattern, 0), 'NaN in sum2': C.one_nan_green(h, w, pattern, 1)}
        for what, a in frames.items():
            xs = C.as_stored(a, storage)
            s32, _ = oracle.green_eq_sums(xs, pat)
            assert not (np.isfinite(s32).all() and (s32 > 0).all())
            ref = C.round_once(oracle.postprocess(xs, pat, green_eq_global=True), storage)
            hold(postprocess(td, dev, frame, pattern, gpu(xs, dev, storage), green_eq_global=True), ref, f'global green eq, {what}, {storage} {frame} {pattern}')


@pytest.mark.parametrize('storage', list(DTYPES))
@pytest.mark.parametrize('frame', C.FRAMES['smoothing'], ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('name', C.COMBINED_CLASSES)
def test_combined_stages(td, oracle, dev, name, frame, storage):
    """Five smoothing passes (two launches), the global and the local equilibration in one call: the stages' ping-pong carries the
    specials from one stage into the next.  In both classes a green sum is inf or NaN under every pattern, so the ratio is no
    ordinary quotient and the whole result is held to the oracle's values."""
    xs = stored_input('combined', name, frame, storage)
    x = gpu(xs, dev, storage)
    for pattern in C.PATTERNS:
        pat = oracle.PATTERNS[pattern]
        s32, _ = oracle.green_eq_sums(oracle.postprocess(xs, pat, color_smoothing_passes=5), pat)
        assert not (np.isfinite(s32).all() and (s32 > 0).all()), s32
        ref = C.round_once(oracle.postprocess(xs, pat, **C.COMBINED), storage)
        hold(postprocess(td, dev, frame, pattern, x, **C.COMBINED), ref, f'combined {name} {storage} {frame} {pattern}')


# ------------------------------------------------------------------ white balance
@pytest.mark.parametrize('storage', list(DTYPES))
@pytest.mark.parametrize('name', C.CLASSES)
def test_white_balance(td, oracle, dev, name, storage):
    """clamp(sample * gain, 0, 1) on a 6 x 10 plane, gains with 0, a negative value and 3e38 in every slot: 0 * inf and
    inf * negative reach the clamp; fmaxf(NaN, 0) == 0 in both implementations.  One pattern also runs on a view that starts one
    element into its allocation."""
    h, w = C.WB_FRAME
    xs = C.as_stored(C.mosaic(name, h, w, (h, w)), storage)
    x = gpu(xs, dev, storage)
    for gains in C.WB_GAINS:
        g = np.array(gains, np.float32)
        for pattern in C.PATTERNS:
            ref = C.round_once(oracle.apply_white_balance(xs, g, oracle.PATTERNS[pattern]), storage)
            got = td.apply_white_balance(x, gpu(g, dev), td.BayerPattern[pattern])
            assert got.dtype == DTYPES[storage]
            hold(npf(got), ref, f'white balance {name} {storage} {pattern} gains {gains}')
            if pattern == 'GRBG':
                pool = torch.zeros(x.numel() + 8, dtype=x.dtype, device=dev)
                view = pool[1:1 + x.numel()].view(x.shape)
                view.copy_(x)
                assert view.is_contiguous() and view.data_ptr() % 16 == x.element_size()
                hold(npf(td.apply_white_balance(view, gpu(g, dev), td.BayerPattern[pattern])), ref, f'white balance {name} {storage} +1 element')
