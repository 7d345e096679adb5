"""GPU: the four denoisers (Wiener, Bilateral, NLMeans, Wavelet) over their whole input domain -- negative, scaled by 10^-3 .. 10^6,
flat, subnormal, binary16 extremes, huge, overflowing, infinite and NaN samples -- against oracle.wiener, oracle.bilateral, nlm_ref
and wavelet_ref.  Value classes, frames and footprints: tests/denoise_cases.py; every claim about the references that is relied on
here is checked without a GPU in tests/test_denoise_cases.py.  Measured maxima (the MEASURED lines): profiles/r28/denoise_domain.txt.

1. Wiener.  Finite classes: the whole frame within F32 * scale of oracle.wiener (binary16 results: half an ulp more), F32 = 2e-5 as
   in test_gpu_wiener_geometry.py, scale PER PIXEL = max(1, largest |input| of the tile pairs that cover the pixel).
   Single samples: outside the sample's footprint the result has the bits of the same call on the frame without the sample (no
   atomics, a fixed summation order: a condition, not a tolerance); other channels of an interleaved frame keep their bits
   everywhere.  NaN / +-inf: the non-finite pixels are EXACTLY the footprint.
   The footprint is the kernels': two horizontally adjacent tiles (tile columns 2 m, 2 m + 1) are the real and the imaginary part
   of one complex transform (wiener_stream, wiener_ystream), so the partner of every tile that reads the sample shares its
   rounding errors and its NaN: up to K / ov columns more than the oracle's tile union on either side, the same rows
   (denoise_cases.wiener_footprint(pairs=True); include/tdk_hip_wiener.h states it).  Every pixel of the oracle's own footprint is
   inside and non-finite, as the oracle's is.
   single_overflowing (1e30, 3e38; float32 only -- binary16 has no such number): the oracle's gain is inf / inf = NaN over the box.
   The kernels evaluate max(GS - 4 sigma^2 GS * rcp(p4), 0) with rcp(inf) = 0: the gain of every overflowing bin is exactly the
   pass-through gain, and a sample of this size overflows every bin of every tile that holds it (|X| >= |v| * 1.7e-4 - |v| / 46:
   window product at the tile corner, mean term) -- the tiles return their input.  That is what float64 gives (gain
   1 - sigma^2 / 1e52 = 1), so inside the footprint the kernels are held to the float64 restatement wiener_fp64 within F32 * |v|,
   and outside to the clean call's bits.  3e38 stays finite on the way (|Z| = |A + i B| <= 2 * 0.09 * 3e38) EXCEPT in the tile
   mean, a float32 sum: a tile within K of a frame edge reads the sample twice (once mirrored), 2 * 3e38 is infinite, and that
   tile and its partner are NaN.  The non-finite set is exactly what those tiles write (denoise_cases.wiener_sum_overflow2d:
   empty for 1e30, and for 3e38 away from the edges); every other pixel is held to float64 as said.
   scattered_special: the tame values (SPECIAL14 without +-1e30, +-inf, NaN) as a finite class; all 14: non-finite on the union of
   the oracle footprints of the NaN / +-inf samples, the tame frame's bits outside the union of the kernels' footprints of the five
   untamed ones (at 1 % of the pixels that union is most of the frame: the mask is the assertion).
2. Fused Lab-chain entry points on color_domain_spec.special_pixels() scattered over a scene: ordinary pixels within TOL (lightness)
   and 2 TOL (chroma, RGB) of the oracle composition, special pixels with the oracle's NaN / inf mask and, where finite, within
   color_domain_spec's GPU bound of the replace step (+ the chain tolerance; x denoise_cases.LAB_LIPSCHITZ for the Lab form);
   every lightness plane handed on is finite.
3. Bilateral.process: the oracle's values with np.array_equal's equality (binary16: rounded once), NaN masks first.
4. NLMeans: 4 x the float32-restatement floor + 2^-23, relative to the scale; NaN masks of nlm_ref.  A NaN in a channel of weight 0
   poisons the same pixels in every channel (0 * NaN in the patch distance), in nlm_ref and in the kernel.  Wavelet: the
   restatement's bits wherever it is not NaN, the same NaN mask.
5. State: after a frame with NaN and +-inf every operator returns, for a clean frame, the bits a fresh object returns.

Tried on mutated copies of the kernels (each fails here): the gain without its fmaxf (every finite Wiener class, from `negative`
on, and the log-lightness entry points); `L * rcp(sigma_r)` for `L / sigma_r` in the grid path's cell coordinate (22 values of
test_bilateral_plane_domain[grid-*-f32]; binary16 rounding hides it); the splat's column accumulators not cleared
(test_bilateral_plane_domain[grid-*], the grid entry points, and test_state_bilateral[grid]: a NaN survives the call).

Kernel instantiation (csrc/)                         reached by                                      classes
  wiener_ystream<float|half>, general body            test_wiener_domain[K32ov4-*]                    all of 1.
  wiener_ystream<float|half>, interior body           test_wiener_domain_interior_body                negative, scaled, single_*
  wiener_stream<T, 16, 4>, <T, 32, 2>                 test_wiener_domain[K16ov4-*, K32ov2-*]          all of 1.
  wiener_finish<T> (C = 1), wiener_finish3<T, 4|1>    test_wiener_domain[*-C1-*], [*-C3-*] (W % 4 == 0: K32ov2, K16ov4; 1: K32ov4)
  lum_lab_extract<T, 4|1> (+ bounds)                  test_wiener_lab_entry_points_on_special_pixels  special RGB pixels
  wiener_finish_modify<T, 4|1>                        test_wiener_log_luminance_on_special_pixels     special RGB pixels
  wiener_finish_lab<4|1>                              test_wiener_lab_entry_points_on_special_pixels  special RGB pixels
  bilateral_tile_kernel<T, T, 0, 4|1>                 test_bilateral_plane_domain[tiles-*]            negative, flat, single_*, scattered
  splat / blur / slice_kernel<T>                      test_bilateral_plane_domain[grid-*]             the same
  bilateral_tile_kernel<float, T, 1|2|3, 4|1>         test_bilateral_entry_points_on_special_pixels[tiles-*]
  slice_modify_kernel<T, LOG, 4|1>, slice_lab_kernel  test_bilateral_entry_points_on_special_pixels[grid-*]
  nlmeans tile kernel <C = 1, 3>                      test_nlmeans_domain, test_nlmeans_nan_*         negative, scaled, flat, NaN, +-inf
  wavelet fused kernels (1, F), (3, F), (3, T)        test_wavelet_domain                             NaN, +-inf, huge, subnormal
  every workspace                                     test_state_*                                    scattered_special, then clean"""

import numpy as np
import pytest
import torch

import color_domain_spec as S
import denoise_cases as dc
from test_gpu_fallback_paths import at_offset, f16_ulp, gpu, npf, oracle_lab
from test_gpu_lab_chain import TOL
from test_gpu_nlmeans import nlm_ref
from test_gpu_wavelet import MODES, make as make_wavelet, thresholds as wavelet_thresholds
from test_gpu_wiener_geometry import F32, RGB_SIGMAS, held
from test_oracle_second_source import wiener_fp64
from test_wavelet_spec import wavelet_ref

pytestmark = pytest.mark.gpu

DTYPES = {'f32': torch.float32, 'f16': torch.float16}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a visible MI355X'
    return torch.device('cuda', 0)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.int16, 4: np.int32}[a.dtype.itemsize])


def same_bits(a, b):
    """Elementwise: the same bits (so -0 is not +0, and a NaN equals only the same NaN)."""
    return bits(a) == bits(b)


def raw(t):
    return t.detach().cpu().numpy()


# ================================================================== 1. Wiener, every kernel
WIENER_CONFIGS = [(K, ov, C, dt) for (K, ov) in dc.WIENER_FRAMES for C in (1, 3) for dt in DTYPES]


@pytest.mark.parametrize('K,ov,C,dt', WIENER_CONFIGS, ids=[f'K{K}ov{ov}-C{C}-{dt}' for K, ov, C, dt in WIENER_CONFIGS])
def test_wiener_domain(td, oracle, dev, scene, K, ov, C, dt):
    """Every class of denoise_cases.classes at every position, on the 3 x 3-workgroup frame of the (K, ov) pair."""
    wiener_domain(td, oracle, dev, scene, K, ov, C, dt, dc.WIENER_FRAMES[(K, ov)], dc.wiener_positions(K, ov), None)


@pytest.mark.parametrize('C,dt', [(1, 'f32'), (1, 'f16'), (3, 'f32')])
def test_wiener_domain_interior_body(td, oracle, dev, scene, C, dt):
    """The strip kernel's guard-free interior body (W % 4 == 0, a workgroup clear of every edge): the single_* classes with the
    sample inside interior workgroup (1, 1) and on its seam with (2, 2), and two whole-frame classes.  The interior body reads a
    plane (C = 1); the interleaved call on the same frame runs the general body with vector loads in every strip."""
    from torch_darktable import _native

    w, h = dc.WIENER_INTERIOR_FRAME
    q = _native.lib.tdk_wiener_strip_interior
    assert q(w, h, 8, 1, 1) == 1 and q(w, h, 8, 2, 2) == 1 and q(w, h, 8, 0, 1) == 0 and q(*dc.WIENER_FRAMES[(32, 4)], 8, 1, 1) == 0
    wiener_domain(td, oracle, dev, scene, 32, 4, C, dt, (w, h), dc.WIENER_INTERIOR_POSITIONS, ['negative', 'scaled'] + list(dc.SINGLE))


def wiener_domain(td, oracle, dev, scene, K, ov, C, dt, size, positions, only):
    w, h = size
    rgb = scene(h, w, 7)
    ws = td.Wiener(dev, (w, h), overlap_factor=ov, tile_size=K)
    half = dt == 'f16'
    ch = 1 if C == 3 else 0   # the channel that carries the class

    def device_frame(case):
        return gpu(dc.rgb_case(case, rgb) if C == 3 else case.frame[:, :, None], dev, DTYPES[dt])

    def sigmas(case):
        return (RGB_SIGMAS if C == 3 else RGB_SIGMAS[:1]) * np.float32(case.sigma_scale)

    def run(x, sig):
        out = ws.process(x, gpu(sig, dev))
        assert out.dtype == DTYPES[dt] and out.shape == x.shape
        return out

    def scale_of(case, x32):
        sc = np.empty(x32.shape)
        for c in range(C):
            sc[:, :, c] = dc.wiener_scale(case, K, ov) if c == ch else max(1.0, float(np.abs(x32[:, :, c]).max()))
        return sc

    def outside_is_clean(got, clean_got, kfp, what):
        g, c = raw(got), raw(clean_got)
        same = same_bits(g, c)
        for k in range(C):
            bad = ~same[:, :, k] & (~kfp if k == ch else True)
            assert not bad.any(), f'{what}: channel {k}: {bad.sum()} values outside the footprint differ from the clean call, first at {np.argwhere(bad)[0].tolist()}'

    cases = dc.classes(rgb[:, :, 1], positions, only)
    clean_x = gpu(rgb if C == 3 else rgb[:, :, 1:2], dev, DTYPES[dt])
    clean_got = run(clean_x, RGB_SIGMAS[:C])
    tame_got = None
    for case in cases:
        if half:
            case = dc.as_f16(case)
            if case is None:
                continue
        what = f'wiener K={K} ov={ov} {w}x{h} C={C} {dt} {case.name}'
        x = device_frame(case)
        x32, sig = npf(x), sigmas(case)
        got = run(x, sig)
        if case.kind == 'finite':
            ref = oracle.wiener(x32, sig, K, ov)
            worst = held(got, ref, F32 * scale_of(case, x32), what, half=half)
            if case.name == 'scaled[0.001]':
                print(f'MEASURED {what}: max |d| {worst:.3e} = {worst / 1e-3:.3e} of the frame\'s scale')
            if case.name.startswith('single_huge'):
                (y, xx, v), = case.samples
                outside_is_clean(got, clean_got, dc.wiener_footprint2d(y, xx, h, w, K, ov, pairs=True), what)
            if case.name == 'scattered_special[tame]':
                tame_got = got
        elif case.kind in ('nonfinite', 'overflowing'):
            (y, xx, v), = case.samples
            kfp = dc.wiener_footprint2d(y, xx, h, w, K, ov, pairs=True)
            outside_is_clean(got, clean_got, kfp, what)
            g = npf(got)[:, :, ch]
            if case.kind == 'nonfinite':
                assert not np.isfinite(g[dc.wiener_footprint2d(y, xx, h, w, K, ov)]).any(), f'{what}: a finite value inside the oracle\'s footprint'
                assert np.array_equal(~np.isfinite(g), kfp), f'{what}: non-finite set {(~np.isfinite(g)).sum()} pixels, footprint {kfp.sum()}'
            else:
                assert not half
                nan = dc.wiener_sum_overflow2d(y, xx, v, h, w, K, ov)   # tiles whose float32 sample sum overflows (3e38 read twice)
                assert np.array_equal(~np.isfinite(g), nan), f'{what}: {(~np.isfinite(g)).sum()} non-finite values, {nan.sum()} derived'
                ref = wiener_fp64(x32[:, :, ch], float(sig[ch]), K, ov).astype(np.float32)
                ref[nan] = g[nan] = 0.0
                held(torch.from_numpy(g), ref, F32 * scale_of(case, x32)[:, :, ch], what + ' vs float64')
        else:
            assert case.kind == 'mixed' and (half or tame_got is not None)
            g = npf(got)[:, :, ch]
            wild = [(y, xx, v) for y, xx, v in case.samples if not dc.is_tame(v)]
            nonfinite = dc.union([dc.wiener_footprint2d(y, xx, h, w, K, ov) for y, xx, v in wild if not np.isfinite(v)], (h, w))
            assert not np.isfinite(g[nonfinite]).any(), what
            if tame_got is not None:   # (binary16 turns 2^40 and 2^41 into infinities: no tame frame there)
                reach = dc.union([dc.wiener_footprint2d(y, xx, h, w, K, ov, pairs=True) for y, xx, v in wild], (h, w))
                outside_is_clean(got, tame_got, reach, what)
                print(f'MEASURED {what}: {int((~reach).sum())} pixels outside the union of footprints, {int(nonfinite.sum())} inside the non-finite union')


# ================================================================== 2. fused Lab-chain entry points on special RGB pixels
CHAIN_SHAPE = (96, 128)   # W % 4 == 0: the aligned call runs the vector instantiations, the offset view the scalar ones
BOUNDS = (0.03, 1.61)


def chain_frame(scene, dt, bounds=False):
    """(float32 values as the kernel reads them after storage in `dt`, mask of the special pixels).  With bounds the frame is what
    normalises to about the plain one: special values are placed after the affine map, so the same specials arrive."""
    h, w = CHAIN_SHAPE
    rgb = scene(h, w, 5)
    if bounds:
        rgb = rgb * np.float32(BOUNDS[1] - BOUNDS[0]) + np.float32(BOUNDS[0])
    frame, mask, _ = dc.special_rgb_frame(rgb, S.special_pixels())
    with np.errstate(over='ignore'):
        return (frame.astype(np.float16).astype(np.float32) if dt == 'f16' else frame), mask


def views(t, dt):
    """The aligned tensor and one contiguous view 4 (binary16: 2) bytes past an aligned allocation."""
    return [('aligned', t), ('offset', at_offset(t, 4 if dt == 'f32' else 2))]


def replace_bound(op, px, lum):
    """color_domain_spec's GPU bound of the replace step on pixels px (N, 3) with the new (log-)lightness lum (N,)."""
    with np.errstate(all='ignore'):
        r, sens, scale, pre = S.evaluate_with_sensitivity(op, np.concatenate([px, lum[:, None]], 1).astype(np.float32))
        return S.bound(op, sens, scale, pre, S.GPU_FACTOR)


def check_rgb(got, ref, mask, b, what):
    """Ordinary pixels within 2 TOL of the oracle composition; special pixels: the oracle's NaN positions and infinities, finite
    values within 1.125 x the replace step's bound (the oracle itself lies within an eighth of it, test_gpu_color_domain.py) plus
    the chain's 2 TOL.  binary16 results: half an ulp more."""
    half = got.dtype == torch.float16
    g = npf(got)
    extra = 0.5 * f16_ulp(np.maximum(np.abs(np.where(np.isfinite(g), g, 1.0)), np.abs(np.where(np.isfinite(ref), ref, 1.0)))) if half else 0.0
    d = np.abs(g - ref)
    print(f'MEASURED {what}: ordinary pixels max |d| {d[~mask].max():.3e}')
    bad = ~(d <= 2 * TOL + extra) & ~mask[:, :, None]
    assert not bad.any(), f'{what}: {bad.sum()} ordinary values beyond 2 TOL, first at {np.argwhere(bad)[0].tolist()}, max {d[~mask].max():.3e}'
    gs, rs, es = g[mask], ref[mask], (extra[mask] if half else 0.0)
    assert np.array_equal(np.isnan(gs), np.isnan(rs)), f'{what}: NaN positions of the special pixels differ at {np.argwhere(np.isnan(gs) != np.isnan(rs))[:3].tolist()}'
    inf = np.isinf(gs) | np.isinf(rs)
    assert np.array_equal(gs[inf], rs[inf]), f'{what}: infinities of the special pixels differ'
    fin = np.isfinite(gs) & np.isfinite(rs)
    with np.errstate(all='ignore'):
        bad = fin & ~(np.abs(gs - rs) <= 1.125 * b + 2 * TOL + es)
    assert not bad.any(), f'{what}: {bad.sum()} special values beyond the bound, first: kernel {gs[bad][0]!r} oracle {rs[bad][0]!r} bound {b[bad][0]!r}'


@pytest.mark.parametrize('dt', list(DTYPES))
def test_wiener_log_luminance_on_special_pixels(td, oracle, dev, scene, dt):
    """Wiener.process_log_luminance: lum_extract + the planar strip kernel + wiener_finish_modify<T, 4> (aligned) / <T, 1> (offset)."""
    h, w = CHAIN_SHAPE
    x32, mask = chain_frame(scene, dt)
    ll = oracle.compute_luminance(x32, True, 1e-4)
    assert np.isfinite(ll).all()
    den = oracle.wiener(ll[:, :, None], 0.075, 32, 4)[:, :, 0]
    ref = oracle.modify_luminance(x32, den, True)
    b = replace_bound('modify_log_luminance', x32[mask], den[mask])
    ws = td.Wiener(dev, (w, h), overlap_factor=4, tile_size=32)
    for name, t in views(gpu(x32, dev, DTYPES[dt]), dt):
        lum = torch.full((h, w), float('nan'), device=dev)
        got = ws.process_log_luminance(t, 0.075, luminance_out=lum)
        assert got.dtype == DTYPES[dt]
        check_rgb(got, ref, mask, b, f'process_log_luminance {dt} {name}')
        assert torch.isfinite(lum).all(), f'{name}: luminance_out is not finite everywhere'


@pytest.mark.parametrize('with_bounds', [False, True], ids=['plain', 'bounds'])
@pytest.mark.parametrize('dt', list(DTYPES))
def test_wiener_lab_entry_points_on_special_pixels(td, oracle, dev, scene, dt, with_bounds):
    """Wiener.process_log_luminance_lab: lum_lab_extract<T, 4|1> (with and without the folded bounds) + wiener_finish_lab<4|1>.
    Ordinary pixels: lightness within TOL, (a, b) within 2 TOL of oracle_lab.  Special pixels: the oracle's NaN / inf mask (the
    oracle's pixel is clipped to [0, 1], so its Lab is finite: so must the kernel's be), finite values within
    LAB_LIPSCHITZ * sum over the channels of 1.125 x the replace step's bound, plus the chain tolerance."""
    h, w = CHAIN_SHAPE
    stored, mask = chain_frame(scene, dt, with_bounds)
    b0, b1 = np.float32(BOUNDS[0]), np.float32(BOUNDS[1])
    with np.errstate(all='ignore'):
        x32 = ((stored - b0) / (b1 - b0)).astype(np.float32) if with_bounds else stored   # normalize_image's float32 expression
    lum_ref, ab_ref, _ = oracle_lab(oracle, x32)
    assert np.isfinite(lum_ref).all() and np.isfinite(ab_ref).all()
    ll = oracle.compute_luminance(x32, True, 1e-4)
    den = oracle.wiener(ll[:, :, None], 0.075, 32, 4)[:, :, 0]
    slack = dc.LAB_LIPSCHITZ * 1.125 * np.nansum(replace_bound('modify_log_luminance', x32[mask], den[mask]), 1)
    ws = td.Wiener(dev, (w, h), overlap_factor=4, tile_size=32)
    kw = dict(bounds=torch.tensor(BOUNDS, device=dev)) if with_bounds else {}
    for name, t in views(gpu(stored, dev, DTYPES[dt]), dt):
        lum, ab = ws.process_log_luminance_lab(t, 0.075, **kw)
        what = f'process_log_luminance_lab {dt} {"bounds" if with_bounds else "plain"} {name}'
        l, a = raw(lum), raw(ab)
        assert np.isfinite(l).all() and np.isfinite(a).all(), f'{what}: a non-finite lightness or chroma is handed on'
        dl, da = np.abs(l - lum_ref), np.abs(a - ab_ref)
        print(f'MEASURED {what}: ordinary pixels max |dL| {dl[~mask].max():.3e} |dab| {da[~mask].max():.3e}; special pixels {dl[mask].max():.3e} {da[mask].max():.3e}')
        assert dl[~mask].max() <= TOL and da[~mask].max() <= 2 * TOL, what
        assert (dl[mask] <= TOL + slack).all() and (da[mask] <= 2 * TOL + slack[:, None]).all(), what


@pytest.mark.parametrize('dt', list(DTYPES))
@pytest.mark.parametrize('path', list(dc.BILATERAL_PATHS))
def test_bilateral_entry_points_on_special_pixels(td, oracle, dev, scene, path, dt):
    """Bilateral.process_rgb / process_log_rgb / process_lab: the tile kernel's epilogues (tiles) and slice_modify_kernel /
    slice_lab_kernel (grid), vector (aligned) and scalar (offset) instantiations."""
    h, w = CHAIN_SHAPE
    ss, sr = dc.BILATERAL_PATHS[path]
    x32, mask = chain_frame(scene, dt)
    bil = td.Bilateral(dev, (w, h), sigma_s=ss, sigma_r=sr)
    t0 = gpu(x32, dev, DTYPES[dt])
    for log, eps in ((False, None), (True, 1e-6)):
        plane = oracle.compute_luminance(x32, log, eps if log else 1e-4)
        assert np.isfinite(plane).all()
        new = oracle.bilateral(plane, ss, sr, 0.4)
        ref = oracle.modify_luminance(x32, new, log)
        b = replace_bound('modify_log_luminance' if log else 'modify_luminance', x32[mask], new[mask])
        for name, t in views(t0, dt):
            got = bil.process_log_rgb(t, 0.4, eps) if log else bil.process_rgb(t, 0.4)
            assert got.dtype == DTYPES[dt]
            check_rgb(got, ref, mask, b, f'Bilateral.process_{"log_" if log else ""}rgb {path} {dt} {name}')
        assert torch.isfinite(td.compute_log_luminance(t0.float(), eps) if log else td.compute_luminance(t0.float())).all()
    # process_lab: the pixel as (lightness, chroma); the chroma of a special pixel may be NaN or infinite, the lightness is finite
    lum = oracle.compute_luminance(x32)
    with np.errstate(all='ignore'):
        ab = np.ascontiguousarray(oracle.color_op('rgb_to_lab', x32)[:, :, 1:])
    assert not np.isfinite(ab).all()
    new = oracle.bilateral(lum, ss, sr, 0.4)
    ref = oracle.modify_luminance(x32, new, False)
    b = replace_bound('modify_luminance', x32[mask], new[mask])
    lt, at = gpu(lum, dev), gpu(ab, dev)
    for name, lv, av in (('aligned', lt, at), ('offset', at_offset(lt, 4), at_offset(at, 8))):
        got = bil.process_lab(lv, av, 0.4, out_dtype=DTYPES[dt])
        check_rgb(got, ref, mask, b, f'Bilateral.process_lab {path} {dt} {name}')


# ================================================================== 3. bilateral plane against the oracle's bits
@pytest.mark.parametrize('dt', list(DTYPES))
@pytest.mark.parametrize('shape', dc.BILATERAL_SHAPES, ids=[f'{w}x{h}' for h, w in dc.BILATERAL_SHAPES])
@pytest.mark.parametrize('path', list(dc.BILATERAL_PATHS))
def test_bilateral_plane_domain(td, oracle, dev, scene, path, shape, dt):
    """Bilateral.process = the oracle's bits (binary16: the oracle's float32 result rounded once) on negative, flat, every single_*
    class at every position and scattered_special: NaN positions first (the oracle shows none: a NaN lightness lands in cell 0
    and leaves as fmaxf(0, NaN) = 0), then every value with np.array_equal's equality, the contract of
    test_bilateral_plane_offset_views: a zero equals a zero.  (flat[-0.0]: the last step is fmaxf(0, -0), whose sign C leaves open;
    the oracle's libm returns -0, v_max_f32 returns +0.)"""
    h, w = shape
    ss, sr = dc.BILATERAL_PATHS[path]
    base = oracle.compute_luminance(scene(h, w, 25))
    bil = td.Bilateral(dev, (w, h), sigma_s=ss, sigma_r=sr)
    n = 0
    for case in dc.classes(base, dc.sample_positions(h, w), only=['negative', 'flat'] + list(dc.SINGLE) + ['scattered_special']):
        if dt == 'f16':
            case = dc.as_f16(case)
            if case is None:
                continue
        x = gpu(case.frame, dev, DTYPES[dt])
        got = raw(bil.process(x, 0.4))
        ref = oracle.bilateral(npf(x), ss, sr, 0.4)
        with np.errstate(over='ignore'):
            want = ref if dt == 'f32' else ref.astype(np.float16)
        what = f'bilateral {path} {w}x{h} {dt} {case.name}'
        assert got.dtype == want.dtype
        assert np.array_equal(np.isnan(got), np.isnan(want)), f'{what}: NaN positions differ at {np.argwhere(np.isnan(got) != np.isnan(want))[:3].tolist()}'
        bad = ~(got == want) & ~np.isnan(want)
        assert not bad.any(), f'{what}: {bad.sum()} values differ, first at {np.argwhere(bad)[0].tolist()}: {got[bad][0]!r} against {want[bad][0]!r}'
        n += 1
    assert n >= (40 if dt == 'f32' else 25), n


# ================================================================== 4. NLMeans and Wavelet
def nlm_run(td, dev, x, h, cw):
    H, W, _ = x.shape
    out = td.NLMeans(dev, (W, H), dc.NLM_S, dc.NLM_P).process(gpu(x, dev), float(h), cw)
    return raw(out).astype(np.float64)


def nlm_held(td, dev, x, h, cw, scale, what):
    """The rule of tests/test_gpu_nlmeans.py relative to `scale`: |kernel - ref64| <= 4 * floor + 2^-23 * scale, floor =
    max |ref32 - ref64| on this input, over the values nlm_ref leaves finite; the NaN mask is nlm_ref's and nothing is infinite."""
    with np.errstate(all='ignore'):
        r64, r32 = nlm_ref(x, dc.NLM_S, dc.NLM_P, h, cw), nlm_ref(x, dc.NLM_S, dc.NLM_P, h, cw, np.float32)
    got = nlm_run(td, dev, x, h, cw)
    assert np.array_equal(np.isnan(got), np.isnan(r64)) and not np.isinf(got).any(), f'{what}: NaN mask {np.isnan(got).sum()} values, nlm_ref {np.isnan(r64).sum()}'
    ok = ~np.isnan(r64)
    floor = float(np.abs(r32.astype(np.float64) - r64)[ok].max())
    tol = 4.0 * floor + 2.0 ** -23 * scale
    err = float(np.abs(got - r64)[ok].max())
    print(f'MEASURED {what}: gpu err {err / scale:.3e} floor {floor / scale:.3e} tol {tol / scale:.3e} (of the scale {scale:g})')
    assert err <= tol, (what, err, floor, tol)
    return got


def nlm_image(scene):
    h, w = dc.NLM_SHAPE
    return np.ascontiguousarray(scene(h, w, 1234, 0.03))


def test_nlmeans_domain_finite_classes(td, dev, scene):
    x = nlm_image(scene)
    cw = [0.3, 2.0, 0.7]
    nlm_held(td, dev, x * np.float32(7.0) - np.float32(3.0), 0.7, cw, 4.0, 'nlmeans negative')
    nlm_held(td, dev, x * np.float32(1e3), 0.1 * 1e3, cw, 1e3, 'nlmeans scaled[1e3]')
    nlm_held(td, dev, x * np.float32(1e20), 0.1 * 1e20, None, 1e20, 'nlmeans scaled[1e20]')
    for c in dc.FLAT_VALUES:
        got = nlm_held(td, dev, np.full(x.shape, c, np.float32), 0.1, None, max(1.0, abs(c)), f'nlmeans flat[{c!r}]')
        assert np.abs(got - c).max() <= 2.0 ** -23 * max(1.0, abs(c))


@pytest.mark.parametrize('channel,cw', [(1, [1.0, 0.25, 0.0]), (0, None), (2, [1.0, 0.25, 0.0])], ids=['weight-0.25', 'weights-1', 'weight-0'])
def test_nlmeans_nan_and_infinities(td, dev, scene, channel, cw):
    """A NaN or an infinity in one channel: the NaN mask of nlm_ref (inside the Chebyshev box of S + P, every channel for a NaN),
    the finite rule elsewhere.  weight-0: the sample sits in a channel whose weight is 0 -- the kernel forms (d * cw) * d, which is
    NaN all the same, so the channel is not shielded: the same mask as nlm_ref, whose cw * d^2 is NaN too."""
    x = nlm_image(scene)
    h, w, _ = x.shape
    for y, xx in [(20, 30), (0, 0), (h - 1, w - 2)]:
        for v in (dc.NAN, dc.INF, -dc.INF):
            f = x.copy()
            f[y, xx, channel] = v
            got = nlm_held(td, dev, f, 0.1, cw, 1.0, f'nlmeans {float(v)} in channel {channel} cw={cw} at {(y, xx)}')
            fp = dc.nlm_footprint2d(y, xx, h, w, dc.NLM_S, dc.NLM_P)
            assert not np.isnan(got[~fp]).any() and (not np.isnan(v) or np.isnan(got[fp]).all())


@pytest.mark.parametrize('channels,ycc', MODES)
def test_wavelet_domain(td, dev, channels, ycc):
    """float32 frames with a NaN, an infinity, +-1e18 or scattered subnormals, three scales: the restatement's bits wherever it is
    not NaN and the same NaN mask (payloads are not compared)."""
    h, w = dc.WAVELET_SHAPE
    base = np.random.default_rng(60 + channels).random((h, w, channels), dtype=np.float32)
    t = wavelet_thresholds(3, channels, 7)
    wv = make_wavelet(td, dev, base, t, ycc)
    frames = []
    for pname, (y, x) in dc.sample_positions(h, w).items():
        for v in [dc.NAN, dc.INF, -dc.INF] + dc.HUGE:
            f = base.copy()
            f[y, x, channels // 2] = v
            frames.append((f'{float(v):g}@{pname}', f))
    sub = base.copy()
    for c in range(channels):
        sub[:, :, c] = dc._scatter(base[:, :, c], dc.SUBNORMALS, 8 + c)[0]
    frames.append(('subnormal', sub))
    for name, f in frames:
        got = raw(wv.process(gpu(f, dev)))
        with np.errstate(all='ignore'):
            want = wavelet_ref(f, t, ycc)
        what = f'wavelet C={channels} ycc={ycc} {name}'
        assert np.array_equal(np.isnan(got), np.isnan(want)), f'{what}: NaN mask {np.isnan(got).sum()} values, restatement {np.isnan(want).sum()}'
        bad = ~same_bits(got, want) & ~np.isnan(want)
        assert not bad.any(), f'{what}: {bad.sum()} values differ, first at {np.argwhere(bad)[0].tolist()}: {got[bad][0]!r} against {want[bad][0]!r}'


# ================================================================== 5. state after a special frame
def poison_plane(base):
    """scattered_special[all] of the plane (NaN, +-inf, +-1e30 among its values)."""
    f = [c for c in dc.classes(base, {}, only=['scattered_special']) if c.kind == 'mixed'][0].frame
    assert np.isnan(f).any() and np.isinf(f).any()
    return f


@pytest.mark.parametrize('last_only', [False, True], ids=['everywhere', 'last-partial-strip'])
@pytest.mark.parametrize('K,ov', [(32, 4), (16, 4)])
def test_state_wiener(td, dev, scene, K, ov, last_only):
    """Slabs, carried seam columns and the slab regions of absent tiles: a frame with NaN and +-inf (everywhere; or only in the last
    partial strip / group and segment / band, whose slabs hold the regions of absent tiles), then a clean frame on the same object,
    for process (C = 1, 3), process_log_luminance and process_log_luminance_lab: the bits of a fresh object."""
    w, h = dc.WIENER_FRAMES[(K, ov)]
    G, TR = dc.WIENER_GROUP[(K, ov)]
    s = K // ov
    rgb, other = scene(h, w, 7), scene(h, w, 8)
    if last_only:
        # the first tile of the last group starts at x0 * s, y0 * s; its tiles read from K before that on (the overlap, mirrored reads)
        x0, y0 = ((w - 1) // s + ov - 1) // G * G - (ov - 1), ((h - 1) // s + ov - 1) // TR * TR - (ov - 1)
        bad_plane, other0 = other[:, :, 1].copy(), other[:, :, 0].copy()
        for k, v in enumerate([np.nan, np.inf, -np.inf, 1e30]):
            bad_plane[max(y0 * s - K, 0) + 3 * k, w - 1 - k] = v
            bad_plane[h - 1 - k, max(x0 * s - K, 0) + 5 * k] = v
            other0[h - 1 - 2 * k, w - 1 - 3 * k] = v
    else:
        bad_plane, other0 = poison_plane(other[:, :, 1]), poison_plane(other[:, :, 0])
    bad_rgb = other.copy()
    bad_rgb[:, :, 1], bad_rgb[:, :, 0] = bad_plane, other0
    clean1, clean3 = gpu(rgb[:, :, 1:2], dev), gpu(rgb, dev)
    entries = {'process C=1': lambda o: (o.process(clean1, 0.05),), 'process C=3': lambda o: (o.process(clean3, gpu(RGB_SIGMAS, dev)),),
               'process_log_luminance': lambda o: (o.process_log_luminance(clean3, 0.075),), 'process_log_luminance_lab': lambda o: o.process_log_luminance_lab(clean3, 0.075)}
    poisons = {'plane': lambda o: o.process(gpu(bad_plane[:, :, None], dev), 0.05), 'rgb': lambda o: o.process(gpu(bad_rgb, dev), 0.05),
               'log-L of rgb': lambda o: o.process_log_luminance_lab(gpu(bad_rgb, dev), 0.075)}
    for ename, entry in entries.items():
        fresh = [t.clone() for t in entry(td.Wiener(dev, (w, h), overlap_factor=ov, tile_size=K))]
        assert all(torch.isfinite(t).all() for t in fresh)
        for pname, poison in poisons.items():
            ws = td.Wiener(dev, (w, h), overlap_factor=ov, tile_size=K)
            left = poison(ws)
            assert pname == 'log-L of rgb' or not torch.isfinite(left).all()
            for a, b in zip(entry(ws), fresh):
                assert torch.equal(a, b), f'K={K} ov={ov} {ename} after a special frame through {pname}: {(a != b).sum().item()} values differ from a fresh object\'s'


@pytest.mark.parametrize('path', list(dc.BILATERAL_PATHS))
def test_state_bilateral(td, oracle, dev, scene, path):
    """The grid and the axis tables: process and process_lab on a special frame, then on a clean one."""
    h, w = dc.BILATERAL_SHAPES[0]
    ss, sr = dc.BILATERAL_PATHS[path]
    rgb = scene(h, w, 25)
    lum = oracle.compute_luminance(rgb)
    ab = np.ascontiguousarray(oracle.color_op('rgb_to_lab', rgb)[:, :, 1:])
    other = oracle.compute_luminance(scene(h, w, 26))
    bad = poison_plane(other)
    bad_ab = ab.copy()
    bad_ab[~same_bits(bad, other)] = np.nan
    lt, at, bt, bat = gpu(lum, dev), gpu(ab, dev), gpu(bad, dev), gpu(bad_ab, dev)
    fresh = td.Bilateral(dev, (w, h), sigma_s=ss, sigma_r=sr)
    want, want_lab = fresh.process(lt, 0.4).clone(), fresh.process_lab(lt, at, 0.4).clone()
    for poison in ('process', 'process_lab'):
        bil = td.Bilateral(dev, (w, h), sigma_s=ss, sigma_r=sr)
        if poison == 'process':
            assert torch.isinf(bil.process(bt, 0.4)).any()   # (+inf at the pixel of a +inf sample)
        else:
            bil.process_lab(bt, bat, 0.4)   # (the result is clipped to [0, 1]: nothing to see in it)
        assert torch.equal(bil.process(lt, 0.4), want), f'{path}: process after a special frame through {poison}'
        assert torch.equal(bil.process_lab(lt, at, 0.4), want_lab), f'{path}: process_lab after a special frame through {poison}'


def test_state_nlmeans_and_wavelet(td, dev, scene):
    """NLMeans keeps no frame data between calls and the wavelet's scratch planes are rewritten by every call: the same bits after
    a frame with NaN and +-inf as from a fresh object (Wavelet at five scales, every mode)."""
    x = nlm_image(scene)
    h, w, _ = x.shape
    bad = x.copy()
    bad[:, :, 1] = poison_plane(x[:, :, 1])
    nl = td.NLMeans(dev, (w, h), dc.NLM_S, dc.NLM_P)
    assert not torch.isfinite(nl.process(gpu(bad, dev), 0.1)).all()
    assert torch.equal(nl.process(gpu(x, dev), 0.1), td.NLMeans(dev, (w, h), dc.NLM_S, dc.NLM_P).process(gpu(x, dev), 0.1))
    hh, ww = dc.WAVELET_SHAPE
    for channels, ycc in MODES:
        base = np.random.default_rng(70).random((hh, ww, channels), dtype=np.float32)
        t = wavelet_thresholds(5, channels, 9)
        poisoned = base.copy()
        poisoned[:, :, 0] = poison_plane(base[:, :, 0])
        wv = make_wavelet(td, dev, base, t, ycc)
        assert not torch.isfinite(wv.process(gpu(poisoned, dev))).all()
        assert torch.equal(wv.process(gpu(base, dev)), make_wavelet(td, dev, base, t, ycc).process(gpu(base, dev))), (channels, ycc)
