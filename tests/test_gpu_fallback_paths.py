"""GPU: the scalar fallbacks of the streaming kernels, run as whole images.

Almost every streaming kernel in csrc/ has a vector path (four pixels per thread, 16-byte accesses) and a scalar fallback the
launcher picks when a buffer is not aligned, when width % 4 != 0 or for the last npix % 4 pixels (`grep -n tdk_aligned csrc/*.hip`).
The rest of the suite runs the vector paths at many shapes; here every fallback runs on a whole image: on contiguous views that
start 2, 4 or 8 bytes past an aligned allocation (frame i of an (N, H, W, 3) batch, a plane carved out of a larger pool), at
widths where the vector path would otherwise run (W % 4 == 0), and on aligned images with npix % 4 in {1, 2, 3} (vector body +
a tail with first > 0).  Each case is held to the oracle with the tolerance of the existing aligned test of the op, and to the
aligned call on the same values (bit for bit where the code claims the same bits).  Each test names the kernel instantiation
it is meant to reach.

Dispatch site (csrc/)                          fallback driven by
  color.hip   run_color_t                      test_color_ops_offset_views_and_tails, test_grid_stride_loops_at_50mp
  color.hip   run_extract                      test_luminance_extract_offset_views_and_tails, test_grid_stride_loops_at_50mp
  color.hip   run_modify                       test_luminance_modify_offset_views_and_tails
  color.hip   tdk_compute_log_luminance_lab    test_wiener_lab_offset_views_and_tails
  color.hip   run_normalize                    test_normalize_image_offset_views, test_normalize_image_on_batch_frames
  tonemap.hip run_tonemap                      test_tonemaps_u8_offset_views_and_tails, test_grid_stride_loops_at_50mp
  wiener.hip  launch_tiles_ys / _ov (vec_ok)   test_wiener_offset_views
  wiener.hip  launch, C = 3 (wiener_finish3)   test_wiener_offset_views[3]
  wiener.hip  launch_log_luminance (finish)    test_wiener_log_luminance_offset_views
  wiener.hip  launch_log_luminance_lab         test_wiener_lab_offset_views_and_tails
  wiener.hip  launch_tiles_ys_lum              not built (TDK_EXPERIMENTS only)
  bilateral.hip launch (plane, tiles)          test_bilateral_plane_offset_views[tiles]
  bilateral.hip launch_rgb (tiles, slice)      test_bilateral_rgb_offset_views
  bilateral.hip launch_lab (tiles)             test_bilateral_lab_offset_views[tiles]
  rcd.hip     launch_mixed (wide_ok, stream)   test_rcd_offset_bayer
  codec.hip   run_decode                       test_gpu_parity.py::test_codec_unaligned_views (the output is always allocated)
  codec.hip   run_encode                       test_codec_encode_offset_views
  codec.hip   tdk_decode12_wb_plane            test_rcd_packed12_offset_views
  postprocess.hip aligned4 (vec_in)            test_postprocess_offset_views; vec_ok (output) only by width % 4 != 0 (test_gpu_parity.py)
  bilinear.hip / ppg.hip vec_ok                the test is on the output, which the wrappers allocate: only width % 4 != 0 reaches it
                                               (test_gpu_parity.py); offset mosaics: test_ppg_bilinear_offset_bayer
  tonemap.hip metrics acc, whitebalance.hip chroma, jpeg.hip workspace: alignment REQUIREs on library-allocated buffers."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 2e-5          # the colour operators' tolerance (tests/test_gpu_parity.py, tests/test_gpu_lab_chain.py)
F32_OFFSETS = [4, 8]
F16_OFFSETS = [2, 4, 8]
DT_OFFSETS = [(torch.float32, o) for o in F32_OFFSETS] + [(torch.float16, o) for o in F16_OFFSETS]
PATTERNS = ['RGGB', 'BGGR', 'GRBG', 'GBRG']


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a visible MI355X'
    return torch.device('cuda', 0)


def npy(t):
    return t.detach().cpu().numpy()


def npf(t):
    """float32 numpy copy (binary16 widened exactly)."""
    return t.detach().float().cpu().numpy()


def gpu(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t if dtype is None else t.to(dtype)


def at_offset(t, offset):
    """A contiguous copy of CUDA tensor `t` that starts `offset` bytes past an aligned allocation: a view into a larger buffer,
    as frame i of a batch or a slice of a pool is.  Asserts the alignment it claims, so a case cannot quietly run the vector
    path (offset % 16 == 0 is refused: use the tensor itself)."""
    es = t.element_size()
    assert offset % es == 0 and offset % 16 != 0, (offset, es)
    k = offset // es
    pool = torch.zeros(t.numel() + k + 16 // es, dtype=t.dtype, device=t.device)
    assert pool.data_ptr() % 256 == 0
    v = pool[k:k + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == offset % 16, (v.data_ptr() % 16, offset)
    return v


def f16_ulp(v):
    """One binary16 ulp of |v| (normal range)."""
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -14))) - 10)


def assert_close(got, ref, tol, what, rounded=False):
    """float32 results within `tol` of the oracle; binary16 results are the fp32 result rounded once: `tol` + half an ulp -- one
    ulp against a `rounded` reference (another binary16 result: the two fp32 values may round to neighbours)."""
    g = npf(got)
    bound = tol if got.dtype == torch.float32 else tol + (1.0 if rounded else 0.5) * f16_ulp(np.maximum(np.abs(g), np.abs(ref)))
    d = np.abs(g - ref)
    bad = d > bound
    assert not bad.any(), f'{what}: {bad.sum()} values beyond the bound, first at {np.argwhere(bad)[:3].tolist()}, max |d| {d.max()}'


def assert_u8_ties(got, ref_u8, ref_f, what):
    """test_gpu_parity.py::test_tonemaps_u8: +-1 LSB, only where the pre-quantisation value sits on a rounding tie."""
    d = np.abs(npy(got).astype(np.int32) - ref_u8.astype(np.int32))
    assert got.dtype == torch.uint8 and d.max() <= 1, (what, d.max())
    frac = np.abs((ref_f * 255.0) - np.floor(ref_f * 255.0) - 0.5)
    assert (frac[d > 0] < 2e-3).all() and (d > 0).mean() < 2e-3, (what, (d > 0).mean(), frac[d > 0].max() if (d > 0).any() else None)


# ------------------------------------------------------------------ colour operators (color.hip: color_vec4 / color_tail)
COLOR_CASES = [('rgb_to_xyz', None), ('xyz_to_lab', None), ('lab_to_xyz', None), ('xyz_to_rgb', None), ('rgb_to_lab', None),
               ('lab_to_rgb', None), ('modify_hsl', (0.1, 0.3, -0.2)), ('modify_vibrance', (0.6,)), ('color_transform_3x3', None)]
MATRIX = np.array([[1.2, -0.1, -0.1], [-0.05, 1.1, -0.05], [0.0, -0.2, 1.2]], np.float32)


def _color_call(td, name, t, params, dev):
    if name == 'color_transform_3x3':
        return td.color_transform_3x3(t, gpu(MATRIX, dev))
    return getattr(td, name)(t, *(params or ()))


def _color_ref(oracle, name, img32, params):
    if name == 'color_transform_3x3':
        return oracle.color_op(name, img32, MATRIX)
    return oracle.color_op(name, img32, params)


@pytest.mark.parametrize('name,params', COLOR_CASES, ids=[c[0] for c in COLOR_CASES])
def test_color_ops_offset_views_and_tails(td, oracle, dev, scene, name, params):
    """color_tail<OP, float> / color_tail<OP, __half> over the whole image (views 4 / 8 B (f32) and 2 / 4 B (f16) off: the vector
    path wants 4 * sizeof(T); f16 +8 B is 8-B aligned and so takes color_vec4<OP, __half>), and color_vec4 + color_tail(first > 0)
    on aligned images with npix % 4 in {1, 2, 3}."""
    def source(h, w, seed):
        img = scene(h, w, seed)
        return oracle.color_op('rgb_to_lab', img) if name in ('lab_to_xyz', 'lab_to_rgb') else img

    img = source(48, 64, 19)  # W % 4 == 0: the vector path would run on an aligned buffer
    for dt, off in DT_OFFSETS:
        t = gpu(img, dev, dt)
        img32 = npf(t)
        ref = _color_ref(oracle, name, img32, params)
        aligned = _color_call(td, name, t, params, dev)
        got = _color_call(td, name, at_offset(t, off), params, dev)
        what = f'{name} {dt} +{off} B'
        assert got.dtype == dt
        if name == 'color_transform_3x3' and dt == torch.float32:  # test_gpu_parity.py::test_color_transform_3x3: the oracle's bits
            assert np.array_equal(npy(got), ref) and torch.equal(got, aligned), what
        else:
            assert_close(got, ref, TOL, what)
            assert_close(got, npf(aligned), TOL, what + ' vs aligned', rounded=True)
    for h, w in ((37, 61), (38, 61), (39, 61)):  # npix % 4 = 1, 2, 3
        src = source(h, w, h)
        got = _color_call(td, name, gpu(src, dev), params, dev)
        ref = _color_ref(oracle, name, src, params)
        if name == 'color_transform_3x3':
            assert np.array_equal(npy(got), ref), (name, h, w)
        else:
            assert_close(got, ref, TOL, f'{name} {h}x{w}')


# ------------------------------------------------------------------ luminance extract / replace (color.hip)
@pytest.mark.parametrize('log', [False, True], ids=['linear', 'log'])
def test_luminance_extract_offset_views_and_tails(td, oracle, dev, scene, log):
    """lum_extract_tail<TR, TL, LOG> over the whole image for offset rgb (the vector path wants 16 B for rgb and plane), and
    lum_extract_vec4 + lum_extract_tail(first > 0) on aligned images with npix % 4 in {1, 2, 3}; the tolerance of
    test_gpu_parity.py::test_luminance_extract_replace (2e-5), plus half a binary16 ulp for a binary16 plane."""
    def extract(t):
        return td.compute_log_luminance(t, 1e-4) if log else td.compute_luminance(t)

    img = scene(48, 64, 21)
    for dt, off in DT_OFFSETS:
        t = gpu(img, dev, dt)
        ref = oracle.compute_luminance(npf(t), log, 1e-4)
        got, aligned = extract(at_offset(t, off)), extract(t)
        assert got.dtype == dt and got.shape == (48, 64)
        assert_close(got, ref, TOL, f'{dt} +{off} B')
        assert_close(got, npf(aligned), TOL, f'{dt} +{off} B vs aligned', rounded=True)
    for h, w in ((37, 61), (38, 61), (39, 61)):
        src = scene(h, w, h + 1)
        for dt in (torch.float32, torch.float16):
            t = gpu(src, dev, dt)
            assert_close(extract(t), oracle.compute_luminance(npf(t), log, 1e-4), TOL, f'{h}x{w} {dt}')


LUM_PAIRS = [(torch.float32, torch.float32), (torch.float16, torch.float32), (torch.float16, torch.float16), (torch.float32, torch.float16)]


@pytest.mark.parametrize('log', [False, True], ids=['linear', 'log'])
@pytest.mark.parametrize('rgb_dt,lum_dt', LUM_PAIRS, ids=['f32-f32', 'f16-f32', 'f16-f16', 'f32-f16'])
def test_luminance_modify_offset_views_and_tails(td, oracle, dev, scene, log, rgb_dt, lum_dt):
    """lum_modify_tail<TR, TL, LOG> for every (rgb, plane) dtype pair modify_luminance accepts, with the rgb, the plane or both
    offset (each breaks the vector path's 16-B requirement), and lum_modify_vec4 + lum_modify_tail(first > 0) on aligned
    images with npix % 4 in {1, 2, 3}: the tolerance of test_luminance_extract_replace (5e-5), plus half a binary16 ulp for a
    binary16 image."""
    def modify(t, lum):
        return td.modify_log_luminance(t, lum, 1e-4) if log else td.modify_luminance(t, lum)

    def case(src):
        t = gpu(src, dev, rgb_dt)
        l32 = oracle.compute_luminance(npf(t), log, 1e-4)
        lum = gpu(l32 - 0.1 if log else l32 * 0.9, dev, lum_dt)
        return t, lum, oracle.modify_luminance(npf(t), npf(lum), log)

    t, lum, ref = case(scene(48, 64, 22))
    aligned = modify(t, lum)
    offs_rgb = F32_OFFSETS if rgb_dt == torch.float32 else F16_OFFSETS
    offs_lum = F32_OFFSETS if lum_dt == torch.float32 else F16_OFFSETS
    runs = [(o, None) for o in offs_rgb] + [(None, o) for o in offs_lum] + [(offs_rgb[0], offs_lum[-1]), (offs_rgb[-1], offs_lum[0])]
    for ro, lo in runs:
        got = modify(at_offset(t, ro) if ro else t, at_offset(lum, lo) if lo else lum)
        what = f'rgb +{ro} B, plane +{lo} B'
        assert got.dtype == rgb_dt
        assert_close(got, ref, 5e-5, what)
        assert_close(got, npf(aligned), 5e-5, what + ' vs aligned', rounded=True)
    for h, w in ((37, 61), (38, 61), (39, 61)):
        t, lum, ref = case(scene(h, w, h + 2))
        assert_close(modify(t, lum), ref, 5e-5, f'{h}x{w}')


# ------------------------------------------------------------------ tone maps (tonemap.hip: tonemap_tail)
def _tonemap(td, name, t, m, p):
    if name == 'reinhard':
        return td.reinhard_tonemap(t, m, p)
    if name == 'linear':
        return td.linear_tonemap(t, m, p)
    return td.aces_tonemap(t, p) if name == 'aces' else td.aces_tonemap(t, p, m)


@pytest.mark.parametrize('name', ['reinhard', 'aces', 'adaptive_aces', 'linear'])
@pytest.mark.parametrize('vibrance', [0.0, 0.4])
def test_tonemaps_u8_offset_views_and_tails(td, oracle, dev, scene, name, vibrance):
    """tonemap_tail<T, MODE> over the whole image: a different arithmetic from tonemap_vec4 (tdk_pow, roundf + fminf, never the
    LEAN variant), reached by every offset view (the vector path wants 16 B for f32 AND f16 input); and tonemap_vec4 +
    tonemap_tail(first > 0) on aligned images with npix % 4 in {1, 2, 3}.  The assertion of test_tonemaps_u8."""
    p = td.TonemapParameters(0.75, 2.0 if name != 'aces' else 0.5, 1.0 if name != 'adaptive_aces' else 0.6, vibrance)
    img = scene(96, 132, 24) * 1.5
    metrics = oracle.image_metrics([img], 8)
    m = gpu(metrics, dev)
    for dt, off in DT_OFFSETS:
        t = gpu(img, dev, dt)
        ref_u8, ref_f = oracle.tonemap(name, npf(t), metrics, p.gamma, p.intensity, p.light_adapt, p.vibrance, return_float=True)
        got = _tonemap(td, name, at_offset(t, off), m, p)
        assert_u8_ties(got, ref_u8, ref_f, f'{dt} +{off} B')
        d = (got.int() - _tonemap(td, name, t, m, p).int()).abs()
        assert d.max().item() <= 1, f'{dt} +{off} B vs aligned'
    for h, w in ((97, 131), (98, 131), (99, 131)):
        src = scene(h, w, h) * 1.5
        ref_u8, ref_f = oracle.tonemap(name, src, metrics, p.gamma, p.intensity, p.light_adapt, p.vibrance, return_float=True)
        assert_u8_ties(_tonemap(td, name, gpu(src, dev), m, p), ref_u8, ref_f, f'{h}x{w}')


# ------------------------------------------------------------------ normalize_image (color.hip: normalize_vec4 / normalize_tail)
@pytest.mark.parametrize('shape', [(48, 64, 3), (37, 61, 3), (5, 7, 3), (1, 1, 1), (2, 3)])
def test_normalize_image_offset_views(td, dev, shape):
    """normalize_tail<T> over the whole buffer for views 4 / 8 B (f32) and 2 / 4 B (f16) off (the vector path wants four
    elements: 16 B f32, 8 B f16 -- f16 +8 B takes normalize_vec4<__half>), and numel % 4 != 0.  float32: the torch expression
    bit for bit; float16: the fp32 expression on the binary16 values rounded once (test_normalize_image_kernel)."""
    from torch_darktable.pipeline.util import normalize_image

    g = torch.Generator().manual_seed(sum(shape))
    x = (torch.rand(shape, generator=g) * 3 - 0.5).to(dev)
    b = torch.tensor([-0.37, 2.11], device=dev)
    for dt, off in DT_OFFSETS:
        xt = x.to(dt)
        v = at_offset(xt, off)
        ref = (xt.float() - b[0]) / (b[1] - b[0])
        got = normalize_image(v, b)
        assert got.dtype == dt and got.shape == xt.shape
        assert torch.equal(got, ref.to(dt)), f'{dt} +{off} B: {(got != ref.to(dt)).sum().item()} values differ'
        assert torch.equal(got, normalize_image(xt, b))


# ------------------------------------------------------------------ Wiener (wiener.hip)
@pytest.mark.parametrize('C', [1, 3])
def test_wiener_offset_views(td, oracle, dev, scene, C):
    """wiener_finish3<T, 1> (C = 3) / the tile kernels with vec_ok = 0 on a W % 4 == 0 frame whose input view is not aligned:
    test_gpu_parity.py::test_wiener's 2e-5 against the oracle (half a binary16 ulp more for binary16 images), and against the
    aligned call on the same values."""
    h, w = 100, 144
    img = scene(h, w, 26)[:, :, :C].copy()
    sig = np.array([0.05, 0.08, 0.03], np.float32)[:C]
    ws = td.Wiener(dev, (w, h), overlap_factor=4, tile_size=32)
    for dt, off in DT_OFFSETS:
        t = gpu(img, dev, dt)
        ref = oracle.wiener(npf(t), sig, 32, 4)
        got = ws.process(at_offset(t, off), gpu(sig, dev))
        assert got.dtype == dt
        assert_close(got, ref, 2e-5, f'C={C} {dt} +{off} B')
        assert_close(got, npf(ws.process(t, gpu(sig, dev))), 2e-5, f'C={C} {dt} +{off} B vs aligned', rounded=True)


def test_wiener_log_luminance_offset_views(td, oracle, dev, scene):
    """wiener_finish_modify<T, 1> on a W % 4 == 0 frame: an offset image and / or an offset luminance_out (the vector finish wants
    16 B for all three) -- test_wiener_log_luminance_pipeline's 2e-5 against the oracle; luminance_out is
    compute_luminance(result) bit for bit, as process_log_luminance documents."""
    h, w = 96, 128
    img = scene(h, w, 27)
    ws = td.Wiener(dev, (w, h))
    for dt, off in DT_OFFSETS:
        t = gpu(img, dev, dt)
        x32 = npf(t)
        ref = oracle.modify_luminance(x32, oracle.wiener(oracle.compute_luminance(x32, True, 1e-4)[:, :, None], 0.075)[:, :, 0], True)
        aligned = ws.process_log_luminance(t, 0.075)
        for img_off, lum_off in ((off, None), (None, 4 if off != 4 else 8), (off, 8 if off != 8 else 4)):
            src = at_offset(t, img_off) if img_off else t
            lum = at_offset(torch.zeros(h, w, device=dev), lum_off) if lum_off else None
            got = ws.process_log_luminance(src, 0.075, luminance_out=lum)
            what = f'{dt} image +{img_off} B, luminance_out +{lum_off} B'
            assert_close(got, ref, 2e-5, what)
            assert_close(got, npf(aligned), 2e-5, what + ' vs aligned', rounded=True)
            if lum is not None:
                assert torch.equal(lum, td.compute_luminance(got.float())), what  # (the fp32 plane of the stored pixels)


def oracle_lab(oracle, x32):
    """(lightness, (a, b)) of the oracle's Wiener(log-L) result (tests/test_gpu_lab_chain.py::oracle_chain, first stage)."""
    ll = oracle.compute_luminance(x32, True, 1e-4)
    den = oracle.modify_luminance(x32, oracle.wiener(ll[:, :, None], 0.075, 32, 4)[:, :, 0], True)
    return oracle.compute_luminance(den), oracle.color_op('rgb_to_lab', den)[:, :, 1:], den


@pytest.mark.parametrize('with_bounds', [False, True], ids=['plain', 'bounds'])
def test_wiener_lab_offset_views_and_tails(td, oracle, dev, scene, with_bounds):
    """lum_lab_extract<T, 1> (with and without the folded bounds) over the whole image for an offset rgb, wiener_finish_lab<1> for
    offset luminance_out / chroma_out, on a W % 4 == 0 frame; and lum_lab_extract<T, 4> + lum_lab_extract<T, 1>(first > 0) on
    aligned images with npix % 4 in {1, 2, 3}.  Against the oracle as tests/test_gpu_lab_chain.py does: lightness within TOL,
    (a, b) within 2 * TOL."""
    b = torch.tensor([0.03, 1.61], device=dev)
    bn = npy(b)

    for h, w, runs in ((96, 128, DT_OFFSETS), (45, 61, None), (46, 61, None), (47, 61, None)):
        wiener = td.Wiener(dev, (w, h), overlap_factor=4, tile_size=32)
        base = scene(h, w, 5 + h)
        if with_bounds:
            base = base * 1.7 + 0.05
        for dt, off in (runs or [(torch.float32, None), (torch.float16, None)]):
            t = gpu(base, dev, dt)
            x32 = npf(t)
            src32 = (x32 - bn[0]) / (bn[1] - bn[0]) if with_bounds else x32
            lum_ref, ab_ref, _ = oracle_lab(oracle, src32)
            kw = dict(bounds=b) if with_bounds else {}
            cases = [(None, None, None)] if off is None else [(off, None, None), (None, 4, 8), (off, 8, 4)]
            for io, lo, ao in cases:
                lum = at_offset(torch.zeros(h, w, device=dev), lo) if lo else None
                ab = at_offset(torch.zeros(h, w, 2, device=dev), ao) if ao else None
                l, a = wiener.process_log_luminance_lab(at_offset(t, io) if io else t, 0.075, luminance_out=lum, chroma_out=ab, **kw)
                what = f'{h}x{w} {dt} image +{io} B, luminance_out +{lo} B, chroma_out +{ao} B'
                assert lum is None or l is lum
                assert ab is None or a is ab
                d = np.abs(npy(l) - lum_ref).max()
                assert d <= TOL, (what, 'lightness', d)
                d = np.abs(npy(a) - ab_ref).max()
                assert d <= 2 * TOL, (what, 'chroma', d)
                if io or lo or ao:
                    l0, a0 = wiener.process_log_luminance_lab(t, 0.075, **kw)
                    assert (l - l0).abs().max().item() <= TOL and (a - a0).abs().max().item() <= 2 * TOL, what


# ------------------------------------------------------------------ bilateral (bilateral.hip, tdk_bilateral_tile.h)
SIGMAS = [(2.0, 0.2), (8.0, 0.1)]   # the LDS tile kernel / the four-kernel grid path
SIG_IDS = ['tiles', 'grid']


@pytest.mark.parametrize('sig', SIGMAS, ids=SIG_IDS)
def test_bilateral_plane_offset_views(td, oracle, dev, scene, sig):
    """bilateral_tile_kernel<T, T, 0, 1> (vec = false) / splat + slice_kernel<T> on offset planes of a W % 4 == 0 frame: the
    oracle's bits (test_bilateral, test_bilateral_tile_kernel: float32, and binary16 = the fp32 result rounded once)."""
    h, w = 96, 128
    lum = oracle.compute_luminance(scene(h, w, 25))
    bil = td.Bilateral(dev, (w, h), sigma_s=sig[0], sigma_r=sig[1])
    for dt, off in DT_OFFSETS:
        t = gpu(lum, dev, dt)
        ref = oracle.bilateral(npf(t), sig[0], sig[1], 0.4)
        got = bil.process(at_offset(t, off), 0.4)
        assert got.dtype == dt
        want = ref if dt == torch.float32 else ref.astype(np.float16)
        assert np.array_equal(npy(got), want), f'{dt} +{off} B: max |d| {np.abs(npf(got) - ref).max()}'
        assert torch.equal(got, bil.process(t, 0.4))


@pytest.mark.parametrize('sig', SIGMAS, ids=SIG_IDS)
@pytest.mark.parametrize('log', [False, True], ids=['rgb', 'log_rgb'])
def test_bilateral_rgb_offset_views(td, oracle, dev, scene, sig, log):
    """process_rgb / process_log_rgb on offset images, with and without a caller-supplied `luminance` plane that is itself an
    offset view (a plane that is not 16-byte aligned is accepted: vec = false): bilateral_tile_kernel<float, T, 1|2, 1> /
    slice_modify_kernel<T, LOG, 1>.  The same bits as the aligned call (VEC 1 and 4 are both bit-identical to the four-kernel
    path, test_bilateral_tile_kernel_geometry_sweep), and -- with the oracle's bilateral run on the GPU's own lightness plane,
    itself within 2e-5 of the oracle's, as test_bilateral_grid_clamp_whole_frame does -- within modify_luminance's 5e-5."""
    h, w = 96, 128
    img = scene(h, w, 41)
    bil = td.Bilateral(dev, (w, h), sigma_s=sig[0], sigma_r=sig[1])
    eps = 1e-6

    def run(x, lum=None):
        return bil.process_log_rgb(x, 0.4, eps, luminance=lum) if log else bil.process_rgb(x, 0.4, luminance=lum)

    for dt, off in DT_OFFSETS:
        t = gpu(img, dev, dt)
        plane = td.compute_log_luminance(t.float(), eps) if log else td.compute_luminance(t.float())  # fp32 plane of the same values
        x32 = npf(t)
        assert np.abs(npy(plane) - oracle.compute_luminance(x32, log, eps)).max() <= TOL
        ref = oracle.modify_luminance(x32, oracle.bilateral(npy(plane), sig[0], sig[1], 0.4), log)
        aligned = run(t)
        assert_close(aligned, ref, 5e-5, f'{dt} aligned')
        for io, lo in ((off, None), (None, 4), (None, 8), (off, 8 if off != 8 else 4)):
            src = at_offset(t, io) if io else t
            lum = at_offset(plane, lo) if lo else None
            got = run(src, lum)
            what = f'{dt} image +{io} B, luminance +{lo} B'
            assert got.dtype == dt
            assert torch.equal(got, aligned), (what, (got != aligned).sum().item())
            assert_close(got, ref, 5e-5, what)


@pytest.mark.parametrize('sig', SIGMAS, ids=SIG_IDS)
def test_bilateral_lab_offset_views(td, oracle, dev, scene, sig):
    """process_lab with offset lightness and chroma planes of a W % 4 == 0 frame: bilateral_tile_kernel<float, T, 3, 1> (vec =
    false) / slice_lab_kernel<T>.  Against the oracle chain within 2 * TOL (tests/test_gpu_lab_chain.py), against the aligned call
    within 2 * TOL, and the float16 result is the float32 result rounded once (test_lab_chain_tile_kernel_geometry_sweep)."""
    h, w = 128, 160
    rgb = scene(h, w, 6)
    wiener = td.Wiener(dev, (w, h), overlap_factor=4, tile_size=32)
    bil = td.Bilateral(dev, (w, h), sigma_s=sig[0], sigma_r=sig[1])
    lum, ab = wiener.process_log_luminance_lab(gpu(rgb, dev), 0.075)
    _, _, den = oracle_lab(oracle, rgb)
    out_ref = oracle.modify_luminance(den, oracle.bilateral(oracle.compute_luminance(den), sig[0], sig[1], 0.4))
    aligned = bil.process_lab(lum, ab, 0.4)
    for lo, ao in ((4, None), (None, 4), (8, 8), (4, 8)):
        lv = at_offset(lum, lo) if lo else lum
        av = at_offset(ab, ao) if ao else ab
        out = bil.process_lab(lv, av, 0.4)
        out16 = bil.process_lab(lv, av, 0.4, out_dtype=torch.float16)
        what = f'luminance +{lo} B, chroma +{ao} B'
        d = np.abs(npy(out) - out_ref).max()
        assert d <= 2 * TOL, (what, 'oracle', d)
        assert (out - aligned).abs().max().item() <= 2 * TOL, what
        assert torch.equal(out16, out.half()), (what, (out16 != out.half()).sum().item())


# ------------------------------------------------------------------ demosaic, post-processing, Laplacian on offset inputs
@pytest.mark.parametrize('pattern', PATTERNS)
def test_rcd_offset_bayer(td, oracle, dev, scene, pattern):
    """An odd-element offset of the mosaic turns RCD's wide_ok off: the tile kernel (rcd_interior<TI, T>) runs on a frame that
    would take the column strips; an even-element offset keeps the strips with pair loads from an 8-B (f32) / 4-B (f16) view.
    float32: the oracle's bits; float16 (the tile kernel rounds the exact fp32 result once; the strips use the approximate
    flavour): within test_rcd_fp16_fast_arithmetic's bounds, and the odd offset equals the aligned tile kernel bit for bit."""
    from test_gpu_parity import assert_f16_close
    from torch_darktable import torch_darktable_extension as ext

    h, w = 130, 258
    bayer = oracle.mosaic(scene(h, w, 13), oracle.PATTERNS[pattern])
    ref = oracle.rcd(bayer, oracle.PATTERNS[pattern])
    ws = td.RCD(dev, (w, h), td.BayerPattern[pattern])
    t = gpu(bayer, dev)
    for off in F32_OFFSETS:
        got = npy(ws.process(at_offset(t, off)))
        bad = np.argwhere(got != ref)
        assert bad.size == 0, f'f32 +{off} B: {len(bad)} mismatches, first at {bad[:5].tolist()}'
    t16 = t.half()
    ref16 = oracle.rcd(npf(t16), oracle.PATTERNS[pattern])
    with ext.verification_paths(rcd_tiles=True):
        tiles16 = ws.process(t16)
    for off in F16_OFFSETS:
        got = ws.process(at_offset(t16, off))
        assert_f16_close(npy(got), ref16, f'f16 +{off} B')
        if (off // 2) % 2:
            assert torch.equal(got, tiles16), f'f16 +{off} B: the tile kernel on a view differs from the aligned tile kernel'


@pytest.mark.parametrize('pattern', PATTERNS)
def test_ppg_bilinear_offset_bayer(td, oracle, dev, scene, pattern):
    """PPG and bilinear 5x5 read the mosaic with scalar loads whatever its alignment (their vector path is on the output, which
    the wrappers allocate): offset mosaics give the oracle's bits."""
    h, w = 64, 96
    bayer = oracle.mosaic(scene(h, w, 12), oracle.PATTERNS[pattern])
    t = gpu(bayer, dev)
    ref_ppg = oracle.ppg(bayer, oracle.PATTERNS[pattern], 1.5)
    ref_bil = oracle.bilinear5x5(bayer, oracle.PATTERNS[pattern])
    ws = td.PPG(dev, (w, h), td.BayerPattern[pattern], median_threshold=1.5)
    for off in F32_OFFSETS:
        v = at_offset(t, off)
        assert np.array_equal(npy(ws.process(v)), ref_ppg), off
        assert np.array_equal(npy(td.bilinear5x5_demosaic(v, td.BayerPattern[pattern])), ref_bil), off


@pytest.mark.parametrize('cfg', [dict(color_smoothing_passes=3, green_eq_local=True), dict(color_smoothing_passes=4), dict(green_eq_local=True, green_eq_threshold=4.0)])
def test_postprocess_offset_views(td, oracle, dev, scene, cfg):
    """PostProcess with vec_in = false (aligned4(): 16 B f32, 8 B f16) on a W % 4 == 0 frame: float32 the oracle's bits and the
    aligned call's; float16 the float32 result on the same values rounded once (test_postprocess_fp16_storage_rounded_once)."""
    h, w = 96, 128
    rgb = oracle.rcd(oracle.mosaic(scene(h, w, 31), oracle.RGGB), oracle.RGGB)
    rgb[5:9, 7:30] -= 0.3
    ws = td.PostProcess(dev, (w, h), td.BayerPattern.RGGB, **cfg)
    ref = oracle.postprocess(rgb, oracle.RGGB, **cfg)
    for dt, off in DT_OFFSETS:
        t = gpu(rgb, dev, dt)
        got = ws.process(at_offset(t, off))
        if dt == torch.float32:
            assert np.array_equal(npy(got), ref), f'+{off} B'
        else:
            got32 = ws.process(t.float())
            assert torch.equal(got, got32.half()), f'f16 +{off} B'
        assert torch.equal(got, ws.process(t)), f'{dt} +{off} B vs aligned'


def test_laplacian_offset_views(td, oracle, dev, scene):
    """Laplacian on offset planes (float32 and binary16 input): without the clarity term the oracle's bits
    (test_gpu_parity.py::test_laplacian), and the aligned call's."""
    h, w = 120, 160
    lum = oracle.compute_luminance(scene(h, w, 28))
    prm = (0.2, 1.6, 0.7, 0.0)
    ws = td.Laplacian(dev, (w, h), td.LaplacianParams(6, *prm))
    for dt, off in DT_OFFSETS:
        t = gpu(lum, dev, dt)
        got = ws.process(at_offset(t, off))
        assert np.array_equal(npf(got), oracle.laplacian(npf(t), *prm)), f'{dt} +{off} B'
        assert torch.equal(got, ws.process(t)), f'{dt} +{off} B vs aligned'


def test_codec_encode_offset_views(td, oracle, dev):
    """encode12 of an input view that is not 16-byte aligned takes the per-pair kernel: the oracle's bits."""
    rng = np.random.default_rng(6)
    n = 4 * 1001 + 2
    f32 = rng.uniform(-0.1, 1.2, n).astype(np.float32)
    u16 = rng.integers(0, 5000, n, dtype=np.uint16)
    for off in F32_OFFSETS:
        assert np.array_equal(npy(td.encode12_float(at_offset(gpu(f32, dev), off))), oracle.encode12_f32(f32, False, True)), off
    for off in (2, 4, 8):
        assert np.array_equal(npy(td.encode12_u16(at_offset(gpu(u16, dev), off))), oracle.encode12_u16(u16, False)), off


@pytest.mark.parametrize('pattern', ['RGGB', 'GBRG'])
def test_rcd_packed12_offset_views(td, oracle, dev, scene, pattern):
    """RCD.process_packed on a packed buffer that is not 4-byte aligned: tdk_decode12_wb_plane takes decode12_wb_pairs for the
    whole frame.  The documented contract: decode12 -> apply_white_balance -> process bit for bit -- the oracle's bits and the
    aligned call's."""
    h, w = 130, 258
    bayer = np.clip(oracle.mosaic(scene(h, w, 33), oracle.PATTERNS[pattern])[:, :, 0], 0, 1)
    packed = oracle.encode12_f32(bayer.ravel(), False, True)
    gains = np.array([1.5, 1.0, 1.2], np.float32)
    b = oracle.apply_white_balance(oracle.decode12_f32(packed, False, True).reshape(h, w), gains, oracle.PATTERNS[pattern])
    ref = oracle.rcd(np.ascontiguousarray(b[:, :, None]), oracle.PATTERNS[pattern])
    rcd = td.RCD(dev, (w, h), td.BayerPattern[pattern])
    t, g = gpu(packed, dev), gpu(gains, dev)
    aligned = rcd.process_packed(t, g)
    assert np.array_equal(npy(aligned), ref)
    for off in (1, 2, 3):
        got = rcd.process_packed(at_offset(t, off), g)
        assert torch.equal(got, aligned), (off, (got != aligned).sum().item())


# ------------------------------------------------------------------ grid-stride loops past 65536 x 256 pixels
def test_grid_stride_loops_at_50mp(td, oracle, dev):
    """stream_grid caps the one-pixel-per-thread kernels at 65536 workgroups of 256 threads = 16 777 216 pixels: an offset
    8192 x 6144 view (50 331 648 pixels, no vector path) runs color_tail, lum_extract_tail and tonemap_tail through three loop
    iterations.  The ops are per pixel, so the oracle runs on row bands holding pixel 0, pixels 16 777 216 +- 256 and
    33 554 432 +- 256 (the starts of the 2nd and 3rd iterations) and the last row."""
    from torch_darktable.synthetic import synthetic_rgb

    W, H = 8192, 6144
    x = at_offset(synthetic_rgb(H, W, seed=91, device=dev), 4)
    bands = [(0, 2), (2047, 2049), (4095, 4097), (H - 1, H)]
    for first in (16_777_216, 33_554_432):
        assert any(y0 * W <= first - 256 and first + 256 <= y1 * W for y0, y1 in bands)
    m = td.compute_image_metrics([x], 8)
    p = td.TonemapParameters(0.75, 2.0, 1.0, 0.0)
    u8 = td.reinhard_tonemap(x, m, p)
    ll = td.compute_log_luminance(x, 1e-4)
    lab = td.rgb_to_lab(x)
    for y0, y1 in bands:
        src = npy(x[y0:y1])
        ref_u8, ref_f = oracle.tonemap('reinhard', src, npy(m), p.gamma, p.intensity, p.light_adapt, p.vibrance, return_float=True)
        assert_u8_ties(u8[y0:y1], ref_u8, ref_f, f'rows {y0}:{y1}')
        assert np.abs(npy(ll[y0:y1]) - oracle.compute_luminance(src, True, 1e-4)).max() <= TOL, (y0, y1)
        assert np.abs(npy(lab[y0:y1]) - oracle.color_op('rgb_to_lab', src)).max() <= TOL, (y0, y1)


# ------------------------------------------------------------------ the pipeline on frames of a batch
@pytest.fixture(scope='module')
def batch(dev):
    """(3, 3041, 4098, 3) float32: frame 1 starts 8 B (mod 16) into the allocation, frame 2 16 B (float16: 12 and 8 B)."""
    from torch_darktable.synthetic import synthetic_rgb

    h, w = 3041, 4098
    frames = [synthetic_rgb(h, w, seed=70 + i, device=dev) * 1.7 + 0.05 for i in range(3)]
    return torch.stack(frames)


def test_normalize_image_on_batch_frames(dev, batch):
    """normalize_image(batch[i], bounds): the frames of a 4098 x 3041 batch are not 16-byte aligned -- the kernel used to reject
    them.  The torch expression bit for bit (float16: the fp32 expression rounded once)."""
    from torch_darktable.pipeline.util import normalize_image

    b = torch.tensor([0.03, 1.61], device=dev)
    for dt in (torch.float32, torch.float16):
        x = batch.to(dt)
        for i in (1, 2):
            assert x[i].data_ptr() % 16 == (i * x[0].numel() * x.element_size()) % 16
            ref = ((x[i].float() - b[0]) / (b[1] - b[0])).to(dt)
            assert torch.equal(normalize_image(x[i], b), ref), (dt, i)


@pytest.mark.parametrize('stages', ['denoise', 'bilateral', 'both'])
def test_image_processor_on_batch_frames(td, dev, batch, stages):
    """ImageProcessor.process_rgb(frame, bounds) -> tonemap on frames 1 and 2 of a (3, 3041, 4098, 3) batch, float32 and
    float16, against the same frames .clone()d (aligned), with test_gpu_bench_chain.py's tolerances: float32 within 2 * TOL and
    1 LSB; float16 within 2e-3 * max(|ref|, 0.05) per value and 2 LSB, at most 1e-5 of the values above 1 LSB."""
    from torch_darktable.pipeline import ImageProcessor
    from torch_darktable.pipeline.config import ImageProcessingSettings

    h, w = batch.shape[1:3]
    settings = ImageProcessingSettings(enable_denoise=stages != 'bilateral', enable_bilateral=stages != 'denoise')
    proc = ImageProcessor((w, h), td.BayerPattern.RGGB, td.PackedFormat.Packed12, settings, dev, None)
    b = torch.tensor([0.03, 1.61], device=dev)
    for dt in (torch.float32, torch.float16):
        x = batch.to(dt)
        for i in (1, 2):
            frame = x[i]
            ref = proc.process_rgb(frame.clone(), b)
            got = proc.process_rgb(frame, b)
            m = td.compute_image_metrics([ref], 8)
            ref_u8, got_u8 = proc.tonemap(ref, m), proc.tonemap(got, m)
            what = f'{stages} {dt} frame {i} (+{frame.data_ptr() % 16} B)'
            assert got.dtype == dt and got.shape == frame.shape
            d = (got.float() - ref.float()).abs()
            du8 = (got_u8.int() - ref_u8.int()).abs()
            if dt == torch.float32:
                assert d.max().item() <= 2 * TOL, (what, d.max().item())
                assert du8.max().item() <= 1, (what, du8.max().item())
            else:
                rel = (d / ref.float().abs().clamp_min(0.05)).max().item()
                assert rel < 2e-3, (what, rel)
                assert du8.max().item() <= 2 and (du8 > 1).float().mean().item() <= 1e-5, (what, du8.max().item())
