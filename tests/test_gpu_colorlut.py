"""GPU: the colour transform (torch_darktable.ColorLUT, include/tdk_hip_lut.h) against the NumPy float32 restatement of its
specification, tests/colorlut_spec.py (held to float64 evaluations in tests/test_colorlut_spec.py).

The kernel's output must have the restatement's exact bits: every comparison is on the raw bits, and there is no tolerance anywhere in
this file.  The one thing left open is the payload of a NaN that reaches a float output (no table behind it), which the header does
not specify: there both sides must be NaN.  Shapes are the smallest that reach the paths: less than one 16-pixel group per lane,
heads and tails, offset views, and one frame large enough for the persistent workgroups to go round their loop."""
import ctypes

import numpy as np
import pytest
import torch

import colorlut_spec as spec

pytestmark = pytest.mark.gpu

F = np.float32
BITS = {np.dtype(np.float32): np.int32, np.dtype(np.float16): np.int16, np.dtype(np.uint8): np.uint8}
DTYPES = [np.float32, np.float16, np.uint8]
TORCH = {np.float32: torch.float32, np.float16: torch.float16, np.uint8: torch.uint8}
TAG = {torch.float32: 0, torch.float16: 1, torch.uint8: 2}
SHAPES = [(5, 7, 3), (33, 61, 3), (64, 128, 3)]      # less than one group per lane; tails; whole groups on an aligned buffer

MATRIX = np.array([[0.9, 0.15, -0.05], [0.02, 0.8, 0.18], [-0.1, 0.25, 0.85]], F)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a visible MI355X'
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def tables():
    """The random tables, made once: {('lut', N): (N, N, N, 3)}, {('shaper', S, tables): (S,) or (3, S)}."""
    rng = np.random.default_rng(2024)
    out = {}
    for n in (2, 3, 17, 18, 33, 65):
        axis = np.arange(n, dtype=np.float64) / (n - 1)
        b, g, r = np.meshgrid(axis, axis, axis, indexing='ij')
        out['lut', n] = (np.stack((r, g, b), axis=-1) ** 0.8 + 0.15 * rng.standard_normal((n, n, n, 3))).astype(F)   # a look plus colour in every node
    for s in (2, 5, 1024):
        out['shaper', s, 1] = (np.linspace(0, 1, s) ** 0.45).astype(F)
        out['shaper', s, 3] = np.stack([np.linspace(0, 1, s) ** p for p in (0.45, 0.5, 0.6)]).astype(F)
    return out


def build(td, dev, tables, matrix=False, shaper=None, lut=None, interpolation='tetrahedral', global_nodes=False):
    """shaper: (S, tables) or None; lut: N or None.  Domains off [0, 1] so that lo and scale are not trivial."""
    obj = td.ColorLUT(dev, matrix=MATRIX if matrix else None, shaper=None if shaper is None else tables['shaper', shaper[0], shaper[1]],
                      shaper_domain=(-0.125, 1.25), lut=None if lut is None else tables['lut', lut], lut_domain=((0, 0, -0.05), (1, 1.0625, 1)),
                      interpolation=interpolation)
    obj.global_nodes = global_nodes
    return obj


def frame(dtype, shape, seed, n=17):
    """Random frame with the seeded cases in front and scattered: node hits (coordinates j / (n - 1)), greys, pixels with two and
    three equal channels (fraction ties), values outside every domain, negatives, and for the float types NaN and both infinities."""
    rng = np.random.default_rng(seed)
    pixels = int(np.prod(shape[:-1]))
    if dtype == np.uint8:
        x = rng.integers(0, 256, (pixels, 3), dtype=np.uint8)
        k = max(pixels // 5, 1)
        x[:k, 1] = x[:k, 0]                                  # r == g
        x[k // 2:k, 2] = x[k // 2:k, 1]                      # ... and grey
        x[-1] = (0, 255, 0)
        return x.reshape(shape)
    x = (rng.random((pixels, 3)) * 1.3 - 0.15).astype(F)
    k = max(pixels // 6, 1)
    x[:k] = rng.integers(0, n, (k, 3)).astype(F) / F(n - 1)   # node hits
    x[k:2 * k, 1] = x[k:2 * k, 0]                             # r == g
    x[k + k // 2:2 * k, 2] = x[k + k // 2:2 * k, 1]           # grey
    x[2 * k:2 * k + k // 2, 2] = x[2 * k:2 * k + k // 2, 1]   # g == b
    special = np.array([np.nan, np.inf, -np.inf, 2.5, -3.0, -0.0, 1e-42, 65504.0, 1.0, 0.0], F)
    m = min(len(special) * 3, pixels)
    x[pixels - m:] = np.stack([np.resize(np.roll(special, shift), m) for shift in (0, 3, 7)], axis=-1)
    return x.astype(dtype).reshape(shape)


def same_bits(got, want):
    """got: CUDA or CPU tensor, want: NumPy array of the same dtype and shape.  A NaN must meet a NaN; everything else its bits."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    view = BITS[want.dtype]
    equal = got.view(view) == np.ascontiguousarray(want).view(view)
    if want.dtype != np.uint8:
        equal |= np.isnan(got) & np.isnan(want)
    return bool(equal.all())


def report(got, want, what):
    got = got.cpu().numpy()
    view = BITS[want.dtype]
    bad = np.argwhere((got.view(view) != want.view(view)) & ~((got != got) & (want != want)) if want.dtype != np.uint8 else got != want)
    print(f'{what}: {len(bad)} of {want.size} values differ, first at {bad[0]}: got {got[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r}')


def at_offset(t, elements):
    """A contiguous copy of CUDA tensor `t` that starts `elements` elements past an aligned allocation."""
    pool = torch.zeros(t.numel() + elements + 64, dtype=t.dtype, device=t.device)
    assert pool.data_ptr() % 256 == 0
    v = pool[elements:elements + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() == pool.data_ptr() + elements * t.element_size()
    return v


def check(obj, dev, x, out_dtype=None, offset=0, what=''):
    out_dtype = x.dtype.type if out_dtype is None else out_dtype
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    if offset:
        t = at_offset(t, offset)
    out = obj.process(t, TORCH[out_dtype])
    assert tuple(out.shape) == x.shape and out.is_contiguous() and out.dtype == TORCH[out_dtype] and out.data_ptr() != t.data_ptr()
    want = spec.of(obj, x, out_dtype)
    ok = same_bits(out, want)
    if not ok:
        report(out, want, f'{what}{x.shape} {x.dtype}->{np.dtype(out_dtype)} {obj}')
    assert ok, (what, x.shape, x.dtype, out_dtype, repr(obj), offset)
    return out


def call_c(obj, src, dst, flags=None):
    """tdk_color_lut on the tensors' own pointers (process allocates an aligned result; this reaches any destination alignment)."""
    from torch_darktable._native import lib

    shaper, lut = obj._upload(src.device)
    rc = lib.tdk_color_lut(src.data_ptr(), TAG[src.dtype], dst.data_ptr(), TAG[dst.dtype], src.numel() // 3,
                           obj._c_matrix, 0 if shaper is None else shaper.data_ptr(), obj.shaper_size, obj.shaper_tables, obj.shaper_lo, obj.shaper_scale,
                           0 if lut is None else lut.data_ptr(), obj.lut_size, obj._c_lut_lo, obj._c_lut_scale, {'tetrahedral': 0, 'trilinear': 1}[obj.interpolation],
                           obj._flags() if flags is None else flags, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.tdk_last_error()


# ------------------------------------------------------------------ 1. shapes, heads and tails, offset views
@pytest.mark.parametrize('dtype', DTYPES)
def test_small_frames_tails_and_whole_groups(td, dev, tables, dtype):
    full = build(td, dev, tables, matrix=True, shaper=(5, 3), lut=17)
    for shape in SHAPES + [(1, 1, 3), (1, 16, 3), (3,), (2, 3, 5, 3)]:
        check(full, dev, frame(dtype, shape, sum(shape)), what='shape ')


@pytest.mark.parametrize('src_dtype', DTYPES)
@pytest.mark.parametrize('dst_dtype', DTYPES)
def test_offset_source_and_destination_views(td, dev, tables, src_dtype, dst_dtype):
    """Source and destination up to a few elements past an aligned buffer, every mix: the head that aligns one side does or does not
    align the other (vector or per-element accesses on either side).  Nothing is written outside the destination."""
    obj = build(td, dev, tables, matrix=True, shaper=(5, 1), lut=3)
    x = frame(src_dtype, (33, 61, 3), 77, n=3)
    want = spec.of(obj, x, dst_dtype)
    for src_off, dst_off in ((1, 0), (0, 1), (1, 1), (3, 2), (5, 16), (4, 7)):
        t = at_offset(torch.from_numpy(x).to(dev), src_off) if src_off else torch.from_numpy(x).to(dev)
        pool = torch.zeros(x.size + dst_off + 64, dtype=TORCH[dst_dtype], device=dev)
        out = pool[dst_off:dst_off + x.size]
        call_c(obj, t, out)
        torch.cuda.synchronize()
        ok = same_bits(out.view(x.shape), want)
        if not ok:
            report(out.view(x.shape), want, f'offsets {src_off}, {dst_off}')
        assert ok, (src_off, dst_off)
        assert float(pool[:dst_off].float().abs().sum()) == 0 and float(pool[dst_off + x.size:].float().abs().sum()) == 0
        if src_off and not dst_off:
            check(obj, dev, x, dst_dtype, offset=src_off, what=f'source offset {src_off} ')


# ------------------------------------------------------------------ 2. the 3D LUT: sizes, both interpolations, both ways to read the nodes
@pytest.mark.parametrize('interpolation', ['tetrahedral', 'trilinear'])
@pytest.mark.parametrize('n', [2, 3, 17, 18, 33, 65])
def test_lut_sizes(td, dev, tables, n, interpolation):
    obj = build(td, dev, tables, lut=n, interpolation=interpolation)
    assert (obj.lds_bytes() > 0) == (n <= 18)                    # 18 is the largest size that is staged (alone: 69 984 bytes)
    x = frame(np.float32, (64, 128, 3), 100 + n, n=n)
    out = check(obj, dev, x, what=f'N = {n} ')
    if n <= 18:
        obj.global_nodes = True
        assert obj.lds_bytes() == 0
        again = check(obj, dev, x, what=f'N = {n} global ')
        assert torch.equal(out.view(torch.int32), again.view(torch.int32))
    if n == 18:                                                  # beside the largest shaper its nodes no longer fit the budget
        both = build(td, dev, tables, shaper=(1024, 3), lut=18, interpolation=interpolation)
        assert both.lds_bytes() == 12288
        check(both, dev, x, what='N = 18 + shaper ')


@pytest.mark.parametrize('interpolation', ['tetrahedral', 'trilinear'])
def test_n17_staged_and_global_give_the_same_bits(td, dev, tables, interpolation):
    x = {d: frame(d, (33, 61, 3), 170) for d in DTYPES}
    for shaper in (None, (1024, 3)):                             # 58 956 bytes, and 71 244 with the largest shaper: above 64 KB
        staged = build(td, dev, tables, matrix=True, shaper=shaper, lut=17, interpolation=interpolation)
        direct = build(td, dev, tables, matrix=True, shaper=shaper, lut=17, interpolation=interpolation, global_nodes=True)
        assert staged.lds_bytes() == 58956 + (12288 if shaper else 0) and direct.lds_bytes() == (12288 if shaper else 0)
        for d in DTYPES:
            a, b = check(staged, dev, x[d], what='staged '), check(direct, dev, x[d], what='global ')
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_node_hits_return_the_nodes_bits(td, dev, tables):
    n = 17
    lut = tables['lut', n]
    obj = td.ColorLUT(dev, lut=lut, lut_domain=((0, 0, 0), (n - 1, n - 1, n - 1)))
    assert obj.lut_scale == (1.0, 1.0, 1.0)
    idx = np.random.default_rng(5).integers(0, n - 1, (2000, 3))           # (b, g, r), below the last node: f = 0
    x = idx[:, ::-1].astype(F)
    for interpolation in ('tetrahedral', 'trilinear'):
        obj.interpolation = interpolation
        out = check(obj, dev, x, what='node hits ')
        assert same_bits(out, lut[idx[:, 0], idx[:, 1], idx[:, 2]])


def test_grey_stays_grey_through_an_identity_lut(td, dev):
    grey = np.repeat(np.random.default_rng(6).random((4000, 1)).astype(F), 3, axis=1)
    for n in (2, 17, 33):
        out = check(td.ColorLUT.identity(dev, n), dev, grey, what='grey ').cpu().numpy()
        assert np.array_equal(out[:, 0].view(np.int32), out[:, 1].view(np.int32)) and np.array_equal(out[:, 1].view(np.int32), out[:, 2].view(np.int32))


# ------------------------------------------------------------------ 3. the shaper
@pytest.mark.parametrize('count', [1, 3])
@pytest.mark.parametrize('s', [2, 5, 1024])
def test_shaper_sizes(td, dev, tables, s, count):
    obj = build(td, dev, tables, shaper=(s, count))
    assert obj.lds_bytes() == 4 * s * count
    for dtype in (np.float32, np.float16):
        check(obj, dev, frame(dtype, (33, 61, 3), s + count), what=f'S = {s} x {count} ')


# ------------------------------------------------------------------ 4. stages and storage types
@pytest.mark.parametrize('dtype', DTYPES)
def test_every_stage_combination(td, dev, tables, dtype):
    x = frame(dtype, (33, 61, 3), 40)
    for matrix in (False, True):
        for shaper in (None, (5, 1), (1024, 3)):
            for lut in (None, 17, 33):
                for interpolation in (('tetrahedral', 'trilinear') if lut else ('tetrahedral',)):
                    check(build(td, dev, tables, matrix=matrix, shaper=shaper, lut=lut, interpolation=interpolation), dev, x, what='stages ')


@pytest.mark.parametrize('src_dtype', DTYPES)
@pytest.mark.parametrize('dst_dtype', DTYPES)
def test_all_nine_dtype_pairs(td, dev, tables, src_dtype, dst_dtype):
    x = frame(src_dtype, (33, 61, 3), 50)
    for obj in (build(td, dev, tables, matrix=True, shaper=(5, 3), lut=17), build(td, dev, tables, matrix=True), build(td, dev, tables, lut=33, interpolation='trilinear')):
        check(obj, dev, x, dst_dtype, what='dtype pair ')


@pytest.mark.parametrize('dtype', DTYPES)
def test_no_stage_returns_the_inputs_bits(td, dev, dtype):
    empty = td.ColorLUT(dev)
    x = frame(dtype, (33, 61, 3), 60)
    if dtype == np.uint8:
        codes = np.arange(256, dtype=np.uint8)
        x = np.stack((codes, codes[::-1], np.roll(codes, 7)), axis=-1)
    out = check(empty, dev, x, what='no stage ')
    assert same_bits(out, x)


def test_uint8_lattice_and_all_greys(td, dev, tables):
    """uint8 -> uint8 over a 64^3 sub-lattice of the codes (both ends included) and the 256 greys: 262 400 pixels, graded by a staged
    and by a gathered LUT, and passed through with no stage."""
    codes = np.rint(np.linspace(0, 255, 64)).astype(np.uint8)
    b, g, r = np.meshgrid(codes, codes, codes, indexing='ij')
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    x = np.concatenate((np.stack((r, g, b), axis=-1).reshape(-1, 3), grey))
    assert x.shape == (64 ** 3 + 256, 3)
    assert same_bits(check(td.ColorLUT(dev), dev, x, what='lattice identity '), x)
    check(build(td, dev, tables, lut=17), dev, x, what='lattice N = 17 ')
    check(build(td, dev, tables, shaper=(1024, 3), lut=33, interpolation='trilinear'), dev, x, what='lattice N = 33 ')
    out = check(td.ColorLUT.identity(dev, 17), dev, x, what='lattice identity LUT ')
    assert np.abs(out.cpu().numpy().astype(int) - x).max() <= 1 and same_bits(out[-256:], grey)


# ------------------------------------------------------------------ 5. persistent workgroups
def test_a_frame_the_persistent_workgroups_loop_over(td, dev, tables):
    """The grid is at most two workgroups per compute unit, 512 lanes each, 16 pixels per lane and step: one sweep of the grid covers
    2 * 256 * 512 * 16 = 4.19 M pixels on the MI355X, so a (1024, 1536, 3) frame (1.57 M) does not loop.  The smallest frame of
    4096-pixel rows that makes a good part of the workgroups go round twice is used instead, odd in its last row so the tail is there
    too.  The operator is pointwise, so the expected frame is the restatement of 65 536 distinct pixels gathered by the same index
    map that builds the input: every position is compared, and the reference costs milliseconds."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    sweep = 2 * cus * 512 * td.ColorLUT.GROUP
    pixels = sweep + sweep // 8 + 5
    rng = np.random.default_rng(8)
    index = rng.integers(0, 65536, pixels)
    for dtype, out_dtype in ((np.uint8, np.uint8), (np.float16, np.float16)):
        base = frame(dtype, (65536, 3), 80)
        x = torch.from_numpy(base).to(dev)[torch.from_numpy(index).to(dev)].contiguous()
        assert tuple(x.shape) == (pixels, 3)
        for obj in (build(td, dev, tables, matrix=True, shaper=(1024, 3), lut=17), build(td, dev, tables, lut=17, global_nodes=True),
                    build(td, dev, tables, lut=33, interpolation='trilinear')):
            want = spec.of(obj, base, out_dtype)[index]
            out = obj.process(x, TORCH[out_dtype])
            ok = same_bits(out, want)
            if not ok:
                report(out, want, f'loop {obj}')
            assert ok, (dtype, repr(obj))


# ------------------------------------------------------------------ 6. reproducibility, graph capture, streams
@pytest.mark.parametrize('shaper', [(5, 1), (1024, 3)], ids=['below-64KB', 'above-64KB'])
def test_graph_capture_as_the_objects_first_call(td, dev, tables, shaper):
    """An object no call has used yet, captured on a side stream without a warm-up, replayed twice; the second replay sees new
    contents in the input buffer.  The larger configuration (71 244 bytes of LDS) raises its kernel's dynamic-LDS limit inside the
    capture: a host-side attribute, not a stream operation."""
    rng = np.random.default_rng(90)
    lut = (tables['lut', 17] + 0.01 * rng.standard_normal((17, 17, 17, 3))).astype(F)
    obj = td.ColorLUT(dev, matrix=MATRIX * F(1.01), shaper=tables['shaper', shaper[0], shaper[1]], lut=lut, interpolation='trilinear' if shaper[1] == 3 else 'tetrahedral')
    a, b = frame(np.uint8, (131, 173, 3), 91), frame(np.uint8, (131, 173, 3), 92)
    x = torch.from_numpy(a).to(dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            captured = obj.process(x, torch.float16)
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(captured, spec.of(obj, a, np.float16))
    x.copy_(torch.from_numpy(b).to(dev))
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(captured, spec.of(obj, b, np.float16)) and same_bits(obj.process(x, torch.float16), spec.of(obj, b, np.float16))


def test_one_object_on_two_streams_and_two_runs_are_identical(td, dev, tables):
    obj = build(td, dev, tables, matrix=True, shaper=(1024, 3), lut=17)
    a, b = frame(np.float16, (301, 403, 3), 93), frame(np.uint8, (301, 403, 3), 94)
    xa, xb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    for s in (s1, s2):
        s.wait_stream(torch.cuda.current_stream())
    outs = []
    for _ in range(3):
        with torch.cuda.stream(s1):
            oa = obj.process(xa)
        with torch.cuda.stream(s2):
            ob = obj.process(xb, torch.float32)
        outs.append((oa, ob))
    s1.synchronize()
    s2.synchronize()
    want_a, want_b = spec.of(obj, a), spec.of(obj, b, np.float32)
    for oa, ob in outs:
        assert same_bits(oa, want_a) and same_bits(ob, want_b)


def test_front_end_errors_that_need_a_device(td, dev):
    from torch_darktable._native import lib

    obj = td.ColorLUT.identity(dev, 2)
    with pytest.raises(RuntimeError, match='contiguous'):
        obj.process(torch.zeros(48, 128, 3, device=dev)[:, ::2])
    with pytest.raises(RuntimeError, match='float32, float16 or uint8'):
        obj.process(torch.zeros(48, 64, 3, device=dev, dtype=torch.int32))
    assert tuple(obj.process(torch.zeros(0, 3, device=dev)).shape) == (0, 3)
    x = torch.zeros(48, 64, 3, device=dev)
    three = (ctypes.c_float * 3)(0, 0, 0)
    rc = lib.tdk_color_lut(x.data_ptr(), 0, x.data_ptr(), 0, x.numel() // 3, None, None, 0, 1, 0.0, 0.0, None, 0, three, three, 0, 0, None)
    assert rc == 1 and b'overlap' in lib.tdk_last_error()


# ------------------------------------------------------------------ 7. pipeline
def _processor(td, dev, w, h, transforms=None, storage_dtype=torch.float32, **kw):
    from torch_darktable.pipeline import ImageProcessingSettings, ImageProcessor, ImageTransform, ToneMapper
    settings = ImageProcessingSettings(moving_average=0.3, postprocess=False, enable_denoise=True, enable_bilateral=True, tone_mapping=ToneMapper.reinhard, resize_width=100)
    return ImageProcessor((w, h), td.BayerPattern.RGGB, td.PackedFormat.Packed12, settings, dev, (1.4, 1.0, 1.3), transforms=transforms or ImageTransform.none,
                          storage_dtype=storage_dtype, **kw)


def _packed(td, dev, w, h, seed):
    from torch_darktable.synthetic import synthetic_bayer
    return td.encode12_float(synthetic_bayer(h, w, seed=seed, device='cpu').to(dev).reshape(-1))


def test_pipeline_look_grades_the_tone_mapped_frame_before_the_orientation(td, dev, tables):
    from torch_darktable.pipeline import ImageTransform
    from torch_darktable.pipeline.transform import transform
    w, h = 256, 192
    packed = _packed(td, dev, w, h, 201)
    look = build(td, dev, tables, shaper=(1024, 3), lut=17)
    plain = _processor(td, dev, w, h).process(packed, 'cam')
    assert plain.dtype == torch.uint8 and tuple(plain.shape) == (h, w, 3)
    out = _processor(td, dev, w, h, look=look).process(packed, 'cam')
    assert torch.equal(out, look.process(plain)) and not torch.equal(out, plain)
    assert same_bits(out, spec.of(look, plain.cpu().numpy()))
    turned = _processor(td, dev, w, h, ImageTransform.rotate_90, look=look).process(packed, 'cam')
    assert torch.equal(turned, transform(out, ImageTransform.rotate_90))
    # in front of the scaler: the resized result is the scaler applied to the graded frame
    small = _processor(td, dev, w, h, look=look).process_resized(packed, 'cam')
    assert torch.equal(small, td.Resize(dev, (w, h), (100, 75)).process(out))


@pytest.mark.parametrize('storage', [torch.float32, torch.float16])
def test_pipeline_color_transforms_the_demosaiced_frame(td, dev, storage):
    """ImageProcessor(color=c) against the stages called one by one, the colour transform between load_image and the bounds."""
    from torch_darktable import tonemap
    from torch_darktable.pipeline.util import lerp
    w, h = 256, 192
    packed = _packed(td, dev, w, h, 202)
    color = td.ColorLUT(dev, matrix=[[1.6, -0.4, -0.2], [-0.3, 1.5, -0.2], [0.0, -0.5, 1.5]], shaper=np.linspace(0, 1, 64) ** 0.9, shaper_domain=(0.0, 1.5))
    out = _processor(td, dev, w, h, storage_dtype=storage, color=color).process(packed, 'cam')
    c = _processor(td, dev, w, h, storage_dtype=storage)
    raw = c.load_image(packed)
    assert raw.dtype == storage
    rgb = [color.process(raw)]
    assert rgb[0].dtype == storage and same_bits(rgb[0], spec.of(color, raw.cpu().numpy()))
    bounds = tonemap.compute_image_bounds(rgb, stride=8)
    acc = tonemap.MetricsAccumulator(dev, stride=8)
    rgb = [c.process_rgb(rgb[0], lerp(bounds, bounds, 0.3), acc)]
    metrics = acc.finish()
    assert torch.equal(c.tonemap(rgb[0], lerp(metrics, metrics, 0.3)), out)
    assert not torch.equal(out, _processor(td, dev, w, h, storage_dtype=storage).process(packed, 'cam'))


def test_pipeline_without_color_and_look_keeps_its_bits(td, dev):
    """color=None, look=None equals the processor built without the keywords, and the stages called one by one as before."""
    from torch_darktable import tonemap
    from torch_darktable.pipeline.util import lerp
    w, h = 256, 192
    packed = _packed(td, dev, w, h, 203)
    a = _processor(td, dev, w, h)
    out = a.process(packed, 'cam')
    assert a.color is None and a.look is None
    b = _processor(td, dev, w, h, color=None, look=None)
    assert torch.equal(b.process(packed, 'cam'), out)
    assert torch.equal(b.process_resized(packed, 'cam'), _processor(td, dev, w, h).process_resized(packed, 'cam'))
    c = _processor(td, dev, w, h)
    rgb = [c.load_image(packed)]
    bounds = tonemap.compute_image_bounds(rgb, stride=8)
    acc = tonemap.MetricsAccumulator(dev, stride=8)
    rgb = [c.process_rgb(rgb[0], lerp(bounds, bounds, 0.3), acc)]
    metrics = acc.finish()
    assert torch.equal(c.tonemap(rgb[0], lerp(metrics, metrics, 0.3)), out)
