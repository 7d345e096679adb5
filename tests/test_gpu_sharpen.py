"""GPU: the sharpener (torch_darktable.Sharpen, include/tdk_hip_sharpen.h) against the NumPy float32 restatement of its
specification, `sharpen_ref` of tests/test_sharpen_spec.py (pinned there to a float64 conv2d computation).

The kernel's output must have the restatement's exact bits: every comparison is torch.equal on the raw bits.  There is no
tolerance anywhere in this file.  Shapes are the smallest that reach the paths: frames smaller than the apron, the seams of the
32 x 32 tile, widths that are and are not whole groups of four pixels (vector and per-element global accesses), offset views."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location('sharpen_spec', Path(__file__).resolve().parent / 'test_sharpen_spec.py')
spec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(spec)
sharpen_ref, gaussian_weights, rand_f, rand_u8 = spec.sharpen_ref, spec.gaussian_weights, spec.rand_f, spec.rand_u8

BITS = {np.dtype(np.float32): np.int32, np.dtype(np.float16): np.int16, np.dtype(np.uint8): np.uint8}
DTYPES = [np.float32, np.float16, np.uint8]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a visible MI355X'
    return torch.device('cuda', 0)


def frame(dtype, shape, seed):
    """Random frame: uint8 over all codes; floats in [0, 1) with a few values outside (negative, above 1)."""
    if dtype == np.uint8:
        return rand_u8(shape, seed)
    x = rand_f(shape, seed)
    x.flat[:: 7] *= np.float32(1.5)
    x.flat[3:: 11] -= np.float32(0.75)
    return x.astype(dtype)


def at_offset(t, elements):
    """A contiguous copy of CUDA tensor `t` that starts `elements` elements past an aligned allocation."""
    pool = torch.zeros(t.numel() + elements + 16, dtype=t.dtype, device=t.device)
    assert pool.data_ptr() % 256 == 0
    v = pool[elements:elements + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() == pool.data_ptr() + elements * t.element_size()
    return v


def same_bits(got, want):
    """got: CUDA or CPU tensor, want: NumPy array of the same dtype and shape."""
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    view = BITS[want.dtype]
    return torch.equal(torch.from_numpy(got.view(view)), torch.from_numpy(np.ascontiguousarray(want).view(view)))


def reference(s, x):
    """The restatement with the parameters of Sharpen object `s` (luminance is dropped for one channel, as process does)."""
    return sharpen_ref(x, s.weights, s.amount, s.threshold, s.luma and x.shape[2] == 3, s.overshoot)


def check(s, dev, x, offset=0, what=''):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    if offset:
        t = at_offset(t, offset)
    out = s.process(t)
    assert tuple(out.shape) == x.shape and out.is_contiguous() and out.data_ptr() != t.data_ptr()
    want = reference(s, x)
    ok = same_bits(out, want)
    if not ok:
        got = out.cpu().numpy()
        bad = np.argwhere(got.view(BITS[want.dtype]) != want.view(BITS[want.dtype]))
        print(f'{what}{x.shape} {x.dtype} {s}: {len(bad)} of {want.size} values differ, first at {bad[0]}: got {got[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r}')
    assert ok, (what, x.shape, x.dtype, repr(s), offset)
    return out


# ------------------------------------------------------------------ 1. frames smaller than the apron
@pytest.mark.parametrize('dtype', DTYPES)
def test_frames_smaller_than_the_apron(td, dev, dtype):
    for h, w in ((1, 1), (3, 2), (5, 17), (17, 5)):
        for c, luma in ((1, False), (3, False), (3, True)):
            s = td.Sharpen(dev, sigma=4.0, amount=1.5, threshold=0.004, luma=luma, overshoot=0.05)
            assert s.radius == 12
            check(s, dev, frame(dtype, (h, w, c), h * 100 + w + c), what='small ')


# ------------------------------------------------------------------ 2. tile seams
@pytest.mark.parametrize('dtype', DTYPES)
def test_tile_seams(td, dev, dtype):
    tw, th = td.Sharpen.TILE
    s3 = td.Sharpen(dev, sigma=1.0, amount=1.0, threshold=0.002, luma=True, overshoot=0.02)
    s1 = td.Sharpen(dev, sigma=1.0, amount=1.0, threshold=0.002, luma=False)
    for w in (tw - 1, tw, tw + 1):
        for h in (th - 1, th, th + 1):
            check(s3, dev, frame(dtype, (h, w, 3), w * 64 + h), what='seam ')
            check(s1, dev, frame(dtype, (h, w, 1), w * 64 + h + 1), what='seam ')
            check(s1, dev, frame(dtype, (h, w, 3), w * 64 + h + 2), what='seam ')


@pytest.mark.parametrize('dtype', DTYPES)
def test_two_tiles_and_a_tail_on_both_axes_at_radius_12(td, dev, dtype):
    tw, th = td.Sharpen.TILE
    h, w = 2 * th + 5, 2 * tw + 3
    for c, luma, overshoot in ((3, True, 0.03), (3, False, None), (1, False, 0.0)):
        check(td.Sharpen(dev, sigma=4.0, amount=2.0, threshold=0.001, luma=luma, overshoot=overshoot), dev, frame(dtype, (h, w, c), 700 + c), what='2 tiles + tail ')


# ------------------------------------------------------------------ 3. every combination
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('width', [150, 152])
def test_every_combination(td, dev, dtype, width):
    """dtype x C x luma x halo limit x sigma on one 90-row frame; width 152 is whole groups of four pixels on an aligned
    allocation (the vector loads and stores), width 150 is not (per element, with a pixel tail)."""
    frames = {c: frame(dtype, (90, width, c), 30 + c + width) for c in (1, 3)}
    assert torch.from_numpy(frames[3]).to(dev).data_ptr() % 16 == 0
    for c in (1, 3):
        for luma in (False, True):
            for overshoot in (None, 0.01):
                for sigma in (0.25, 1.0, 4.0):
                    s = td.Sharpen(dev, sigma=sigma, amount=1.25, threshold=0.003, luma=luma, overshoot=overshoot)
                    check(s, dev, frames[c], what='combination ')


# ------------------------------------------------------------------ 4. alignment
@pytest.mark.parametrize('dtype', DTYPES)
def test_offset_source_and_destination_views(td, dev, dtype):
    """Source and destination one and three elements past an aligned buffer, through the C entry point (process allocates an
    aligned result); W = 150 is no multiple of 4, W = 152 is and loses its vector path to the offset alone."""
    from torch_darktable._native import lib
    import ctypes

    for w in (150, 152):
        for c, luma in ((3, True), (3, False), (1, False)):
            s = td.Sharpen(dev, sigma=1.0, amount=1.0, threshold=0.002, luma=luma, overshoot=0.02)
            x = frame(dtype, (45, w, c), 41 + c + w)
            want = reference(s, x)
            for off in (1, 3):
                check(s, dev, x, offset=off, what=f'source offset {off} ')
                for src_off in (0, off):
                    t = torch.from_numpy(x).to(dev)
                    if src_off:
                        t = at_offset(t, src_off)
                    pool = torch.zeros(x.size + off + 32, dtype=t.dtype, device=dev)
                    out = pool[off:off + x.size]
                    assert out.data_ptr() % (4 * t.element_size()) != 0
                    weights = (ctypes.c_float * len(s.weights))(*s.weights)
                    rc = lib.tdk_sharpen(t.data_ptr(), out.data_ptr(), w, 45, c, {np.float32: 0, np.float16: 1, np.uint8: 2}[dtype], weights, s.radius,
                                         s.amount, s.threshold, s.overshoot, (1 if luma else 0) | 2, torch.cuda.current_stream().cuda_stream)
                    assert rc == 0, lib.tdk_last_error()
                    torch.cuda.synchronize()
                    assert same_bits(out.view(x.shape), want), (w, c, luma, off, src_off)
                    assert float(pool[:off].float().abs().max()) == 0 and float(pool[off + x.size:].float().abs().max()) == 0   # nothing written outside


# ------------------------------------------------------------------ 5. edge values
def test_uint8_extremes_side_by_side(td, dev):
    """0 and 255 beside each other: results beyond [0, 255] are clamped.  With taps (0.5, 0.25) and amount 0.5 every intermediate
    is a multiple of 1/32 below 2^9, exact in float32, so the result is known without rounding and exact k + 1/2 ties reach
    rint (to even)."""
    x = np.zeros((40, 53, 3), np.uint8)
    x[:, 1::2] = 255
    x[::3, :, 1] = 255
    x[7:23, 11:40] = rand_u8((16, 29, 3), 5) // 128 * 255
    r = rand_u8((40, 53, 3), 6)
    for luma in (False, True):
        for overshoot in (None, 0.0):
            s = td.Sharpen.from_weights(dev, (0.5, 0.25), amount=0.5, luma=luma, overshoot=overshoot)
            check(s, dev, x, what='0/255 ')
            check(s, dev, r, what='ties ')
            check(td.Sharpen(dev, sigma=1.0, amount=16.0, luma=luma, overshoot=overshoot), dev, x, what='0/255 amount 16 ')

    def blur(a, axis):
        n = a.shape[axis]
        before, after = np.take(a, np.clip(np.arange(n) - 1, 0, n - 1), axis=axis), np.take(a, np.clip(np.arange(n) + 1, 0, n - 1), axis=axis)
        return 0.5 * a + 0.25 * (before + after)

    for img in (x, r):
        exact = img.astype(np.float64)
        unrounded = exact + 0.5 * (exact - blur(blur(exact, 1), 0))
        got = td.Sharpen.from_weights(dev, (0.5, 0.25), amount=0.5, luma=False).process(torch.from_numpy(img).to(dev)).cpu().numpy()
        assert np.array_equal(got, np.rint(np.clip(unrounded, 0, 255)).astype(np.uint8))
    assert (unrounded - np.floor(unrounded) == 0.5).sum() > 50            # the random frame does contain ties
    assert (unrounded < 0).any() and (unrounded > 255).any()              # and values to clamp


def test_float16_near_its_largest_values_with_amount_zero(td, dev):
    x = frame(np.float16, (37, 45, 3), 6)
    x[::2, ::3] = np.float16(65504.0)
    x[1::2, 1::3] = np.float16(-65504.0)
    x[5, 5] = np.float16(-0.0)
    x[6, 6] = np.float16(6e-8)   # a subnormal
    for luma in (False, True):
        s = td.Sharpen(dev, sigma=2.0, amount=0.0, luma=luma, overshoot=0.0)
        out = check(s, dev, x, what='f16 max ')
        assert same_bits(out, x)
    f = frame(np.float32, (37, 45, 1), 7)
    f[3, 3] = np.float32(-0.0)
    assert same_bits(check(td.Sharpen(dev, amount=0.0), dev, f), f)
    u = rand_u8((37, 45, 3), 8)
    assert same_bits(check(td.Sharpen(dev, amount=0.0, overshoot=0.1), dev, u), u)


# ------------------------------------------------------------------ 6. a caller's own kernel
@pytest.mark.parametrize('dtype', DTYPES)
def test_custom_weights_radius_1(td, dev, dtype):
    for c, luma in ((1, False), (3, False), (3, True)):
        s = td.Sharpen.from_weights(dev, (0.5, 0.25), amount=1.0, threshold=0.01, luma=luma, overshoot=0.02)
        assert s.radius == 1 and s.weights == (0.5, 0.25)
        check(s, dev, frame(dtype, (67, 71, c), 60 + c), what='custom ')
    # weights that do not sum to 1 are taken as they are
    check(td.Sharpen.from_weights(dev, (0.3, 0.2, 0.1), amount=0.75, luma=False), dev, frame(dtype, (40, 44, 3), 64), what='custom unnormalised ')


# ------------------------------------------------------------------ 7. reproducibility, graph capture, streams
def test_two_runs_are_bit_identical(td, dev):
    for dtype in DTYPES:
        x = torch.from_numpy(frame(dtype, (301, 403, 3), 71)).to(dev)
        s = td.Sharpen(dev, sigma=2.0, amount=1.0, threshold=0.002, overshoot=0.02)
        assert torch.equal(s.process(x).view(torch.uint8), s.process(x).view(torch.uint8))


@pytest.mark.parametrize('dtype', DTYPES)
def test_graph_capture_from_the_first_call(td, dev, dtype):
    """A parameter set no earlier call of this process has used, captured on a side stream without a warm-up call; the replay
    equals the restatement bit for bit, also after the input buffer's contents change."""
    s = td.Sharpen(dev, sigma=1.3, amount=0.9, threshold=0.0015, luma=True, overshoot=0.015)
    a, b = frame(dtype, (131, 173, 3), 81), frame(dtype, (131, 173, 3), 82)
    x = torch.from_numpy(a).to(dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            captured = s.process(x)
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(captured, reference(s, a))
    x.copy_(torch.from_numpy(b).to(dev))
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(captured, reference(s, b)) and same_bits(s.process(x), reference(s, b))


def test_non_default_stream(td, dev):
    s = td.Sharpen(dev, sigma=1.0, amount=1.0, luma=False)
    a = frame(np.uint8, (97, 131, 3), 91)
    x = torch.from_numpy(a).to(dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        out = s.process(x)
    stream.synchronize()
    assert same_bits(out, reference(s, a))


def test_front_end_errors_that_need_a_device(td, dev):
    s = td.Sharpen(dev)
    with pytest.raises(RuntimeError, match='contiguous'):
        s.process(torch.zeros(48, 128, 3, device=dev)[:, ::2])
    with pytest.raises(RuntimeError, match='float32, float16 or uint8'):
        s.process(torch.zeros(48, 64, 3, device=dev, dtype=torch.int32))
    x = torch.zeros(48, 64, 3, device=dev)
    from torch_darktable._native import lib
    import ctypes
    w = (ctypes.c_float * 2)(0.5, 0.25)
    assert lib.tdk_sharpen(x.data_ptr(), x.data_ptr(), 64, 48, 3, 0, w, 1, 0.5, 0.0, 0.0, 0, None) == 1 and b'overlap' in lib.tdk_last_error()


# ------------------------------------------------------------------ 8. pipeline
def _processor(td, dev, w, h, resize_width, sharpen=None, transforms=None):
    from torch_darktable.pipeline import ImageProcessingSettings, ImageProcessor, ImageTransform, ToneMapper
    settings = ImageProcessingSettings(moving_average=0.3, postprocess=False, enable_denoise=True, enable_bilateral=True,
                                       tone_mapping=ToneMapper.reinhard, resize_width=resize_width)
    kw = {} if sharpen is None else {'sharpen': sharpen}
    return ImageProcessor((w, h), td.BayerPattern.RGGB, td.PackedFormat.Packed12, settings, dev, (1.4, 1.0, 1.3),
                          transforms=transforms or ImageTransform.none, **kw)


def _packed(td, dev, w, h, seed):
    from torch_darktable.synthetic import synthetic_bayer
    return td.encode12_float(synthetic_bayer(h, w, seed=seed, device='cpu').to(dev).reshape(-1))


def test_pipeline_sharpens_after_the_tone_mapper_and_the_scaler(td, dev):
    from torch_darktable.pipeline import ImageTransform
    from torch_darktable.pipeline.transform import transform
    w, h = 256, 192
    packed = _packed(td, dev, w, h, 101)
    s = td.Sharpen(dev, sigma=1.0, amount=0.8, threshold=0.004, overshoot=0.03)
    plain = _processor(td, dev, w, h, 100).process(packed, 'cam')
    assert plain.dtype == torch.uint8 and tuple(plain.shape) == (h, w, 3)
    out = _processor(td, dev, w, h, 100, s).process(packed, 'cam')
    assert torch.equal(out, s.process(plain)) and not torch.equal(out, plain)
    assert same_bits(out, reference(s, plain.cpu().numpy()))
    small_plain = _processor(td, dev, w, h, 100).process_resized(packed, 'cam')
    assert tuple(small_plain.shape) == (75, 100, 3)
    small = _processor(td, dev, w, h, 100, s).process_resized(packed, 'cam')
    assert torch.equal(small, s.process(small_plain)) and not torch.equal(small, small_plain)
    # before the orientation
    turned = _processor(td, dev, w, h, 100, s, ImageTransform.rotate_90).process(packed, 'cam')
    assert torch.equal(turned, transform(out, ImageTransform.rotate_90))


def test_pipeline_without_a_sharpener_keeps_its_bits(td, dev):
    """sharpen=None (and the argument left out, which is how from_camera_settings builds a processor) returns what the stages give
    when they are called one by one as `process` called them before the hook existed."""
    from torch_darktable import tonemap
    from torch_darktable.pipeline import CameraSettings, ImageProcessor, ImageTransform
    from torch_darktable.pipeline.util import lerp
    w, h = 256, 192
    packed = _packed(td, dev, w, h, 102)
    a = _processor(td, dev, w, h, 0)
    out = a.process(packed, 'cam')
    assert a.sharpen is None
    cam = CameraSettings(name='cam', image_size=(w, h), padding=0, white_balance=(1.4, 1.0, 1.3), image_processing=a.settings, transform=ImageTransform.none)
    b = ImageProcessor.from_camera_settings(cam, dev)
    assert b.sharpen is None and torch.equal(b.process(packed, 'cam'), out)
    c = _processor(td, dev, w, h, 0)
    rgb = [c.load_image(packed)]
    bounds = tonemap.compute_image_bounds(rgb, stride=8)
    acc = tonemap.MetricsAccumulator(dev, stride=8)
    rgb = [c.process_rgb(rgb[0], lerp(bounds, bounds, 0.3), acc)]
    metrics = acc.finish()
    assert torch.equal(c.tonemap(rgb[0], lerp(metrics, metrics, 0.3)), out)


# ------------------------------------------------------------------ 9. full size
def test_12mp_uint8_frame_on_windows(td, dev):
    """One 4096 x 3072 uint8 run (the pipeline's call: luminance, sigma 1, halo limit), checked on three interior windows that
    cross tile seams and on one window touching each edge.  The restatement runs on each window cut out with a margin of R + 1
    pixels (the blur reaches R, the limit 1); where the cut coincides with the frame's edge its replicate border is the frame's."""
    h, w = 3072, 4096
    x = rand_u8((h, w, 3), 111)
    s = td.Sharpen(dev, sigma=1.0, amount=1.0, threshold=0.004, luma=True, overshoot=0.02)
    out = s.process(torch.from_numpy(x).to(dev)).cpu().numpy()
    m = s.radius + 1
    windows = [(1500, 1600, 2000, 2100), (40, 140, 3000, 3100), (2900, 3000, 50, 150),        # interior
               (0, 70, 1000, 1100), (h - 70, h, 2000, 2100), (1000, 1100, 0, 70), (2000, 2100, w - 70, w),   # top, bottom, left, right
               (0, 40, 0, 40), (h - 40, h, w - 40, w)]                                                # two corners
    for y0, y1, x0, x1 in windows:
        cy0, cy1, cx0, cx1 = max(y0 - m, 0), min(y1 + m, h), max(x0 - m, 0), min(x1 + m, w)
        want = reference(s, x[cy0:cy1, cx0:cx1])[y0 - cy0:y1 - cy0, x0 - cx0:x1 - cx0]
        assert same_bits(torch.from_numpy(np.ascontiguousarray(out[y0:y1, x0:x1])), want), (y0, y1, x0, x1)
    assert not np.array_equal(out, x)
