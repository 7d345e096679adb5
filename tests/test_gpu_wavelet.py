"""GPU: the wavelet denoiser (include/tdk_hip_wavelet.h, csrc/wavelet.hip, torch_darktable.Wavelet) against `wavelet_ref`, the
float32 restatement of the specification in tests/test_wavelet_spec.py.  Every comparison is on the raw bits: no tolerance anywhere."""

import ctypes
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location('wavelet_spec', Path(__file__).resolve().parent / 'test_wavelet_spec.py')
spec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(spec)
wavelet_ref, bands, forward, inverse = spec.wavelet_ref, spec.bands, spec.forward, spec.inverse

BITS = {np.dtype(np.float32): np.int32, np.dtype(np.float16): np.int16, np.dtype(np.uint8): np.uint8}
DTYPES = [np.float32, np.float16]
MODES = [(1, False), (3, False), (3, True)]   # (channels, ycc)
TAG = {np.float32: 0, np.float16: 1}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a visible MI355X'
    return torch.device('cuda', 0)


def frame(dtype, shape, seed):
    """Random frame in [0, 1) with a few values outside (negative, above 1)."""
    x = np.random.default_rng(seed).random(shape, dtype=np.float32)
    x.flat[:: 7] *= np.float32(1.5)
    x.flat[3:: 11] -= np.float32(0.75)
    return x.astype(dtype)


def thresholds(scales, channels, seed=0):
    """Per scale and channel, all different, of the size of the details of `frame` (some coefficients survive, some do not)."""
    t = 0.004 + 0.05 * np.random.default_rng(1000 + seed).random((scales, channels))
    assert len(set(t.flat)) == t.size
    return t.astype(np.float32)


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


def make(td, dev, x, t, ycc):
    return td.Wavelet(dev, (x.shape[1], x.shape[0]), len(t), [list(map(float, row)) for row in t], ycc)


def check(td, dev, x, t, ycc, offset=0, what=''):
    w = make(td, dev, x, t, ycc)
    src = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    if offset:
        src = at_offset(src, offset)
    out = w.process(src)
    assert tuple(out.shape) == x.shape and out.is_contiguous() and out.data_ptr() != src.data_ptr()
    want = wavelet_ref(x, t, ycc)
    ok = same_bits(out, want)
    if not ok:
        got = out.cpu().numpy()
        bad = np.argwhere(got.view(BITS[want.dtype]) != want.view(BITS[want.dtype]))
        print(f'{what}{x.shape} {x.dtype} S={len(t)} ycc={ycc}: {len(bad)} of {want.size} values differ, first at {bad[0]}: '
              f'got {got[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r}')
    assert ok, (what, x.shape, x.dtype, len(t), ycc, offset)
    return out


# ------------------------------------------------------------------ 1. frames smaller than the support
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('channels,ycc', MODES)
def test_frames_smaller_than_the_support(td, dev, dtype, channels, ycc):
    for i, (h, w) in enumerate([(1, 1), (3, 2), (5, 70), (70, 5)]):
        check(td, dev, frame(dtype, (h, w, channels), 10 + i), thresholds(5, channels, i), ycc)


# ------------------------------------------------------------------ 2. tile seams
@pytest.mark.parametrize('dtype', DTYPES)
def test_tile_seams(td, dev, dtype):
    tw, th = td.Wavelet.TILE
    for w in (tw - 1, tw, tw + 1):
        for h in (th - 1, th, th + 1):
            for channels, ycc in MODES:
                check(td, dev, frame(dtype, (h, w, channels), 20 + w + h), thresholds(3, channels, w), ycc)
                check(td, dev, frame(dtype, (h, w, channels), 21 + w + h), thresholds(2, channels, h), ycc)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('channels,ycc', MODES)
def test_two_tiles_and_a_tail_on_both_axes_at_five_scales(td, dev, dtype, channels, ycc):
    tw, th = td.Wavelet.TILE
    check(td, dev, frame(dtype, (2 * th + 5, 2 * tw + 3, channels), 30), thresholds(5, channels, 3), ycc)


# ------------------------------------------------------------------ 3. every combination
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('width', [150, 152])
@pytest.mark.parametrize('scales', [1, 2, 3, 4, 5])
def test_every_combination(td, dev, dtype, width, scales):
    """W = 150: stores per element; W = 152 on an aligned allocation: vectors of four elements."""
    for channels, ycc in MODES:
        check(td, dev, frame(dtype, (90, width, channels), 40 + scales + channels), thresholds(scales, channels, scales), ycc)


# ------------------------------------------------------------------ 4. limits
@pytest.mark.parametrize('dtype', DTYPES)
def test_zero_thresholds_give_the_restatements_bits(td, dev, dtype):
    """Not the input's: c_0 - c_1 + ... + c_S rounds at every step, which float32 storage shows (binary16 storage rounds the
    float32 sum back to the input's value almost everywhere, so there only the restatement is asked for)."""
    for channels, ycc in MODES:
        x = frame(dtype, (75, 83, channels), 50)
        out = check(td, dev, x, np.zeros((5, channels), np.float32), ycc)
        assert dtype is np.float16 or not same_bits(out, x)


@pytest.mark.parametrize('dtype', DTYPES)
def test_thresholds_above_every_detail_leave_the_coarsest_scale(td, dev, dtype):
    for channels, ycc in MODES:
        x = frame(dtype, (75, 83, channels), 51)
        out = check(td, dev, x, np.full((4, channels), 100.0, np.float32), ycc)
        _, c = bands(forward(x, ycc), 4)
        assert same_bits(out, inverse(c, ycc).astype(dtype))   # acc is +0 everywhere: 0 + c_S


def test_float16_extremes_subnormals_and_negative_zero(td, dev):
    """Without the colour transform, so that nothing overflows: a filter is a convex combination and stays within +-65504, a detail
    of two extremes stays below 2^17 in float32, and the result is the input up to the shrinkage -- where Y, Cb and Cr of such values
    would leave the binary16 range on the way back."""
    rng = np.random.default_rng(52)
    special = np.array([65504.0, -65504.0, 6e-8, -6e-8, 6.1e-5, -0.0, 0.0, 1.0], dtype=np.float16)
    for channels in (1, 3):
        x = special[rng.integers(0, len(special), (70, 77, channels))]
        x[:3, :3] = np.float16(-0.0)
        for t in (0.0, 1e-7, 1000.0):
            check(td, dev, x, np.full((5, channels), t, np.float32), False)
        flat = np.full((40, 45, channels), -0.0, dtype=np.float16)
        out = check(td, dev, flat, np.zeros((3, channels), np.float32), False)
        assert out.cpu().numpy().view(np.int16).tolist() == wavelet_ref(flat, np.zeros((3, channels), np.float32)).view(np.int16).tolist()


# ------------------------------------------------------------------ 5. alignment
@pytest.mark.parametrize('dtype', DTYPES)
def test_offset_source_and_destination_views(td, dev, dtype):
    """Source and destination one and three elements past an aligned buffer, through the C entry point (process allocates an
    aligned result); W = 150 is no multiple of 4, W = 152 is and loses its vector path to the offset alone.  The workspace is offset too."""
    from torch_darktable._native import lib

    for w in (150, 152):
        for channels, ycc in MODES:
            for scales in (2, 5):
                x = frame(dtype, (45, w, channels), 60 + channels + w)
                t = thresholds(scales, channels, w)
                want = wavelet_ref(x, t, ycc)
                carr = (ctypes.c_float * t.size)(*map(float, t.flat))
                nws = lib.tdk_wavelet_workspace_bytes(w, 45, channels, scales)
                for off in (1, 3):
                    check(td, dev, x, t, ycc, offset=off, what=f'source offset {off} ')
                    for src_off in (0, off):
                        src = torch.from_numpy(x).to(dev)
                        if src_off:
                            src = at_offset(src, src_off)
                        pool = torch.zeros(x.size + off + 32, dtype=src.dtype, device=dev)
                        out = pool[off:off + x.size]
                        assert out.data_ptr() % (4 * src.element_size()) != 0
                        wpool = torch.zeros(nws + 64, dtype=torch.uint8, device=dev)
                        ws = wpool[off:off + nws]
                        rc = lib.tdk_wavelet(src.data_ptr(), out.data_ptr(), ws.data_ptr() if nws else None, w, 45, channels, TAG[dtype], scales, carr,
                                             1 if ycc else 0, torch.cuda.current_stream().cuda_stream)
                        assert rc == 0, lib.tdk_last_error()
                        torch.cuda.synchronize()
                        assert same_bits(out.view(x.shape), want), (w, channels, ycc, scales, off, src_off)
                        assert float(pool[:off].float().abs().max()) == 0 and float(pool[off + x.size:].float().abs().max()) == 0   # nothing written outside
                        assert int(wpool[:off].max()) == 0 and int(wpool[off + nws:].max()) == 0


# ------------------------------------------------------------------ 6. launches
def test_a_call_makes_at_most_scales_minus_one_launches(td, dev):
    from torch_darktable import _native

    x = torch.from_numpy(frame(np.float16, (90, 150, 3), 70)).to(dev)
    for scales in range(1, 6):
        w = td.Wavelet(dev, (150, 90), scales, 0.01, ycc=True)
        _native.profile_enable(True)
        try:
            w.process(x)
            torch.cuda.synchronize()
            report = _native.profile_report()
        finally:
            _native.profile_enable(False)
        ours = {name: n for name, (n, _) in report.items() if name.startswith('tdk_wavelet(')}
        print(scales, ours)
        assert sum(ours.values()) <= max(1, scales - 1) and ours.get('tdk_wavelet(fine)') == 1, (scales, report)
        assert set(ours) == {'tdk_wavelet(fine)'} | {f'tdk_wavelet(scale {s})' for s in range(td.Wavelet.FUSED, scales)}
        assert all(name.startswith('tdk_wavelet(') for name in report), report


# ------------------------------------------------------------------ 7. reproducibility, graph capture, streams
def test_two_runs_are_bit_identical(td, dev):
    for dtype in DTYPES:
        x = torch.from_numpy(frame(dtype, (301, 403, 3), 71)).to(dev)
        w = td.Wavelet(dev, (403, 301), 5, 0.01, ycc=True)
        assert torch.equal(w.process(x).view(torch.uint8), w.process(x).view(torch.uint8))


@pytest.mark.parametrize('dtype', DTYPES)
def test_graph_capture_from_the_first_call(td, dev, dtype):
    """An object built on the side stream and captured there without a warm-up call (its workspace exists since construction); the
    replay equals the restatement bit for bit, also after the input buffer's contents change."""
    a, b = frame(dtype, (131, 173, 3), 81), frame(dtype, (131, 173, 3), 82)
    t = thresholds(5, 3, 8)
    x = torch.from_numpy(a).to(dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        w = make(td, dev, a, t, True)
        with torch.cuda.graph(graph, stream=stream):
            captured = w.process(x)
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(captured, wavelet_ref(a, t, True))
    x.copy_(torch.from_numpy(b).to(dev))
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(captured, wavelet_ref(b, t, True)) and same_bits(w.process(x), wavelet_ref(b, t, True))


def test_non_default_stream(td, dev):
    a = frame(np.float16, (97, 131, 3), 91)
    t = thresholds(4, 3, 9)
    w = make(td, dev, a, t, True)
    x = torch.from_numpy(a).to(dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        out = w.process(x)
    stream.synchronize()
    assert same_bits(out, wavelet_ref(a, t, True))


def test_one_object_on_two_streams_at_once(td, dev):
    """Different inputs on two streams, the calls interleaved: each stream has its own planes between the launches."""
    a, b = frame(np.float32, (300, 420, 3), 92), frame(np.float32, (300, 420, 3), 93)
    t = thresholds(5, 3, 10)
    w = make(td, dev, a, t, True)
    xa, xb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    for s in (s1, s2):
        s.wait_stream(torch.cuda.current_stream())
    outs = []
    for _ in range(3):
        with torch.cuda.stream(s1):
            oa = w.process(xa)
        with torch.cuda.stream(s2):
            ob = w.process(xb)
        outs.append((oa, ob))
    torch.cuda.synchronize()
    assert len(w._workspaces) == 3   # the constructing stream's and one per side stream
    wa, wb = wavelet_ref(a, t, True), wavelet_ref(b, t, True)
    for oa, ob in outs:
        assert same_bits(oa, wa) and same_bits(ob, wb)


# ------------------------------------------------------------------ 8. a frame of many tiles
def test_multi_tile_frame_on_windows(td, dev):
    """700 x 900 float16, luma/chroma, five scales.  A window is cut with a margin of 63 pixels (the support is 62): the restatement
    of the cut equals that of the frame wherever the margin, or the frame's own edge, surrounds a pixel."""
    h, w, m = 900, 700, 63
    x = frame(np.float16, (h, w, 3), 95)
    t = thresholds(5, 3, 11)
    out = make(td, dev, x, t, True).process(torch.from_numpy(x).to(dev)).cpu().numpy()
    windows = {'interior': (400, 300), 'top': (0, 250), 'bottom': (h - 96, 310), 'left': (333, 0), 'right': (410, w - 96),
               'top-left': (0, 0), 'bottom-right': (h - 96, w - 96)}
    for name, (y0, x0) in windows.items():
        ya, yb, xa, xb = max(y0 - m, 0), min(y0 + 96 + m, h), max(x0 - m, 0), min(x0 + 96 + m, w)
        want = wavelet_ref(x[ya:yb, xa:xb], t, True)[y0 - ya:y0 - ya + 96, x0 - xa:x0 - xa + 96]
        got = out[y0:y0 + 96, x0:x0 + 96]
        assert np.array_equal(got.view(np.int16), want.view(np.int16)), name


# ------------------------------------------------------------------ 9. pipeline
def _processor(td, dev, w, h, **kw):
    from torch_darktable.pipeline import ImageProcessingSettings, ImageProcessor, ImageTransform, ToneMapper
    settings = ImageProcessingSettings(moving_average=0.3, postprocess=False, enable_denoise=True, enable_bilateral=True, tone_mapping=ToneMapper.reinhard)
    return ImageProcessor((w, h), td.BayerPattern.RGGB, td.PackedFormat.Packed12, settings, dev, (1.4, 1.0, 1.3), transforms=ImageTransform.none, **kw)


def _packed(td, dev, w, h, seed):
    from torch_darktable.synthetic import synthetic_bayer
    return td.encode12_float(synthetic_bayer(h, w, seed=seed, device='cpu').to(dev).reshape(-1))


def _by_hand(c, rgb, dev):
    """The stages after load_image, called one by one as `process` calls them."""
    from torch_darktable import tonemap
    from torch_darktable.pipeline.util import lerp
    bounds = tonemap.compute_image_bounds([rgb], stride=8)
    acc = tonemap.MetricsAccumulator(dev, stride=8)
    rgb = c.process_rgb(rgb, lerp(bounds, bounds, 0.3), acc)
    metrics = acc.finish()
    return c.tonemap(rgb, lerp(metrics, metrics, 0.3))


def test_pipeline_denoises_every_demosaiced_frame_before_the_bounds(td, dev):
    w, h = 256, 192
    packed = _packed(td, dev, w, h, 101)
    wav = td.Wavelet.from_sigma(dev, (w, h), (0.02, 0.015, 0.025), scales=4)
    plain = _processor(td, dev, w, h).process(packed, 'cam')
    out = _processor(td, dev, w, h, chroma_denoise=wav).process(packed, 'cam')
    assert out.dtype == torch.uint8 and tuple(out.shape) == (h, w, 3) and not torch.equal(out, plain)
    c = _processor(td, dev, w, h)
    loaded = c.load_image(packed)
    denoised = wav.process(loaded)
    assert same_bits(denoised, wavelet_ref(loaded.cpu().numpy(), np.array(wav.thresholds, np.float32), True))
    assert torch.equal(_by_hand(c, denoised, dev), out)
    with pytest.raises(ValueError, match='chroma_denoise is for 128x192'):
        _processor(td, dev, w, h, chroma_denoise=td.Wavelet(dev, (128, h)))
    with pytest.raises(ValueError, match='three channels'):
        _processor(td, dev, w, h, chroma_denoise=td.Wavelet(dev, (w, h), 2, [[0.1], [0.1]]))
    with pytest.raises(TypeError, match='chroma_denoise must be a Wavelet'):
        _processor(td, dev, w, h, chroma_denoise=td.Sharpen(dev))


def test_pipeline_without_a_chroma_denoiser_keeps_its_bits(td, dev):
    """chroma_denoise=None (and the argument left out, which is how from_camera_settings builds a processor) returns what the stages
    give when they are called one by one as `process` called them before the hook existed."""
    from torch_darktable.pipeline import CameraSettings, ImageProcessor, ImageTransform
    w, h = 256, 192
    packed = _packed(td, dev, w, h, 102)
    a = _processor(td, dev, w, h)
    out = a.process(packed, 'cam')
    assert a.chroma_denoise is None
    assert torch.equal(_processor(td, dev, w, h, chroma_denoise=None).process(packed, 'cam'), out)
    cam = CameraSettings(name='cam', image_size=(w, h), padding=0, white_balance=(1.4, 1.0, 1.3), image_processing=a.settings, transform=ImageTransform.none)
    b = ImageProcessor.from_camera_settings(cam, dev)
    assert b.chroma_denoise is None and torch.equal(b.process(packed, 'cam'), out)
    c = _processor(td, dev, w, h)
    assert torch.equal(_by_hand(c, c.load_image(packed), dev), out)


# ------------------------------------------------------------------ 10. front end
def test_front_end_errors_that_need_a_device(td, dev):
    from torch_darktable._native import lib

    w = td.Wavelet(dev, (64, 48), 3, 0.01)
    with pytest.raises(RuntimeError, match='contiguous'):
        w.process(torch.zeros(48, 128, 3, device=dev)[:, ::2])
    with pytest.raises(RuntimeError, match='float32, float16 or uint8'):
        w.process(torch.zeros(48, 64, 3, device=dev, dtype=torch.int32))
    with pytest.raises(RuntimeError, match='unsupported dtype'):
        w.process(torch.zeros(48, 64, 3, device=dev, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match='expected'):
        w.process(torch.zeros(48, 32, 3, device=dev))
    with pytest.raises(ValueError, match='channels must be 3'):
        td.Wavelet(dev, (64, 48), 1, [[0.1, 0.1, 0.1]]).process(torch.zeros(48, 64, 1, device=dev))
    with pytest.raises(ValueError, match='channels must be 3 with ycc'):
        td.Wavelet(dev, (64, 48), 1, 0.1, ycc=True).process(torch.zeros(48, 64, 1, device=dev))
    x = torch.zeros(48, 64, 3, device=dev)
    t = (ctypes.c_float * 9)(*([0.01] * 9))
    ws = torch.zeros(lib.tdk_wavelet_workspace_bytes(64, 48, 3, 3), dtype=torch.uint8, device=dev)
    assert lib.tdk_wavelet(x.data_ptr(), x.data_ptr(), ws.data_ptr(), 64, 48, 3, 0, 3, t, 0, None) == 1 and b'overlap' in lib.tdk_last_error()
    assert lib.tdk_wavelet(x.data_ptr(), ws.data_ptr(), ws.data_ptr(), 64, 48, 3, 0, 3, t, 0, None) == 1 and b'workspace overlaps' in lib.tdk_last_error()
    # the luminance front ends: extract -> process -> replace
    from torch_darktable.extension import extension
    rgb = torch.from_numpy(frame(np.float32, (48, 64, 3), 97)).abs().to(dev)
    lum = extension.compute_log_luminance(rgb, 1e-4)
    assert torch.equal(w.process_log_luminance(rgb), extension.modify_log_luminance(rgb, w.process(lum.unsqueeze(2)).squeeze(2), 1e-4))
    lum = extension.compute_luminance(rgb)
    assert torch.equal(w.process_luminance(rgb), extension.modify_luminance(rgb, w.process(lum.unsqueeze(2)).squeeze(2)))
