"""GPU: the frame statistics (torch_darktable.FrameStats, include/tdk_hip_stats.h) against the NumPy restatement of the specification,
tests/framestats_spec.py (held to independent evaluations in tests/test_framestats_spec.py).

Every counter must be the restatement's integer and every float must have its exact bits: there is no tolerance anywhere in this
file.  Shapes are the smallest that reach the paths: frames smaller than one 16-pixel unit, odd widths whose rows start at every
alignment, buffers that start one element off a vector boundary, strides beyond the frame, and one frame just larger than one sweep
of the fixed grid."""
import numpy as np
import pytest
import torch

import framestats_spec as spec

pytestmark = pytest.mark.gpu

F = np.float32
DTYPES = [np.float32, np.float16, np.uint8, np.uint16]
RANGES = {np.float32: (-0.125, 1.25), np.float16: (-0.125, 1.25), np.uint8: (0, 256), np.uint16: (1000, 60000)}
QUANTILES = (0.0, 0.001, 0.5, 0.999, 1.0)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a visible MI355X'
    return torch.device('cuda', 0)


def upload(a, dev, offset=0):
    """A contiguous device tensor with the contents of `a` that starts `offset` elements behind an allocation's first byte."""
    flat = np.ascontiguousarray(a).reshape(-1)
    if flat.dtype == np.uint16:   # (moved as int16: the bits are what travels)
        buf = torch.empty(flat.size + offset, dtype=torch.int16, device=dev)
        buf[offset:].copy_(torch.from_numpy(flat.view(np.int16)))
        return buf.view(torch.uint16)[offset:].view(a.shape)
    buf = torch.empty(flat.size + offset, dtype=torch.from_numpy(flat[:1]).dtype, device=dev)
    buf[offset:].copy_(torch.from_numpy(flat))
    return buf[offset:].view(a.shape)


def values(rng, shape, dtype):
    """A natural-looking frame over the range of RANGES[dtype], with some values below and above it; the float types also get NaN,
    both infinities, -0 and the ends of the range with their neighbours, scattered."""
    lo, hi = RANGES[dtype]
    v = (rng.gamma(2.0, 0.14, size=shape) - 0.03) * (hi - lo) + lo
    if np.issubdtype(dtype, np.integer):
        return np.clip(np.rint(v), 0, np.iinfo(dtype).max).astype(dtype)
    v = v.astype(dtype)
    flat = v.reshape(-1)
    t = dtype
    special = [np.nan, np.inf, -np.inf, -0.0, t(lo), t(hi), np.nextafter(t(lo), t(-9)), np.nextafter(t(lo), t(9)), np.nextafter(t(hi), t(-9)), np.nextafter(t(hi), t(9))]
    if flat.size >= 40:
        at = rng.choice(flat.size, size=min(flat.size // 4, 3 * len(special)), replace=False)
        flat[at] = np.resize(np.array(special, dtype), at.size)
    return v


def same(result, want, what=''):
    """Every integer equal, every float with the same bits; prints what differs."""
    ok = True
    for field in ('hist', 'below', 'above', 'nan', 'valid', 'sum'):
        got = getattr(result, field).cpu().numpy()
        if got.dtype != np.int64 or not np.array_equal(got, getattr(want, field)):
            print(f'{what}: {field} differs: {np.count_nonzero(got != getattr(want, field))} entries, got sum {got.sum()}, want {getattr(want, field).sum()}')
            ok = False
    for field in ('mean', 'percentiles', 'gains'):
        got, exp = getattr(result, field).cpu().numpy(), getattr(want, field)
        if got.dtype != np.float32 or got.shape != exp.shape or not np.array_equal(got.view(np.int32), exp.view(np.int32)):
            print(f'{what}: {field} differs: got {got.tolist()}, want {exp.tolist()}')
            ok = False
    return ok


def measure(td, dev, frames, pattern=None, offset=0, **kw):
    """(result of the device, restatement) for host frames of one shape."""
    a = frames[0]
    channels = 3 if pattern is not None else a.shape[2]
    fs = td.FrameStats(dev, (a.shape[1], a.shape[0]), channels=channels, bayer_pattern=None if pattern is None else td.BayerPattern[pattern],
                       max_frames=max(len(frames), 1), **kw)
    got = fs.measure([upload(f, dev, offset) for f in frames])
    kw.pop('max_frames', None)
    want = spec.framestats(frames, channels=channels, pattern=None if pattern is None else spec.PATTERNS[pattern], **kw)
    torch.cuda.synchronize()
    return got, want


# ------------------------------------------------------------------ 1. geometry
@pytest.mark.parametrize('w, h', [(2, 2), (6, 4), (34, 18)])
def test_small_mosaics_every_pattern_stride_and_type(td, dev, w, h):
    rng = np.random.default_rng(w * h)
    for dtype in DTYPES:
        m = values(rng, (h, w), dtype)
        for pattern in spec.PATTERNS:
            for stride in (1, 2, 8):
                for offset in (0, 1, 2):
                    got, want = measure(td, dev, [m], pattern, offset, bins=37, value_range=RANGES[dtype], stride=stride, quantiles=QUANTILES, min_count=1)
                    assert same(got, want, f'{w}x{h} {dtype.__name__} {pattern} stride {stride} offset {offset}')
                    assert int(want.hist.sum()) == 4 * -(-(h // 2) // stride) * -(-(w // 2) // stride) - int(want.nan.sum())


@pytest.mark.parametrize('w, h, c', [(1, 1, 1), (33, 17, 3), (35, 9, 1)])
def test_small_images_odd_widths_every_stride_and_type(td, dev, w, h, c):
    """Rows of 33 x 3 or 35 elements start at every alignment of a 16-byte vector; with the buffer one or three elements off as well."""
    rng = np.random.default_rng(w * h + c)
    for dtype in DTYPES:
        x = values(rng, (h, w, c), dtype)
        for stride in (1, 2, 8):
            for offset in (0, 1, 3):
                got, want = measure(td, dev, [x], None, offset, bins=256, value_range=RANGES[dtype], stride=stride, quantiles=QUANTILES, min_count=1)
                assert same(got, want, f'{w}x{h}x{c} {dtype.__name__} stride {stride} offset {offset}')
                assert int(want.hist.sum()) == c * -(-h // stride) * -(-w // stride) - int(want.nan.sum())


# ------------------------------------------------------------------ 2. storage types
@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize('kind', ['rgb', 'grey', 'GRBG'])
def test_storage_types_on_a_mid_size_frame(td, dev, dtype, kind):
    """250 x 334: whole units on aligned and on unaligned rows, heads and tails; 200 bins over a range whose scale is not exact."""
    rng = np.random.default_rng(334)
    w, h = 250, 334
    pattern = kind if kind in spec.PATTERNS else None
    x = values(rng, (h, w) if pattern else (h, w, 3 if kind == 'rgb' else 1), dtype)
    for stride, bins in ((1, 200), (3, 1024)):
        got, want = measure(td, dev, [x], pattern, bins=bins, value_range=RANGES[dtype], stride=stride, quantiles=QUANTILES)
        assert same(got, want, f'{kind} {dtype.__name__} stride {stride} bins {bins}')
    assert want.valid.min() > 64 and (dtype in (np.uint8,) or want.below.sum() > 0 and want.above.sum() > 0)


def test_byte_histogram_is_bincount(td, dev):
    rng = np.random.default_rng(8)
    x = rng.integers(0, 256, size=(120, 200, 3), dtype=np.uint8)
    fs = td.FrameStats(dev, (200, 120), bins=256, value_range=(0, 256))
    hist = fs.measure(upload(x, dev)).hist.cpu().numpy()
    for k in range(3):
        assert np.array_equal(hist[k], np.bincount(x[..., k].ravel(), minlength=256))


# ------------------------------------------------------------------ 3. adversarial values
@pytest.mark.parametrize('dtype', [np.float32, np.float16], ids=lambda d: d.__name__)
def test_nan_infinities_signed_zero_and_the_ends_of_the_range(td, dev, dtype):
    lo, hi = dtype(0.25), dtype(0.75)
    up, down = lambda v: np.nextafter(dtype(v), dtype(9)), lambda v: np.nextafter(dtype(v), dtype(-9))
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, down(lo), lo, up(lo), 0.5, 0.3, down(hi), hi, up(hi)], dtype)
    x = np.resize(special, (16, 24, 3))                       # thirteen values over three channels: every channel sees every value,
    got, want = measure(td, dev, [x], bins=8, value_range=(0.25, 0.75), quantiles=QUANTILES, min_count=1)   # pixels mix valid and invalid members
    assert same(got, want, dtype.__name__)
    assert want.nan.min() > 0 and want.nan.sum() == np.isnan(x).sum() and want.hist.sum() == x.size - want.nan.sum()
    assert want.below.sum() == np.isin(x, special[[2, 3, 4, 5]]).sum() and want.above.sum() == np.isin(x, special[[1, 11, 12]]).sum()
    assert 0 < want.valid[0] < want.hist[0].sum()
    m = np.resize(special, (16, 24))
    got, want = measure(td, dev, [m], 'BGGR', bins=8, value_range=(0.25, 0.75), quantiles=QUANTILES, min_count=1)
    assert same(got, want, f'{dtype.__name__} mosaic') and want.nan.sum() == np.isnan(m).sum() > 0
    nothing = np.full((10, 12, 3), np.nan, dtype)             # an empty histogram: every percentile is lo
    got, want = measure(td, dev, [nothing], bins=16, value_range=(-2, 2), quantiles=QUANTILES)
    assert same(got, want, 'all NaN') and (want.percentiles == F(-2)).all() and want.hist.sum() == 0


@pytest.mark.parametrize('dtype', [np.float32, np.uint8], ids=lambda d: d.__name__)
def test_a_flat_frame_counts_every_lane_into_one_bin(td, dev, dtype):
    value = 0.6 if dtype == np.float32 else 153
    x = np.full((512, 512, 3), value, dtype)
    got, want = measure(td, dev, [x], bins=256, value_range=(0, 1) if dtype == np.float32 else (0, 256), quantiles=QUANTILES)
    assert same(got, want, 'flat') and want.hist[:, 153].tolist() == [512 * 512] * 3
    m = np.full((512, 512), value, dtype)
    got, want = measure(td, dev, [m], 'RGGB', bins=1024, value_range=(0, 1) if dtype == np.float32 else (0, 256), quantiles=QUANTILES)
    assert same(got, want, 'flat mosaic') and want.hist.max(axis=1).tolist() == [65536, 131072, 65536]


def test_a_frame_with_every_value_out_of_range(td, dev):
    rng = np.random.default_rng(5)
    x = (rng.random((64, 96, 3)) + 4 * rng.integers(0, 2, size=(64, 96, 3)) - 2.5).astype(F)   # in [-2.5, -1.5) or [1.5, 2.5)
    got, want = measure(td, dev, [x], bins=64, value_range=(0, 1), quantiles=QUANTILES, min_count=1)
    assert same(got, want, 'out of range')
    assert want.hist.sum() == x.size and want.valid.sum() == 0 and (want.below + want.above).sum() == x.size
    assert (want.mean == 0).all() and want.gains.tolist() == [1, 1, 1]


# ------------------------------------------------------------------ 4. the grid-stride loop
def test_a_frame_just_beyond_one_sweep_of_the_grid(td, dev):
    grid, chunk = td.FrameStats.GRID, td.FrameStats.CHUNK
    w = 2048
    h = grid * chunk // w + 52          # 2100 rows: every workgroup takes a second step, the last ones a short one
    assert w * h > grid * chunk and w * (h - 60) < grid * chunk
    rng = np.random.default_rng(6)
    x = rng.integers(0, 256, size=(h, w, 1), dtype=np.uint8)
    x[:, : w // 2] //= 3                # not uniform: a lost or doubled unit shows in the bins
    got, want = measure(td, dev, [x], bins=256, value_range=(0, 256), quantiles=QUANTILES)
    assert same(got, want, 'sweep')
    assert np.array_equal(want.hist[0], np.bincount(x.ravel(), minlength=256)) and want.valid[0] == w * h


# ------------------------------------------------------------------ 5. sets
def test_three_frames_pool_into_one_result(td, dev):
    rng = np.random.default_rng(7)
    frames = [values(rng, (41, 53, 3), np.float16) for _ in range(3)]
    kw = dict(bins=128, value_range=RANGES[np.float16], quantiles=QUANTILES, min_count=1)
    got, want = measure(td, dev, frames, **kw)
    assert same(got, want, 'set')
    joined = spec.framestats([np.concatenate(frames, axis=0)], **kw)
    assert same(got, joined, 'set against the concatenation')
    fewer, want2 = td.FrameStats(dev, (53, 41), max_frames=3, **kw).measure([upload(f, dev) for f in frames[:2]]), spec.framestats(frames[:2], **kw)
    assert same(fewer, want2, 'two of three slots')
    mosaics = [values(rng, (20, 36), np.uint16) for _ in range(3)]
    got, want = measure(td, dev, mosaics, 'GBRG', bins=512, value_range=RANGES[np.uint16], stride=2, quantiles=QUANTILES, min_count=1)
    assert same(got, want, 'mosaic set')


# ------------------------------------------------------------------ 6. no state survives a call
def test_a_second_frame_on_one_object_two_streams_and_a_graph(td, dev):
    rng = np.random.default_rng(9)
    kw = dict(bins=256, value_range=RANGES[np.float32], quantiles=QUANTILES, min_count=1)
    a, b = values(rng, (130, 170, 3), np.float32), values(rng, (130, 170, 3), np.float32)
    b[:, :, 0] *= F(0.5)
    want_a, want_b = spec.framestats([a], **kw), spec.framestats([b], **kw)
    xa, xb = upload(a, dev), upload(b, dev)
    used = td.FrameStats(dev, (170, 130), **kw)
    first, second = used.measure(xa), used.measure(xb)
    fresh = td.FrameStats(dev, (170, 130), **kw).measure(xb)
    torch.cuda.synchronize()
    assert same(first, want_a, 'A') and same(second, want_b, 'B after A') and same(fresh, want_b, 'B alone')
    # a second stream: its own workspace, the same object
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s1, s2 = used.measure(xa), used.measure(xb)
    main = used.measure(xa)
    side.synchronize()
    torch.cuda.synchronize()
    assert same(s1, want_a, 'A on the side stream') and same(s2, want_b, 'B on the side stream') and same(main, want_a, 'A beside them')
    assert len(used._workspaces) == 2
    # a graph captured as a fresh object's first call, replayed twice, the second time on new contents
    x = xa.clone()
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        obj = td.FrameStats(dev, (170, 130), **kw)   # its workspace for this stream exists before the capture
        with torch.cuda.graph(graph, stream=stream):
            captured = obj.measure(x)
            bounds, gains = obj.bounds(x), obj.white_balance(x)
    graph.replay()
    torch.cuda.synchronize()
    assert same(captured, want_a, 'replay 1')
    x.copy_(xb)
    graph.replay()
    torch.cuda.synchronize()
    assert same(captured, want_b, 'replay 2')
    assert np.array_equal(bounds.cpu().numpy().view(np.int32), want_b.percentiles[3, [0, -1]].view(np.int32))
    assert np.array_equal(gains.cpu().numpy().view(np.int32), want_b.gains.view(np.int32))


def test_bounds_and_gains_feed_the_operators_that_take_device_tensors(td, dev):
    rng = np.random.default_rng(10)
    m = (rng.random((64, 96), dtype=np.float32) * np.tile(np.array([[0.4, 0.8], [0.8, 0.6]], F), (32, 48))).astype(F)   # RGGB: a red and blue cast
    wb = td.FrameStats(dev, (96, 64), bayer_pattern=td.BayerPattern.RGGB, min_count=1)
    x = upload(m, dev)
    gains = wb.white_balance(x)
    want = spec.framestats([m], pattern=spec.PATTERNS['RGGB'], min_count=1)
    assert gains.is_cuda and np.array_equal(gains.cpu().numpy().view(np.int32), want.gains.view(np.int32))
    assert want.gains[0] > 1.5 and want.gains[1] == 1 and want.gains[2] > 1.2
    balanced = td.apply_white_balance(x, gains, td.BayerPattern.RGGB)
    assert torch.equal(balanced, td.apply_white_balance(x, torch.from_numpy(want.gains).to(dev), td.BayerPattern.RGGB))
    q2 = td.FrameStats(dev, (96, 64), channels=1, quantiles=(0.01, 0.99))
    q3 = td.FrameStats(dev, (96, 64), channels=1, quantiles=(0.01, 0.5, 0.99))
    q1 = td.FrameStats(dev, (96, 64), channels=1, quantiles=(0.5,))
    grey = x.unsqueeze(-1)
    assert torch.equal(q2.bounds(grey), q3.bounds(grey)) and tuple(q2.bounds(grey).shape) == (2,)
    assert torch.equal(q1.bounds(grey), q3.measure(grey).percentiles[1, 1].expand(2))


def test_front_end_errors_that_need_a_device(td, dev):
    fs = td.FrameStats(dev, (64, 48), max_frames=2)
    with pytest.raises(RuntimeError, match='contiguous'):
        fs.measure(torch.zeros(48, 64, 6, device=dev)[:, :, ::2])
    with pytest.raises(RuntimeError, match='float32, float16, uint8 or uint16'):
        fs.measure(torch.zeros(48, 64, 3, device=dev, dtype=torch.int32))
    with pytest.raises(RuntimeError, match='share their dtype'):
        fs.measure([torch.zeros(48, 64, 3, device=dev), torch.zeros(48, 64, 3, device=dev, dtype=torch.float16)])


# ------------------------------------------------------------------ 7. pipeline
def _processor(td, dev, w, h, storage_dtype=torch.float32, **kw):
    from torch_darktable.pipeline import ImageProcessingSettings, ImageProcessor, ToneMapper
    settings = ImageProcessingSettings(moving_average=0.3, postprocess=False, enable_denoise=True, enable_bilateral=True, tone_mapping=ToneMapper.reinhard)
    return ImageProcessor((w, h), td.BayerPattern.RGGB, td.PackedFormat.Packed12, settings, dev, (1.4, 1.0, 1.3), storage_dtype=storage_dtype, **kw)


def _packed(td, dev, w, h, seed):
    from torch_darktable.synthetic import synthetic_bayer
    return td.encode12_float(synthetic_bayer(h, w, seed=seed, device='cpu').to(dev).reshape(-1))


@pytest.mark.parametrize('storage', [torch.float32, torch.float16])
def test_pipeline_exposure_takes_the_percentile_bounds(td, dev, storage):
    """ImageProcessor(exposure=fs) against the stages called one by one with fs.bounds in the place of compute_image_bounds, on a set
    of two cameras."""
    from torch_darktable import tonemap
    from torch_darktable.pipeline.util import lerp
    w, h = 256, 192
    packed = {'left': _packed(td, dev, w, h, 301), 'right': _packed(td, dev, w, h, 302)}
    make = lambda: td.FrameStats(dev, (w, h), bins=1024, value_range=(0.0, 2.0), stride=2, quantiles=(0.01, 0.99), max_frames=2)
    out = _processor(td, dev, w, h, storage_dtype=storage, exposure=make()).process_image_set(packed)
    c, fs = _processor(td, dev, w, h, storage_dtype=storage), make()
    rgb = [c.load_image(b) for b in packed.values()]
    bounds = fs.bounds(rgb)
    want = spec.framestats([r.cpu().numpy() for r in rgb], bins=1024, value_range=(0.0, 2.0), stride=2, quantiles=(0.01, 0.99))
    assert np.array_equal(bounds.cpu().numpy().view(np.int32), want.percentiles[3].view(np.int32))
    assert not torch.equal(bounds, tonemap.compute_image_bounds(rgb, stride=8))
    acc = tonemap.MetricsAccumulator(dev, stride=8)
    rgb = [c.process_rgb(img, lerp(bounds, bounds, 0.3), acc) for img in rgb]
    metrics = acc.finish()
    for name, img in zip(packed, rgb):
        assert torch.equal(c.tonemap(img, lerp(metrics, metrics, 0.3)), out[name]), name
    with pytest.raises(ValueError, match='max_frames'):
        _processor(td, dev, w, h, exposure=td.FrameStats(dev, (w, h))).process_image_set(packed)


def test_pipeline_without_exposure_keeps_its_bits(td, dev):
    """exposure=None equals the processor built without the keyword, and the stages called one by one with compute_image_bounds."""
    from torch_darktable import tonemap
    from torch_darktable.pipeline.util import lerp
    w, h = 256, 192
    packed = _packed(td, dev, w, h, 303)
    a = _processor(td, dev, w, h)
    out = a.process(packed, 'cam')
    assert a.exposure is None
    assert torch.equal(_processor(td, dev, w, h, exposure=None).process(packed, 'cam'), out)
    c = _processor(td, dev, w, h)
    rgb = [c.load_image(packed)]
    bounds = tonemap.compute_image_bounds(rgb, stride=8)
    acc = tonemap.MetricsAccumulator(dev, stride=8)
    rgb = [c.process_rgb(rgb[0], lerp(bounds, bounds, 0.3), acc)]
    metrics = acc.finish()
    assert torch.equal(c.tonemap(rgb[0], lerp(metrics, metrics, 0.3)), out)
