"""GPU: the noise profile (torch_darktable.NoiseProfile / NoiseModel, include/tdk_hip_noise.h) against the NumPy restatement of the
specification, tests/noiseprofile_spec.py (held to independent evaluations in tests/test_noiseprofile_spec.py).

Every counter must be the restatement's integer and every float must have its exact bits: there is no tolerance anywhere in this
file.  Shapes are the smallest that reach the paths: one block per plane, no complete block, tails that are ignored, strips with one
tile and with a partial last strip, buffers that start one element off a vector boundary, one frame just larger than one sweep of the
fixed grid, and for the transform every tail length of the vector, rows that straddle vectors and one launch in which every lane
loops."""
import numpy as np
import pytest
import torch

import noiseprofile_spec as spec

pytestmark = pytest.mark.gpu

F = np.float32
PATTERNS = {'RGGB': spec.RGGB, 'BGGR': spec.BGGR, 'GRBG': spec.GRBG, 'GBRG': spec.GBRG}
DTYPES = [np.float32, np.float16, np.uint16]


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


def mosaic(rng, h, w, dtype=np.float32, special=False):
    """A ramp with signal-dependent noise, so that several intensity bins and levels fill; white is 1 (65535 for uint16).  `special`
    scatters NaN, both infinities, zeros and saturated sites."""
    yy, xx = np.mgrid[0:h, 0:w]
    v = 0.04 + 0.85 * (xx / max(w - 1, 1)) * (0.3 + 0.7 * yy / max(h - 1, 1))
    v = v + rng.normal(0.0, 1.0, (h, w)) * np.sqrt(3e-4 * v + 2e-6)
    if np.issubdtype(dtype, np.integer):
        v = np.clip(np.rint(v * 65535.0), 0, 65535).astype(dtype)
        if special:
            flat = v.reshape(-1)
            at = rng.choice(flat.size, size=max(flat.size // 200, 4), replace=False)
            flat[at] = np.resize(np.array([0, 65535, 1, 64224, 64225], dtype), at.size)
        return v
    v = v.astype(dtype)
    if special:
        flat = v.reshape(-1)
        at = rng.choice(flat.size, size=max(flat.size // 200, 8), replace=False)
        flat[at] = np.resize(np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, 1.5, -0.25], dtype), at.size)
    return v


def white_of(dtype):
    return 65535.0 if dtype == np.uint16 else 1.0


def same_estimate(stats, model, want, what=''):
    """Every integer equal, every float with the same bits; prints what differs."""
    counts, want_model, want_curve = want
    bins = want_curve.shape[2]
    words = 3 * bins * spec.LEVELS
    got = np.concatenate([t.cpu().numpy().reshape(-1) for t in (stats.hist, stats.sum, stats.blocks, stats.nan, stats.clipped)])
    ok = True
    if got.dtype != np.int64 or not np.array_equal(got, counts):
        bad = np.flatnonzero(got != counts)
        print(f'{what}: counts differ at {bad[:8].tolist()} of {bad.size} (levels end at {words}): got {got[bad[:8]].tolist()}, want {counts[bad[:8]].tolist()}')
        ok = False
    for name, g, w in (('model', model.model.cpu().numpy(), want_model), ('curve', model.curve.cpu().numpy(), want_curve)):
        if g.dtype != np.float32 or g.shape != w.shape or not np.array_equal(g.view(np.int32), w.view(np.int32)):
            print(f'{what}: {name} differs: got {g.tolist()}, want {w.tolist()}')
            ok = False
    return ok


def run(td, dev, frames, pattern, offset=0, **kw):
    """(statistics, model of the device, restatement) for host frames of one shape."""
    a = frames[0]
    kw.setdefault('white', white_of(a.dtype.type))
    profile = td.NoiseProfile(dev, (a.shape[1], a.shape[0]), td.BayerPattern[pattern], max_frames=len(frames), **kw)
    x = [upload(f, dev, offset) for f in frames]
    stats, model = profile.statistics(x), profile.estimate(x)
    want = spec.estimate(frames, PATTERNS[pattern], **kw)
    torch.cuda.synchronize()
    return stats, model, want


# ------------------------------------------------------------------ 1. estimation: geometry
def test_one_block_per_plane_no_block_and_ignored_tails(td, dev):
    rng = np.random.default_rng(1)
    for h, w, blocks in ((16, 16, 1), (14, 18, 0), (18, 14, 0), (50, 94, 15), (16, 2, 0), (2, 16, 0)):
        for dtype in DTYPES:
            m = mosaic(rng, h, w, dtype)
            stats, model, want = run(td, dev, [m], 'RGGB', min_count=1)
            assert same_estimate(stats, model, want, f'{w}x{h} {dtype.__name__}')
            assert stats.blocks.cpu().tolist() == [blocks, 2 * blocks, blocks]
            if blocks == 0:
                assert not want[0].any() and not model.model.cpu().numpy().any() and not model.curve.cpu().numpy().any()
    stats, model, want = run(td, dev, [mosaic(rng, 50, 94)], 'RGGB', min_count=1)
    assert (model.valid.cpu().numpy() == 1).all()   # the chart is worth a fit: the comparison above is not one of zeros


@pytest.mark.parametrize('pattern', list(PATTERNS))
def test_every_pattern_and_storage_type(td, dev, pattern):
    rng = np.random.default_rng(2)
    for dtype in DTYPES:
        m = mosaic(rng, 48, 80, dtype, special=True)
        for offset in (0, 1):
            for kw in (dict(min_count=1), dict(bins=7, clip=(0, 65535), min_count=2)):
                stats, model, want = run(td, dev, [m], pattern, offset, **kw)
                assert same_estimate(stats, model, want, f'{pattern} {dtype.__name__} offset {offset} {kw}')
    assert int(stats.nan.sum()) == 0 and int(stats.blocks.sum()) == 60


def test_partial_strips_and_special_values(td, dev):
    """144 columns are 9 tiles: a full float32 strip and one of a single tile, a partial 16-bit strip; 272 columns are 17 tiles: a full
    16-bit strip and one of a single tile.  NaN, both infinities, zeros and saturated sites are scattered; white is not 1."""
    rng = np.random.default_rng(3)
    for w, h in ((144, 32), (272, 34)):
        for dtype in DTYPES:
            m = mosaic(rng, h, w, dtype, special=True)
            for offset in (0, 1, 3):
                kw = dict(min_count=1, white=white_of(dtype) * 0.9, clip=(1, 65534))
                stats, model, want = run(td, dev, [m], 'GRBG', offset, **kw)
                assert same_estimate(stats, model, want, f'{w}x{h} {dtype.__name__} offset {offset}')
            if dtype != np.uint16:
                assert int(stats.nan.sum()) > 0
            assert int(stats.clipped.sum()) > 0


def test_a_set_of_three_frames_pools(td, dev):
    rng = np.random.default_rng(4)
    for dtype in (np.float32, np.uint16):
        frames = [mosaic(rng, 34, 50, dtype, special=(i == 1)) for i in range(3)]
        stats, model, want = run(td, dev, frames, 'BGGR', min_count=2)
        assert same_estimate(stats, model, want, f'set {dtype.__name__}')
        assert stats.blocks.cpu().tolist() == [18, 36, 18]


@pytest.mark.parametrize('dtype, w, h', [(np.float32, 144, 4160), (np.uint16, 16, 8208)], ids=['float32', 'uint16'])
def test_one_frame_beyond_one_sweep_of_the_grid(td, dev, dtype, w, h):
    """float32: 260 rows of tiles of two strips each, 520 units; uint16: 513 rows of one strip: more than the 512 workgroups."""
    rng = np.random.default_rng(5)
    m = mosaic(rng, h, w, dtype, special=True)
    stats, model, want = run(td, dev, [m], 'GBRG')
    assert same_estimate(stats, model, want, f'{w}x{h}')
    assert (model.valid.cpu().numpy() == 1).all()


# ------------------------------------------------------------------ 2. no state survives a call
def test_twice_on_one_workspace_two_streams_and_a_graph(td, dev):
    rng = np.random.default_rng(6)
    P, kw = td.BayerPattern.RGGB, dict(min_count=1)
    a, b = mosaic(rng, 64, 96), mosaic(rng, 64, 96, special=True)
    want_a, want_b = spec.estimate([a], spec.RGGB, **kw), spec.estimate([b], spec.RGGB, **kw)
    xa, xb = upload(a, dev), upload(b, dev)
    used = td.NoiseProfile(dev, (96, 64), P, **kw)
    r = [(used.statistics(x), used.estimate(x)) for x in (xa, xb, xb)]
    torch.cuda.synchronize()
    assert same_estimate(*r[0], want_a, 'A') and same_estimate(*r[1], want_b, 'B after A') and same_estimate(*r[2], want_b, 'B again')
    # a second stream: its own workspace, the same object
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s = [(used.statistics(x), used.estimate(x)) for x in (xa, xb)]
    main = (used.statistics(xa), used.estimate(xa))
    side.synchronize()
    torch.cuda.synchronize()
    assert same_estimate(*s[0], want_a, 'A on the side stream') and same_estimate(*s[1], want_b, 'B on the side stream') and same_estimate(*main, want_a, 'A beside them')
    assert len(used._workspaces) == 2
    # a graph captured as a fresh object's first call: estimate, and the model straight into stabilize; replayed on new contents
    x = xa.clone()
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        obj = td.NoiseProfile(dev, (96, 64), P, **kw)   # its workspace for this stream exists before the capture
        with torch.cuda.graph(graph, stream=stream):
            stats = obj.statistics(x)
            model = obj.estimate(x)
            flat = model.stabilize(x, bayer_pattern=P, sigma_out=0.5)
    graph.replay()
    torch.cuda.synchronize()
    assert same_estimate(stats, model, want_a, 'replay 1')
    x.copy_(xb)
    graph.replay()
    torch.cuda.synchronize()
    assert same_estimate(stats, model, want_b, 'replay 2')
    want = spec.stabilize(b, want_b[1], spec.RGGB, None, 0.5)
    assert np.array_equal(flat.cpu().numpy().view(np.int32), want.view(np.int32))


# ------------------------------------------------------------------ 3. the transform
MODEL = np.array([[2e-4, 1e-6, 1, 20], [5e-5, 4e-6, 1, 20], [1e-3, 1e-5, 1, 20]], F)
DEGENERATE = np.array([[0.0, 4e-4, 1, 5], [2e-4, 1e-6, 0, 1], [0.0, 0.0, 1, 3]], F)   # Gaussian, invalid, nothing known
MIXED = np.array([[3e-4, 0.0, 1, 9], [0.0, 4e-4, 1, 5], [1e-3, 1e-5, 1, 7]], F)
GAINS = np.array([1.9, 1.0, 1.4], F)
TORCH = {np.float32: torch.float32, np.float16: torch.float16}


def bits(a):
    """The bit patterns, with every NaN as one pattern: which NaN an operation returns is not part of the specification."""
    out = a.view(np.int32 if a.dtype == np.float32 else np.int16).copy()
    out[np.isnan(a)] = -1
    return out


def both_ways(td, dev, x, model, pattern=None, gains=None, sigma_out=1.0, offset=0, out=np.float32, what=''):
    """stabilize, then unstabilize its result with both inverses, each against the restatement."""
    m = td.NoiseModel(torch.from_numpy(model).to(dev))
    P = None if pattern is None else td.BayerPattern[pattern]
    word = None if pattern is None else PATTERNS[pattern]
    g = None if gains is None else torch.from_numpy(gains).to(dev)
    y = m.stabilize(upload(x, dev, offset), P, g, sigma_out, TORCH[out])
    want_y = spec.stabilize(x, model, word, gains, sigma_out, out)
    ok = y.dtype == TORCH[out] and tuple(y.shape) == x.shape and np.array_equal(bits(y.cpu().numpy()), bits(want_y))
    if not ok:
        print(f'{what}: stabilize differs in {np.count_nonzero(bits(y.cpu().numpy()) != bits(want_y))} of {want_y.size}')
    for inverse in ('unbiased', 'algebraic'):
        for back in (None, np.float32 if out == np.float16 else np.float16):
            z = m.unstabilize(upload(want_y, dev, offset), P, g, sigma_out, inverse, None if back is None else TORCH[back])
            want_z = spec.unstabilize(want_y, model, word, gains, sigma_out, inverse, back)
            if z.dtype != TORCH[want_z.dtype.type] or not np.array_equal(bits(z.cpu().numpy()), bits(want_z)):
                print(f'{what}: unstabilize {inverse} -> {back} differs in {np.count_nonzero(bits(z.cpu().numpy()) != bits(want_z))} of {want_z.size}')
                ok = False
    return ok


def signal(rng, shape, dtype):
    x = rng.uniform(-0.02, 1.1, shape).astype(dtype)
    if x.size >= 16:
        flat = x.reshape(-1)
        flat[rng.choice(flat.size, 6, replace=False)] = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0], dtype)
    return x


def test_transform_every_tail_type_and_offset(td, dev):
    rng = np.random.default_rng(7)
    shapes = [(n, 3) for n in (1, 5, 6, 7, 8)] + [(n, 1) for n in (1, 2, 3, 4, 9)] + [(3, 7, 1), (37, 29, 3)]
    for shape in shapes:
        for src in (np.float32, np.float16):
            for out in (np.float32, np.float16):
                x = signal(rng, shape, src)
                for offset in (0, 1):
                    for gains in (None, GAINS):
                        assert both_ways(td, dev, x, MODEL, None, gains, 1.0, offset, out, f'{shape} {src.__name__}->{out.__name__} offset {offset}')
    for shape, pattern in (((6, 8), 'RGGB'), ((10, 14), 'GRBG'), ((2, 2), 'BGGR'), ((38, 54), 'GBRG')):   # 14 and 54 columns: vectors straddle rows
        for src in (np.float32, np.float16):
            for out in (np.float32, np.float16):
                x = signal(rng, shape, src)
                for offset in (0, 1):
                    assert both_ways(td, dev, x, MODEL, pattern, GAINS, 0.25, offset, out, f'{shape} {pattern} {src.__name__}->{out.__name__} offset {offset}')


def test_transform_degenerate_rows(td, dev):
    rng = np.random.default_rng(8)
    for model in (DEGENERATE, MIXED):
        for gains in (None, GAINS, np.array([0.0, 1.0, 2.0], F)):
            assert both_ways(td, dev, signal(rng, (21, 13, 3), np.float32), model, None, gains, 0.5, what='rgb')
            assert both_ways(td, dev, signal(rng, (12, 10), np.float32), model, 'GRBG', gains, 2.0, what='mosaic')
            assert both_ways(td, dev, signal(rng, (50, 1), np.float16), model, None, gains, 1.0, out=np.float16, what='grey')


@pytest.mark.parametrize('shape, pattern', [((700, 1001, 3), None), ((1450, 1450), 'GRBG')], ids=['rgb', 'mosaic'])
def test_transform_beyond_one_sweep_of_its_grid(td, dev, shape, pattern):
    """More than 2048 * 256 * 4 elements: every lane loops, and the channel phase of an RGB image moves with the stride."""
    rng = np.random.default_rng(9)
    x = rng.uniform(0.0, 1.0, shape).astype(F)
    m = td.NoiseModel(torch.from_numpy(MODEL).to(dev))
    P = None if pattern is None else td.BayerPattern[pattern]
    word = None if pattern is None else PATTERNS[pattern]
    g = torch.from_numpy(GAINS).to(dev)
    xd = upload(x, dev)
    y = m.stabilize(xd, P, g)
    z = m.unstabilize(y, P, g, out_dtype=torch.float16)
    want_y = spec.stabilize(x, MODEL, word, GAINS)
    assert np.array_equal(bits(y.cpu().numpy()), bits(want_y))
    assert np.array_equal(bits(z.cpu().numpy()), bits(spec.unstabilize(want_y, MODEL, word, GAINS, out_dtype=np.float16)))


def test_an_estimated_model_goes_straight_into_stabilize(td, dev):
    rng = np.random.default_rng(10)
    m = mosaic(rng, 64, 96)
    P = td.BayerPattern.GBRG
    model = td.NoiseProfile(dev, (96, 64), P, min_count=1).estimate(upload(m, dev))
    y = model.stabilize(upload(m, dev), P)
    back = model.unstabilize(y, P, inverse='algebraic')
    _, want_model, _ = spec.estimate([m], spec.GBRG, min_count=1)
    assert (want_model[:, 2] == 1).all() and (want_model[:, 0] > 0).all()
    want_y = spec.stabilize(m, want_model, spec.GBRG)
    assert np.array_equal(bits(y.cpu().numpy()), bits(want_y))
    assert np.array_equal(bits(back.cpu().numpy()), bits(spec.unstabilize(want_y, want_model, spec.GBRG, inverse='algebraic')))
    assert np.abs(back.cpu().numpy() - m).max() < 1e-4
    d = model.to_dict()
    assert d['valid'] == [True] * 3 and d['a'] == [float(v) for v in want_model[:, 0]] and d['bins'] == [int(v) for v in want_model[:, 3]]
    again = td.NoiseModel.from_dict(d, dev)
    assert torch.equal(again.model, model.model)


# ------------------------------------------------------------------ 4. pipeline
def _processor(td, dev, w, h, **kw):
    from torch_darktable.pipeline import ImageProcessingSettings, ImageProcessor, ImageTransform, ToneMapper
    settings = ImageProcessingSettings(moving_average=0.3, postprocess=False, enable_denoise=True, enable_bilateral=True, tone_mapping=ToneMapper.reinhard)
    return ImageProcessor((w, h), td.BayerPattern.RGGB, td.PackedFormat.Packed12, settings, dev, (1.4, 1.0, 1.3), transforms=ImageTransform.none, **kw)


def _by_hand(c, rgb, dev):
    """The stages after the chroma denoiser, called one by one as `process` calls them."""
    from torch_darktable import tonemap
    from torch_darktable.pipeline.util import lerp
    bounds = tonemap.compute_image_bounds([rgb], stride=8)
    acc = tonemap.MetricsAccumulator(dev, stride=8)
    rgb = c.process_rgb(rgb, lerp(bounds, bounds, 0.3), acc)
    metrics = acc.finish()
    return c.tonemap(rgb, lerp(metrics, metrics, 0.3))


@pytest.mark.parametrize('storage', [torch.float32, torch.float16], ids=['float32', 'float16'])
def test_pipeline_runs_the_denoiser_inside_the_transform(td, dev, storage):
    from torch_darktable.synthetic import synthetic_bayer
    w, h = 96, 64
    packed = td.encode12_float(synthetic_bayer(h, w, seed=103, device='cpu').to(dev).reshape(-1))
    wav = td.Wavelet.from_sigma(dev, (w, h), (1.0, 1.0, 1.0), scales=3)
    model = td.NoiseModel.from_values((2e-4, 1.5e-4, 3e-4), 2e-6, dev)
    plain = _processor(td, dev, w, h, chroma_denoise=wav, storage_dtype=storage)
    out_plain = plain.process(packed, 'cam')
    out = _processor(td, dev, w, h, chroma_denoise=wav, noise_model=model, storage_dtype=storage).process(packed, 'cam')
    assert out.dtype == torch.uint8 and tuple(out.shape) == (h, w, 3) and not torch.equal(out, out_plain)
    # the three stages by hand, in the place of the chroma denoiser
    c = _processor(td, dev, w, h, storage_dtype=storage)
    loaded = c.load_image(packed)
    assert loaded.dtype == storage
    flat = model.stabilize(loaded, gains=c.white_balance)
    assert flat.dtype == torch.float32
    restored = model.unstabilize(wav.process(flat), gains=c.white_balance, out_dtype=storage)
    assert restored.dtype == storage
    assert torch.equal(out, _by_hand(c, restored, dev))
    # without a model: the stage on the frame as it is, as before the hook existed
    assert plain.noise_model is None
    assert torch.equal(out_plain, _by_hand(c, wav.process(loaded), dev))
    assert torch.equal(_processor(td, dev, w, h, chroma_denoise=wav, noise_model=None, storage_dtype=storage).process(packed, 'cam'), out_plain)
