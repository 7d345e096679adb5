"""GPU: the temporal denoiser (torch_darktable.TemporalDenoise, include/tdk_hip_temporal.h) against the NumPy restatement of the
specification, tests/temporal_spec.py (held to a second evaluation and to the algorithm's purpose in tests/test_temporal_spec.py).

After every step the output, both planes of the state the step wrote and the frame index must have the restatement's exact bits:
there is no tolerance anywhere in this file.  Shapes are sized by the tile of a workgroup and are the smallest that reach the paths:
one cell, a frame smaller than the apron, one whole tile, a tile with a two-site rim of partial tiles (rows that alternate between
the vector and the per-element path), an interior tile with eight neighbours, one row and one column of tiles."""
import numpy as np
import pytest
import torch

import temporal_spec as spec

pytestmark = pytest.mark.gpu

F = np.float32
PATTERNS = {'RGGB': spec.RGGB, 'BGGR': spec.BGGR, 'GRBG': spec.GRBG, 'GBRG': spec.GBRG}
TORCH = {np.float32: torch.float32, np.float16: torch.float16}
MODEL = np.array([[3e-4, 2e-6, 1, 20], [2e-4, 1e-6, 1, 20], [5e-4, 3e-6, 1, 20]], F)
GAINS = np.array([2.0, 1.0, 1.5], F)
FRAMES = 6   # first, static, static, motion and special values, static, one after reset()


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a visible MI355X'
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def tile(td):
    return td.TemporalDenoise.TILE   # (TW, TH)


def upload(a, dev, offset=0):
    """A contiguous device tensor with the contents of `a` that starts `offset` elements behind an allocation's first byte."""
    flat = np.ascontiguousarray(a).reshape(-1)
    buf = torch.empty(flat.size + offset, dtype=torch.from_numpy(flat[:1]).dtype, device=dev)
    buf[offset:].copy_(torch.from_numpy(flat))
    return buf[offset:].view(a.shape)


def bits(a):
    """The bit patterns, with every NaN as one pattern: which NaN an operation returns is not part of the specification."""
    a = np.asarray(a)
    out = a.view(np.int32 if a.dtype == np.float32 else np.int16).copy()
    out[np.isnan(a)] = -1
    return out


def sequence(h, w, dtype=np.float32, seed=0):
    """The six frames of a shape: a ramp with signal-dependent noise; the fourth has a rectangle moved in and NaN, both infinities, a
    negative, a zero and a 65504 site."""
    rng = np.random.default_rng(1000 * h + w + seed)
    yy, xx = np.mgrid[0:h, 0:w]
    clean = 0.05 + 0.8 * (xx / max(w - 1, 1)) * (0.4 + 0.6 * yy / max(h - 1, 1))
    frames = []
    for f in range(FRAMES):
        scene = clean.copy()
        if f == 3:
            scene[h // 4:h // 4 + max(h // 3, 1), w // 3:w // 3 + max(w // 4, 1)] += 0.3
        x = (scene + rng.normal(0.0, 1.0, (h, w)) * np.sqrt(3e-4 * scene + 2e-6)).astype(dtype)
        if f == 3:
            flat = x.reshape(-1)
            special = np.array([np.nan, np.inf, -np.inf, -0.25, 0.0, 65504.0], dtype)
            at = rng.choice(flat.size, size=min(flat.size, special.size), replace=False)
            flat[at] = special[:at.size]
        frames.append(x)
    return frames


def same_step(t, key, out, want, state, what):
    """The output, the two planes the step wrote and the index word against the restatement; prints what differs."""
    torch.cuda.synchronize()
    acc, cnt = t.state(key)
    want_acc, want_cnt = state.next_read()
    ok = True
    for name, g, w in (('out', out.cpu().numpy(), want), ('acc', acc.cpu().numpy(), want_acc), ('cnt', cnt.cpu().numpy(), want_cnt)):
        if g.dtype != w.dtype or g.shape != w.shape or not np.array_equal(bits(g), bits(w)):
            bad = np.argwhere(bits(g) != bits(w)) if g.shape == w.shape and g.dtype == w.dtype else []
            print(f'{what}: {name} differs at {len(bad)} sites, first {[tuple(b) for b in bad[:6]]}: got {[g[tuple(b)] for b in bad[:6]]}, want {[w[tuple(b)] for b in bad[:6]]}')
            ok = False
    idx = int(t.frames(key).item())
    if idx != state.idx:
        print(f'{what}: index {idx}, want {state.idx}')
        ok = False
    return ok


def run(td, dev, h, w, pattern='RGGB', model=MODEL, gains=None, src=np.float32, state=np.float32, out=None, offset=0, fill=None, what='', **kw):
    """The six-frame sequence of one object against the restatement, compared after every step."""
    m = td.NoiseModel(torch.from_numpy(np.asarray(model, F)).to(dev))
    t = td.TemporalDenoise(dev, (w, h), td.BayerPattern[pattern], m, state_dtype=TORCH[state], **kw)
    if fill is not None:
        t._states[None].fill_(fill)
        t.reset()
    g = None if gains is None else torch.from_numpy(gains).to(dev)
    ref = spec.State((h, w), state)
    ok = True
    for f, frame in enumerate(sequence(h, w, src)):
        if f == FRAMES - 1:
            t.reset()
            ref.reset()
            assert int(t.frames().item()) == 0
        got = t.process(upload(frame, dev, offset), gains=g, out_dtype=None if out is None else TORCH[out])
        want = spec.step(frame, ref, model, PATTERNS[pattern], gains=gains, out_dtype=out, **kw)
        ok = same_step(t, None, got, want, ref, f'{what} {w}x{h} frame {f + 1}') and ok
        if f in (0, FRAMES - 1):
            assert np.array_equal(bits(got.cpu().numpy()), bits(frame.astype(got.cpu().numpy().dtype))), 'the first frame passes through'
    return ok


# ------------------------------------------------------------------ 1. geometry
def shapes(tile):
    tw, th = tile
    return [(2, 2), (4, 6), (th, tw), (th + 2, tw + 2), (3 * th + 2, 3 * tw - 2), (2, 2 * tw + 2), (2 * th + 2, 2)]


@pytest.mark.parametrize('radius', [2, 3])
@pytest.mark.parametrize('which', range(7))
def test_every_shape_at_both_radii(td, dev, tile, which, radius):
    h, w = shapes(tile)[which]
    for offset in (0, 1):   # the frame starts on an allocation's first byte, and one element behind it
        assert run(td, dev, h, w, radius=radius, offset=offset, what=f'radius {radius} offset {offset}')


@pytest.mark.parametrize('pattern', list(PATTERNS))
def test_every_pattern(td, dev, tile, pattern):
    tw, th = tile
    for radius in (2, 3):
        assert run(td, dev, th + 2, tw + 2, pattern, gains=GAINS, radius=radius, what=pattern)


@pytest.mark.parametrize('src', [np.float32, np.float16], ids=['src32', 'src16'])
@pytest.mark.parametrize('state', [np.float32, np.float16], ids=['state32', 'state16'])
@pytest.mark.parametrize('out', [np.float32, np.float16], ids=['out32', 'out16'])
def test_every_combination_of_storage_types(td, dev, tile, src, state, out):
    tw, th = tile
    for radius, offset in ((2, 1), (3, 0)):
        assert run(td, dev, th + 2, tw + 2, 'GRBG', src=src, state=state, out=out, radius=radius, offset=offset, what=f'{src.__name__}/{state.__name__}/{out.__name__}')


def test_an_output_one_element_behind_an_allocation(td, dev, tile):
    """`process` returns a fresh tensor, which starts on an allocation; the C entry point takes an output at any element alignment."""
    from torch_darktable._native import check, lib
    from torch_darktable.torch_darktable_extension import _ptr, _stream

    tw, th = tile
    h, w = th + 2, tw + 2
    for np_out, radius in ((np.float32, 2), (np.float16, 3)):
        m = td.NoiseModel(torch.from_numpy(MODEL).to(dev))
        t = td.TemporalDenoise(dev, (w, h), td.BayerPattern.RGGB, m, radius=radius)
        ref = spec.State((h, w))
        for f, frame in enumerate(sequence(h, w)[:4]):
            x = upload(frame, dev, 1)
            out = upload(np.zeros((h, w), np_out), dev, 1)
            check(lib.tdk_temporal_denoise(_ptr(x), 0, _ptr(out), 0 if np_out == np.float32 else 1, _ptr(t._states[None]), 0, w, h, spec.RGGB, _ptr(m.model), None,
                                           radius, 1.5, 3.0, 16.0, 8.0, 1e-12, _stream()))
            want = spec.step(frame, ref, MODEL, spec.RGGB, radius=radius, out_dtype=np_out)
            assert same_step(t, None, out, want, ref, f'offset output frame {f + 1}')


# ------------------------------------------------------------------ 2. parameters
def test_gains_and_degenerate_models(td, dev, tile):
    tw, th = tile
    h, w = th + 2, tw + 2
    invalid_green = MODEL.copy()
    invalid_green[1, 2] = 0
    no_shot = MODEL.copy()
    no_shot[:, 0] = 0
    nothing = np.array([[0.0, 0.0, 1, 0]] * 3, F)
    for name, model in (('invalid green', invalid_green), ('a = 0', no_shot), ('a = b = 0', nothing)):
        for gains in (None, GAINS):
            assert run(td, dev, h, w, 'GBRG', model=model, gains=gains, radius=2, what=name)
    assert run(td, dev, h, w, gains=GAINS, radius=3, what='gains')


def test_max_frames_and_the_pixel_test(td, dev, tile):
    tw, th = tile
    h, w = th + 2, tw + 2
    for kw in (dict(max_frames=64.0), dict(max_frames=2.5), dict(pixel_threshold=None), dict(thresholds=(0.8, 1.1), pixel_threshold=2.0), dict(variance_floor=1e-5)):
        assert run(td, dev, h, w, radius=2, what=str(kw), **kw)
    # max_frames = 1: the output is the input's bits, whatever they are
    m = td.NoiseModel(torch.from_numpy(MODEL).to(dev))
    for dtype in (np.float32, np.float16):
        t = td.TemporalDenoise(dev, (w, h), td.BayerPattern.RGGB, m, max_frames=1.0, radius=3)
        for frame in sequence(h, w, dtype):
            x = upload(frame, dev)
            out = t.process(x)
            assert out.dtype == x.dtype and out.data_ptr() != x.data_ptr()
            assert np.array_equal(out.cpu().numpy().view(np.int32 if dtype == np.float32 else np.int16), frame.view(np.int32 if dtype == np.float32 else np.int16))
            assert (t.state()[1] == 1).all()


def test_a_state_of_ff_bytes_is_not_trusted(td, dev, tile):
    tw, th = tile
    for state in (np.float32, np.float16):
        assert run(td, dev, th + 2, tw + 2, state=state, radius=2, fill=0xFF, what='0xFF state')


# ------------------------------------------------------------------ 3. keys, streams, graphs
def test_two_keys_interleaved_share_nothing(td, dev, tile):
    tw, th = tile
    h, w = th + 2, tw + 2
    m = td.NoiseModel(torch.from_numpy(MODEL).to(dev))
    t = td.TemporalDenoise(dev, (w, h), td.BayerPattern.RGGB, m)
    t.prepare(['left', 'right'])
    assert set(t._states) == {None, 'left', 'right'} and len({s.data_ptr() for s in t._states.values()}) == 3
    seq = {'left': sequence(h, w, seed=1), 'right': sequence(h, w, seed=2)}
    ref = {k: spec.State((h, w)) for k in seq}
    for f in range(5):
        for key in (('left', 'right') if f != 2 else ('right',)):   # 'left' misses a frame: the parities of the two keys differ from then on
            got = t.process(upload(seq[key][f], dev), key=key)
            assert same_step(t, key, got, spec.step(seq[key][f], ref[key], MODEL, spec.RGGB), ref[key], f'{key} frame {f + 1}')
    t.reset(key='left')
    ref['left'].reset()
    assert int(t.frames('left').item()) == 0 and int(t.frames('right').item()) == 5 and int(t.frames().item()) == 0
    for key in ('left', 'right', 'third'):   # a key first seen in process is prepared there
        frame = seq.get(key, seq['left'])[5]
        got = t.process(upload(frame, dev), key=key)
        assert same_step(t, key, got, spec.step(frame, ref.setdefault(key, spec.State((h, w))), MODEL, spec.RGGB), ref[key], f'{key} after the reset of left')
    t.reset()
    assert [int(t.frames(k).item()) for k in (None, 'left', 'right', 'third')] == [0, 0, 0, 0]


def test_two_keys_on_two_streams(td, dev, tile):
    tw, th = tile
    h, w = 3 * th + 2, 3 * tw - 2
    m = td.NoiseModel(torch.from_numpy(MODEL).to(dev))
    t = td.TemporalDenoise(dev, (w, h), td.BayerPattern.RGGB, m, radius=3)
    t.prepare(['a', 'b'])
    seq = {'a': sequence(h, w, seed=3), 'b': sequence(h, w, seed=4)}
    inputs = {k: [upload(x, dev) for x in v[:5]] for k, v in seq.items()}
    streams = {k: torch.cuda.Stream(device=dev) for k in seq}
    outs = {k: [] for k in seq}
    for s in streams.values():
        s.wait_stream(torch.cuda.current_stream())   # the resets and the uploads are in front of both
    for f in range(5):
        for key, s in streams.items():
            with torch.cuda.stream(s):
                outs[key].append(t.process(inputs[key][f], key=key))
    for s in streams.values():
        s.synchronize()
    for key in seq:
        ref = spec.State((h, w))
        for f in range(5):
            want = spec.step(seq[key][f], ref, MODEL, spec.RGGB, radius=3)
            assert np.array_equal(bits(outs[key][f].cpu().numpy()), bits(want)), (key, f)
        assert same_step(t, key, outs[key][4], want, ref, f'stream {key}')


def test_a_captured_call_replays_an_odd_number_of_times(td, dev, tile):
    tw, th = tile
    h, w = th + 2, tw + 2
    m = td.NoiseModel(torch.from_numpy(MODEL).to(dev))
    t = td.TemporalDenoise(dev, (w, h), td.BayerPattern.RGGB, m)
    t.prepare(['graph', 'eager'])   # ahead of the capture: the captured call allocates nothing but its result
    frames = sequence(h, w, seed=5)[:5]
    x = upload(frames[0], dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            out = t.process(x, key='graph')
    torch.cuda.synchronize()
    assert int(t.frames('graph').item()) == 0   # a capture runs nothing
    replayed = []
    for frame in frames:
        x.copy_(torch.from_numpy(frame))
        graph.replay()
        replayed.append(out.clone())
    torch.cuda.synchronize()
    ref = spec.State((h, w))
    for f, frame in enumerate(frames):
        eager = t.process(upload(frame, dev), key='eager')
        want = spec.step(frame, ref, MODEL, spec.RGGB)
        assert torch.equal(replayed[f].view(torch.int32), eager.view(torch.int32)), f
        assert np.array_equal(bits(eager.cpu().numpy()), bits(want)), f
    assert same_step(t, 'graph', replayed[4], want, ref, 'graph') and same_step(t, 'eager', eager, want, ref, 'eager')
    assert (t.state('graph')[1] > 1).any()
    # the model is read from device memory by every call: an in-place update reaches the captured call
    m.model.copy_(torch.from_numpy(np.array([[0.0, 0.0, 1, 0]] * 3, F)))
    x.copy_(torch.from_numpy(frames[1]))
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), frames[1]) and (t.state('graph')[1] == 1).all()   # a model without noise: everything is motion


# ------------------------------------------------------------------ 4. pipeline
def _processor(td, dev, w, h, **kw):
    from torch_darktable.pipeline import ImageProcessingSettings, ImageProcessor, ImageTransform, ToneMapper
    settings = ImageProcessingSettings(moving_average=0.3, postprocess=False, enable_denoise=True, enable_bilateral=True, tone_mapping=ToneMapper.reinhard)
    return ImageProcessor((w, h), td.BayerPattern.RGGB, td.PackedFormat.Packed12, settings, dev, (1.4, 1.0, 1.3), transforms=ImageTransform.none, **kw)


def _packed_frames(td, dev, w, h, count=2, sigma=0.004):
    from torch_darktable.synthetic import synthetic_bayer
    base = synthetic_bayer(h, w, seed=104, device='cpu', noise_sigma=0.0) * 0.8 + 0.05
    g = torch.Generator(device='cpu').manual_seed(7)
    return [td.encode12_float((base + sigma * torch.randn(base.shape, generator=g)).clamp(0.0, 1.0).to(dev).reshape(-1)) for _ in range(count)]


def test_pipeline_with_one_frame_of_history_is_the_plain_pipeline(td, dev):
    w, h = 96, 64
    frames = _packed_frames(td, dev, w, h)
    m = td.NoiseModel.from_values(0.0, 1.6e-5, dev)
    plain = _processor(td, dev, w, h)
    with_temporal = _processor(td, dev, w, h, temporal=td.TemporalDenoise(dev, (w, h), td.BayerPattern.RGGB, m, max_frames=1.0))
    for packed in frames:
        a, b = plain.process(packed, 'cam'), with_temporal.process(packed, 'cam')
        assert a.dtype == torch.uint8 and tuple(a.shape) == (h, w, 3) and torch.equal(a, b)
    assert int(with_temporal.temporal.frames('cam').item()) == 2 and int(with_temporal.temporal.frames().item()) == 0   # the image name is the key
    assert plain.temporal is None


def test_pipeline_runs_the_filter_on_the_linear_mosaic(td, dev):
    from torch_darktable import tonemap
    from torch_darktable.pipeline.util import lerp

    w, h = 96, 64
    frames = _packed_frames(td, dev, w, h)
    m = td.NoiseModel.from_values(0.0, 1.6e-5, dev)
    make = lambda: td.TemporalDenoise(dev, (w, h), td.BayerPattern.RGGB, m, max_frames=8.0)
    piped = _processor(td, dev, w, h, temporal=make())
    plain = _processor(td, dev, w, h)
    c, by_hand = _processor(td, dev, w, h), make()
    bounds = metrics = None
    for f, packed in enumerate(frames):
        out = piped.process(packed, 'cam')
        # the same public operators, one by one
        mosaic = by_hand.process(c.load_bytes(packed), key='cam')
        rgb = c._demosaic(td.apply_white_balance(mosaic, c.white_balance, td.BayerPattern.RGGB)).to(c.storage_dtype)
        assert torch.equal(piped.load_image(packed, f'first {f}'), c._demosaic(td.apply_white_balance(c.load_bytes(packed), c.white_balance, td.BayerPattern.RGGB)))
        now = tonemap.compute_image_bounds([rgb], stride=8)
        bounds = lerp(bounds if bounds is not None else now, now, 0.3)
        acc = tonemap.MetricsAccumulator(dev, stride=8)
        rgb = c.process_rgb(rgb, bounds, acc)
        now = acc.finish()
        metrics = lerp(metrics if metrics is not None else now, now, 0.3)
        assert torch.equal(out, c.tonemap(rgb, metrics)), f
        same = torch.equal(out, plain.process(packed, 'cam'))
        assert same == (f == 0)   # the first frame passes through; the second is averaged with it
    acc_plane, cnt = piped.temporal.state('cam')
    assert float((cnt > 1).float().mean()) > 0.9
