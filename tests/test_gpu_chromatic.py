"""GPU: lateral chromatic aberration (torch_darktable.ChromaticAberration, include/tdk_hip_ca.h) against the NumPy restatement of the
specification, tests/chromatic_spec.py (held to literal loops and to the algorithm's purpose in tests/test_chromatic_spec.py).

Every bit of `correct`, every integer of the workspace and every bit of the model of `estimate` must be the restatement's: there is no
tolerance anywhere in this file and no site is excluded.  Shapes are sized by the tile of a workgroup and by the block of the estimator
and are the smallest that reach the paths: frames smaller than any apron, one tile, two sites past a tile in both axes, sizes that are
no multiple of the tile, partial blocks."""
import numpy as np
import pytest
import torch

import chromatic_spec as spec

pytestmark = pytest.mark.gpu

F = np.float32
TORCH = {np.float32: torch.float32, np.float16: torch.float16}
INTERPS = {'bilinear': spec.BILINEAR, 'bicubic': spec.BICUBIC}
FITS = {'linear': spec.LINEAR, 'poly3': spec.POLY3}
MODELS = {
    'lens': np.array([[1.004, 0.002, -0.001, 1], [0.997, -0.001, 0.002, 1]], F),          # red and blue differ
    'clamped': np.array([[1.3, 0.0, 0.2, 1], [0.6, 0.1, 0.0, 1]], F),                     # the clamp at D acts on part of the frame
    'red only': np.array([[1.02, 0.0, 0.0, 1], [5.0, 1.0, 1.0, 0]], F),                   # valid == 0: the blue row is the identity
    'not finite': np.array([[np.inf, 0.0, 0.0, 1], [1.01, np.nan, 0.0, 1]], F),           # a non-finite displacement is no displacement
}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a visible MI355X'
    return torch.device('cuda', 0)


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


def frame(w, h, dtype=np.float32, seed=0, special=True):
    """A textured mosaic (the planes carry different gains), with single NaN, +inf, -inf, negative and clipped samples."""
    rng = np.random.default_rng(1000 * h + w + seed)
    yy, xx = np.mgrid[0:h, 0:w]
    x = 0.35 + 0.25 * np.sin(0.21 * xx + 0.13 * yy) * np.cos(0.17 * yy - 0.05 * xx) + 0.02 * rng.standard_normal((h, w))
    x *= np.where((yy & 1) == 0, np.where((xx & 1) == 0, 0.5, 1.0), np.where((xx & 1) == 0, 1.0, 0.7))
    if special and w >= 6 and h >= 4:
        for n, value in enumerate((np.nan, np.inf, -np.inf, -0.25, 0.97, 1.5)):
            x[rng.integers(0, h), rng.integers(0, w)] = value
        x[h // 2:h // 2 + 3, w // 3:w // 3 + 4] = 1.0   # a clipped region
    return x.astype(dtype)


def make(td, dev, w, h, pattern='RGGB', **kw):
    return td.ChromaticAberration(dev, (w, h), td.BayerPattern[pattern], **kw)


def check_correct(td, dev, w, h, pattern='RGGB', model='lens', interp='bicubic', src=np.float32, out=None, center=None, rn=None, offset=0, what=''):
    out = src if out is None else out
    x = frame(w, h, src)
    ca = make(td, dev, w, h, pattern, model=torch.from_numpy(MODELS[model]).to(dev), center=center, rn=rn, interp=interp)
    got = ca.correct(upload(x, dev, offset), out_dtype=TORCH[out]).cpu().numpy()
    want = spec.correct(x, spec.PATTERNS[pattern], MODELS[model], ca.center[0], ca.center[1], ca.rn, INTERPS[interp], out)
    same = got.dtype == want.dtype and np.array_equal(bits(got), bits(want))
    if not same:
        bad = np.argwhere(bits(got) != bits(want))
        print(f'{what} {w}x{h} {pattern} {model} {interp} {src.__name__}->{out.__name__}: {len(bad)} sites differ, first {bad[:4].tolist()}')
    return same


def sizes(td):
    tw, th = td.ChromaticAberration.TILE
    assert (tw, th) == spec.TILE
    return [(2, 2), (6, 4), (tw, th), (tw + 2, th + 2), (130, 70), (250, 334)]   # (w, h)


# ------------------------------------------------------------------ 1. correct
@pytest.mark.parametrize('interp', sorted(INTERPS))
def test_correct_frame_sizes(td, dev, interp):
    ok = True
    for w, h in sizes(td):
        for model in ('lens', 'clamped'):
            ok = check_correct(td, dev, w, h, model=model, interp=interp, what='size') and ok
    assert ok


@pytest.mark.parametrize('pattern', sorted(spec.PATTERNS))
def test_correct_patterns_and_storage_types(td, dev, pattern):
    ok = True
    for src in (np.float32, np.float16):
        for out in (np.float32, np.float16):
            for interp in sorted(INTERPS):
                ok = check_correct(td, dev, 130, 70, pattern, 'clamped', interp, src, out, what='storage') and ok
    assert ok


def test_correct_models_centres_and_alignment(td, dev):
    ok = True
    for model in sorted(MODELS):
        for interp in sorted(INTERPS):
            ok = check_correct(td, dev, 66, 34, 'GRBG', model, interp, what='model') and ok
    # a centre far outside the frame, with an rn of its own; the clamp acts everywhere or nowhere
    for center, rn in (((-5000.0, 9000.0), 12000.0), ((40.5, -300.25), 250.0), ((1e30, 0.0), 1.0)):
        ok = check_correct(td, dev, 130, 70, 'BGGR', 'lens', 'bicubic', center=center, rn=rn, what=f'centre {center}') and ok
    # offset views at odd element alignment: the per-element paths of the box and of the store
    for offset in (1, 3):
        for src in (np.float32, np.float16):
            ok = check_correct(td, dev, 130, 70, 'RGGB', 'lens', 'bilinear', src, offset=offset, what=f'offset {offset}') and ok
    assert ok


def test_identity_returns_the_input_bits(td, dev):
    for src in (np.float32, np.float16):
        x = frame(130, 70, src)
        for ca in (td.ChromaticAberration.identity(dev, (130, 70), td.BayerPattern.RGGB), make(td, dev, 130, 70),
                   make(td, dev, 130, 70, model=torch.tensor([[7.0, 1.0, 1.0, 0.0]] * 2, device=dev))):
            got = ca.correct(upload(x, dev)).cpu().numpy()
            assert np.array_equal(got.view(np.uint16 if src == np.float16 else np.uint32), x.view(np.uint16 if src == np.float16 else np.uint32))
    # a single NaN does not spread under the identity, and under a model it reaches only the taps of its own plane
    x = frame(66, 34, special=False)
    x[16, 30] = np.nan
    got = td.ChromaticAberration.identity(dev, (66, 34), td.BayerPattern.RGGB).correct(upload(x, dev)).cpu().numpy()
    assert np.isnan(got).sum() == 1 and np.isnan(got[16, 30])
    moved = make(td, dev, 66, 34, model=torch.from_numpy(MODELS['lens']).to(dev)).correct(upload(x, dev)).cpu().numpy()
    where = np.argwhere(np.isnan(moved))
    assert len(where) >= 1 and all(i % 2 == 0 and j % 2 == 0 and abs(i - 16) <= 6 and abs(j - 30) <= 6 for i, j in where)


def test_correct_on_another_stream_and_captured(td, dev):
    w, h = 130, 70
    x = frame(w, h)
    xs = upload(x, dev)
    model = torch.from_numpy(MODELS['lens']).to(dev)
    ca = make(td, dev, w, h, model=model, interp='bicubic')
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        got = ca.correct(xs)
    stream.synchronize()
    want = spec.correct(x, spec.PATTERNS['RGGB'], MODELS['lens'], *ca.center, ca.rn)
    assert np.array_equal(bits(got.cpu().numpy()), bits(want))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):   # capturable from the first call of this object: nothing of it ran before
            out = make(td, dev, w, h, model=model, interp='bicubic').correct(xs, out_dtype=torch.float16)
    torch.cuda.synchronize()
    for name in ('clamped', 'red only', 'lens'):   # the captured call follows the model tensor as it is at the replay
        model.copy_(torch.from_numpy(MODELS[name]))
        graph.replay()
        torch.cuda.synchronize()
        want = spec.correct(x, spec.PATTERNS['RGGB'], MODELS[name], *ca.center, ca.rn, out_dtype=np.float16)
        assert np.array_equal(bits(out.cpu().numpy()), bits(want)), name


# ------------------------------------------------------------------ 2. estimate
def textured(w, h, s_red, s_blue, dtype=np.float32, seed=0, noise=0.0):
    """Something the estimator can hold on to: smooth texture, red and blue magnified about the centre."""
    rng = np.random.default_rng(seed)
    x0, y0 = (w - 1) / 2, (h - 1) / 2
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    scene = lambda x, y: 0.4 + 0.15 * np.sin(0.19 * x + 0.07 * y) + 0.12 * np.sin(0.05 * x - 0.23 * y) + 0.08 * np.sin(0.31 * x + 0.29 * y)
    m = np.zeros((h, w))
    for gain, s, (oy, ox) in ((0.5, s_red, (0, 0)), (1.0, 1.0, (0, 1)), (1.0, 1.0, (1, 0)), (0.7, s_blue, (1, 1))):
        x, y = xx[oy::2, ox::2], yy[oy::2, ox::2]
        m[oy::2, ox::2] = gain * scene(x0 + (x - x0) / s, y0 + (y - y0) / s)
    m += noise * rng.standard_normal(m.shape)
    return m.astype(dtype)


def check_estimate(td, dev, frames, pattern='RGGB', noise=None, fit='linear', what='', poison=None, **kw):
    h, w = frames[0].shape
    ca = make(td, dev, w, h, pattern)
    block = kw.get('block', 64)
    if poison is not None:   # the workspace of this stream, filled before the call: nothing of it may be read
        ca._workspace(block, dev).fill_(poison)
    noise_model = None if noise is None else td.NoiseModel(torch.from_numpy(noise).to(dev))
    xs = [upload(x, dev) for x in frames]
    got = ca.estimate(xs if len(xs) > 1 else xs[0], noise_model=noise_model, fit=fit, **kw)
    sums = ca.statistics(xs, clip=kw.get('clip', 0.95), block=block).cpu().numpy()
    want, want_sums = spec.estimate(frames, spec.PATTERNS[pattern], ca.center[0], ca.center[1], ca.rn, noise, FITS[fit], kw.get('clip', 0.95), block, kw.get('max_shift', 2.0))
    model = got.model.cpu().numpy()
    same = np.array_equal(sums, want_sums) and np.array_equal(bits(model), bits(want)) and got.center == ca.center and got.rn == ca.rn
    if not same:
        print(f'{what}: sums differ at {np.argwhere(sums != want_sums)[:4].tolist() if sums.shape == want_sums.shape else (sums.shape, want_sums.shape)}\n got {model}\nwant {want}')
    return same, want


NOISE = np.array([[3e-5, 1e-6, 1, 20], [2e-5, 2e-6, 1, 20], [5e-5, 3e-6, 1, 20]], F)


@pytest.mark.parametrize('fit', sorted(FITS))
def test_estimate_frames_noise_models_and_fits(td, dev, fit):
    ok = True
    w, h = 200, 136   # partial blocks on the right and at the bottom
    one = [textured(w, h, 1.01, 0.992, noise=0.004)]
    three = [textured(w, h, 1.01, 0.992, np.float16, seed=s, noise=0.004) for s in range(3)]
    invalid_green = NOISE.copy()
    invalid_green[1, 2] = 0
    for frames, name in ((one, 'one frame'), (three, 'three binary16 frames')):
        for noise in (None, NOISE, invalid_green):
            same, want = check_estimate(td, dev, frames, noise=noise, fit=fit, block=32, what=f'{name} {fit}', poison=0xA5)
            ok = same and ok
            assert want[:, 3].min() == 1, (name, want)   # the case fits something
    for pattern in ('BGGR', 'GBRG'):
        ok = check_estimate(td, dev, one, pattern, NOISE, fit, block=32, what=pattern)[0] and ok
    same, want = check_estimate(td, dev, [textured(256, 192, 1.006, 0.996)], noise=NOISE, fit=fit, what='default block', max_shift=1.5)
    assert same and ok


def test_estimate_special_frames(td, dev):
    ok = True
    w, h = 200, 136
    clipped = textured(w, h, 1.01, 0.992)
    clipped[40:90, 30:120] = 0.99                     # a clipped region
    clipped[100, 150], clipped[7, 9], clipped[8, 9] = np.nan, np.inf, -np.inf
    same, want = check_estimate(td, dev, [clipped], block=32, clip=0.9, what='clipped region', poison=0xFF)
    ok = same and ok and want[:, 3].min() == 1
    for frames, block, name in (([np.full((h, w), 0.3, F)], 32, 'flat'), ([textured(60, 40, 1.01, 0.99)], 64, 'smaller than a block'),
                                ([np.full((h, w), 0.97, F)], 32, 'clipped everywhere'), ([textured(w, h, 1.2, 0.8)], 32, 'beyond max_shift')):
        for fit in sorted(FITS):
            same, want = check_estimate(td, dev, frames, fit=fit, block=block, what=name, poison=0x7F)
            ok = same and ok
            if name != 'beyond max_shift':
                assert np.array_equal(want, np.array([[1, 0, 0, 0]] * 2, F)), name
    assert ok


def test_estimate_captured_and_replayed(td, dev):
    w, h = 200, 136
    first, second = textured(w, h, 1.01, 0.992, noise=0.004), textured(w, h, 0.994, 1.008, seed=5, noise=0.004)
    xs = upload(first, dev)
    noise = td.NoiseModel(torch.from_numpy(NOISE).to(dev))
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ca = make(td, dev, w, h)   # (the workspace of this stream and of block 32 does not exist yet: the capture's pool holds it)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):   # capturable from the first call; estimate -> correct: the model never leaves the device
            fitted = ca.estimate(xs, noise_model=noise, fit='poly3', block=32)
            out = fitted.correct(xs)
    torch.cuda.synchronize()
    for x in (first, second):
        xs.copy_(torch.from_numpy(x))
        graph.replay()
        torch.cuda.synchronize()
        want, _ = spec.estimate([x], spec.PATTERNS['RGGB'], *ca.center, ca.rn, NOISE, spec.POLY3, block=32)
        assert np.array_equal(bits(fitted.model.cpu().numpy()), bits(want))
        assert np.array_equal(bits(out.cpu().numpy()), bits(spec.correct(x, spec.PATTERNS['RGGB'], want, *ca.center, ca.rn, spec.BILINEAR)))
    # refine is the composition it says, on the device coefficients
    refined = ca.refine(xs, fitted, noise_model=noise, block=32).model.cpu().numpy()
    residual, _ = spec.estimate([spec.correct(second, spec.PATTERNS['RGGB'], want, *ca.center, ca.rn, spec.BILINEAR)], spec.PATTERNS['RGGB'], *ca.center, ca.rn, NOISE, block=32)
    expected = want.copy()
    expected[:, :3] += (residual[:, :3] - np.array([1, 0, 0], F)) * residual[:, 3:4]
    assert np.array_equal(bits(refined), bits(expected))


# ------------------------------------------------------------------ 3. pipeline
def _processor(td, dev, w, h, **kw):
    from torch_darktable.pipeline import ImageProcessingSettings, ImageProcessor, ImageTransform, ToneMapper
    settings = ImageProcessingSettings(moving_average=0.3, postprocess=False, enable_denoise=True, enable_bilateral=True, tone_mapping=ToneMapper.reinhard)
    return ImageProcessor((w, h), td.BayerPattern.RGGB, td.PackedFormat.Packed12, settings, dev, (1.4, 1.0, 1.3), transforms=ImageTransform.none, **kw)


def test_pipeline_with_chromatic_is_the_stages_called_by_hand(td, dev):
    from torch_darktable import tonemap
    from torch_darktable.pipeline.util import lerp
    from torch_darktable.synthetic import synthetic_bayer

    w, h = 96, 64
    payload = td.encode12_float(synthetic_bayer(h, w, seed=104, device='cpu', noise_sigma=0.002).clamp(0.0, 1.0).to(dev).reshape(-1))
    model = torch.from_numpy(MODELS['lens'] + np.array([[0.02, 0, 0, 0], [-0.02, 0, 0, 0]], F)).to(dev)
    ca = lambda: td.ChromaticAberration(dev, (w, h), td.BayerPattern.RGGB, model=model)
    piped, plain, c, by_hand = _processor(td, dev, w, h, chromatic=ca()), _processor(td, dev, w, h), _processor(td, dev, w, h), ca()
    hl = td.Highlights(dev, (w, h), td.BayerPattern.RGGB)
    with_hl = _processor(td, dev, w, h, chromatic=ca(), highlights=hl)
    bounds = metrics = None
    for step in range(2):   # the second call: the moving averages of bounds and metrics
        out = piped.process(payload, 'cam')
        mosaic = by_hand.correct(c.load_bytes(payload))
        rgb = c._demosaic(td.apply_white_balance(mosaic, c.white_balance, td.BayerPattern.RGGB)).to(c.storage_dtype)
        now = tonemap.compute_image_bounds([rgb], stride=8)
        bounds = lerp(bounds if bounds is not None else now, now, 0.3)
        acc = tonemap.MetricsAccumulator(dev, stride=8)
        rgb = c.process_rgb(rgb, bounds, acc)
        now = acc.finish()
        metrics = lerp(metrics if metrics is not None else now, now, 0.3)
        assert out.dtype == torch.uint8 and tuple(out.shape) == (h, w, 3) and torch.equal(out, c.tonemap(rgb, metrics)), step
    assert not torch.equal(out, plain.process(payload, 'cam'))   # the stage did something
    # in front of highlights: load_image is the stages by hand
    want = c._demosaic(hl.process(by_hand.correct(c.load_bytes(payload)), c.white_balance)).to(c.storage_dtype)
    assert torch.equal(with_hl.load_image(payload), want)
    # with the identity the unfused path gives what the parent's fused path gives; without the argument the call is the parent's
    same = _processor(td, dev, w, h, chromatic=td.ChromaticAberration.identity(dev, (w, h), td.BayerPattern.RGGB))
    fresh = _processor(td, dev, w, h)
    assert fresh.chromatic is None and torch.equal(same.process(payload, 'cam'), fresh.process(payload, 'cam'))
