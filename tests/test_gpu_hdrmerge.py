"""GPU: the exposure-bracket merge (torch_darktable.HdrMerge, include/tdk_hip_hdr.h) against the NumPy restatement of the
specification, tests/hdrmerge_spec.py (held to literal loops and to the algorithm's purpose in tests/test_hdrmerge_spec.py).

Every bit of the output and every byte of the mask must be the restatement's: there is no tolerance anywhere in this file and no site
is excluded.  Shapes are sized by the tile of a workgroup and are the smallest that reach the paths: one cell, a window wider than the
frame, one whole tile, one site past a tile in both axes, and aprons that cross two seams."""
import numpy as np
import pytest
import torch

import hdrmerge_spec as spec

pytestmark = pytest.mark.gpu

F = np.float32
PATTERNS = {'RGGB': spec.RGGB, 'BGGR': spec.BGGR, 'GRBG': spec.GRBG, 'GBRG': spec.GBRG}
TORCH = {np.float32: torch.float32, np.float16: torch.float16}
A, B = 3e-4, 2e-6
MODEL = np.array([[3e-4, 2e-6, 1, 20], [2e-4, 1e-6, 1, 20], [5e-4, 3e-6, 1, 20]], F)
# unsorted, with a tie at the longest and at the shortest exposure; whole stops, whose ratios are powers of two (the kernel multiplies by the
# exact reciprocal of such a ratio) ...
EXPOSURES = {2: (0.25, 1.0), 3: (0.25, 1.0, 1 / 16), 8: (1 / 8, 1.0, 0.5, 1 / 64, 0.25, 1.0, 1 / 32, 1 / 64)}
# ... and shutter times as a camera has them: no ratio is a power of two, or only some are (the kernel divides)
SHUTTER = {2: (1 / 30, 1 / 125), 3: (1 / 500, 1 / 30, 1 / 125), 8: (1 / 60, 1 / 30, 1 / 125, 1 / 1000, 1 / 250, 1 / 30, 1 / 500, 1 / 1000), 4: (0.3, 1.2, 0.6, 0.1)}
KINDS = ('noise', 'clipped', 'blown', 'moved', 'special')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a visible MI355X'
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def tile(td):
    assert td.HdrMerge.TILE == spec.TILE
    return td.HdrMerge.TILE   # (TW, TH)


def sizes(tile):
    tw, th = tile
    return [(2, 2), (6, 4), (tw, th), (tw + 2, th + 2), (2 * tw + 6, th - 2), (3 * tw - 2, 2 * th + 2)]   # (w, h)


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


def bracket(w, h, exposures, dtype=np.float32, kinds=KINDS, seed=0, tile=spec.TILE):
    """The frames of one bracket: a ramp with signal-dependent noise, the sensor saturating at 1.  'clipped': a patch that only the
    longer frames clip, its 3 x 3 rim across the first tile seam in both axes; 'blown': a patch every frame clips; 'moved': a rectangle
    that half of the frames have; 'special': single NaN, +inf, -inf, negative and zero samples in several frames."""
    tw, th = tile
    rng = np.random.default_rng(1000 * h + w + seed)
    yy, xx = np.mgrid[0:h, 0:w]
    scene = 0.02 + 0.7 * (xx / max(w - 1, 1)) * (0.4 + 0.6 * yy / max(h - 1, 1))   # in units of the longest frame
    if 'clipped' in kinds:
        scene[max(th - 6, 0):th, max(tw - 7, 0):tw] = 2.5   # up to the last row and column of the first tile: its rim lies in the three tiles next to it
        scene[h // 2:h // 2 + 3, w // 2:w // 2 + 5] = 6.0
    if 'blown' in kinds:
        scene[h // 4:h // 4 + 4, (3 * w) // 4:(3 * w) // 4 + 3] = 1000.0
    top = max(exposures)
    frames = []
    for f, e in enumerate(exposures):
        s = scene.copy()
        if 'moved' in kinds and f % 2 == 1:
            s[h // 3:h // 3 + max(h // 4, 1), w // 5:w // 5 + max(w // 3, 1)] += 0.15
        clean = s * (e / top)
        x = np.minimum(clean + rng.normal(0.0, 1.0, (h, w)) * np.sqrt(A * clean + B), 1.0).astype(dtype)
        if 'special' in kinds:
            flat = x.reshape(-1)
            special = np.array([np.nan, np.inf, -np.inf, -0.25, 0.0], dtype)
            at = rng.choice(flat.size, size=min(flat.size, special.size), replace=False)
            if f % 3 != 2:   # (a frame in three has none)
                flat[at] = special[:at.size]
        frames.append(x)
    return frames


def same(got, got_mask, want, want_mask, what):
    ok = True
    for name, g, w in (('out', got.cpu().numpy(), want), ('mask', got_mask.cpu().numpy() if got_mask is not None else want_mask, want_mask)):
        cmp = bits if name == 'out' else (lambda a: a)
        if g.dtype != w.dtype or g.shape != w.shape or not np.array_equal(cmp(g), cmp(w)):
            bad = np.argwhere(cmp(g) != cmp(w)) if g.shape == w.shape and g.dtype == w.dtype else []
            print(f'{what}: {name} differs at {len(bad)} sites, first {[tuple(b) for b in bad[:6]]}: got {[g[tuple(b)] for b in bad[:6]]}, want {[w[tuple(b)] for b in bad[:6]]}')
            ok = False
    return ok


def run(td, dev, w, h, nf=3, pattern='RGGB', model=MODEL, src=np.float32, out=None, ref=None, kinds=KINDS, offsets=(1, 0, 3), stacked=False, seed=0, what='',
        exposures=EXPOSURES, **kw):
    """One merge against the restatement, with and without the mask."""
    exposures = exposures[nf]
    frames = bracket(w, h, exposures, src, kinds, seed, td.HdrMerge.TILE)
    m = td.NoiseModel(torch.from_numpy(np.asarray(model, F)).to(dev))
    merge = td.HdrMerge(dev, (w, h), td.BayerPattern[pattern], m, **kw)
    if stacked:
        device_frames = upload(np.stack(frames), dev, offsets[0])
    else:
        device_frames = [upload(x, dev, offsets[f % len(offsets)]) for f, x in enumerate(frames)]
    out_dtype = None if out is None else TORCH[out]
    got, got_mask = merge.process(device_frames, exposures, ref=ref, out_dtype=out_dtype, return_mask=True)
    alone = merge.process(device_frames, exposures, ref=ref, out_dtype=out_dtype)
    torch.cuda.synchronize()
    want, want_mask = spec.merge(frames, exposures, model, PATTERNS[pattern], ref=-1 if ref is None else ref, out_dtype=out, **kw)
    what = f'{what} {w}x{h} F={nf} ref={ref}'
    ok = same(got, got_mask, want, want_mask, what)
    return same(alone, None, want, want_mask, what + ' (mask=NULL)') and ok


# ------------------------------------------------------------------ 1. geometry
@pytest.mark.parametrize('radius', [2, 3])
@pytest.mark.parametrize('which', range(6))
def test_every_size_at_both_radii(td, dev, tile, which, radius):
    w, h = sizes(tile)[which]
    ok = run(td, dev, w, h, radius=radius, what=f'radius {radius}')
    ok = run(td, dev, w, h, radius=radius, kinds=('noise',), offsets=(0,), what=f'radius {radius} noise only') and ok
    assert ok


@pytest.mark.parametrize('nf', [2, 3, 8])
def test_every_frame_count_and_anchor(td, dev, tile, nf):
    tw, th = tile
    ok = True
    for w, h in ((tw + 2, th + 2), (3 * tw - 2, 2 * th + 2)):
        for ref in (0, nf // 2, nf - 1, None):
            ok = run(td, dev, w, h, nf=nf, ref=ref, radius=2 + (nf == 8), what='anchor') and ok
    assert ok


@pytest.mark.parametrize('pattern', list(PATTERNS))
def test_every_pattern(td, dev, tile, pattern):
    tw, th = tile
    for radius in (2, 3):
        assert run(td, dev, 2 * tw + 6, th - 2, pattern=pattern, radius=radius, what=pattern)


@pytest.mark.parametrize('src', [np.float32, np.float16], ids=['src32', 'src16'])
@pytest.mark.parametrize('out', [np.float32, np.float16], ids=['out32', 'out16'])
def test_every_combination_of_storage_types(td, dev, tile, src, out):
    tw, th = tile
    ok = True
    for radius, offsets, nf in ((2, (1, 3, 5), 3), (3, (0,), 8)):
        ok = run(td, dev, tw + 2, th + 2, nf=nf, pattern='GRBG', src=src, out=out, radius=radius, offsets=offsets, what=f'{src.__name__}/{out.__name__}') and ok
    assert ok


def test_a_stacked_bracket_one_element_behind_an_allocation(td, dev, tile):
    tw, th = tile
    for src in (np.float32, np.float16):
        assert run(td, dev, 3 * tw - 2, 2 * th + 2, nf=3, src=src, stacked=True, offsets=(1,), what='stacked')


# ------------------------------------------------------------------ 2. inputs and parameters
@pytest.mark.parametrize('kind', KINDS)
def test_every_class_of_input_alone(td, dev, tile, kind):
    tw, th = tile
    ok = True
    for w, h in ((2 * tw + 6, th - 2), (3 * tw - 2, 2 * th + 2)):
        for nf in (3, 8):
            ok = run(td, dev, w, h, nf=nf, kinds=(kind,), seed=7, what=kind) and ok
    assert ok


def test_models_and_parameters(td, dev, tile):
    tw, th = tile
    w, h = 2 * tw + 6, th + 2
    invalid_green = MODEL.copy()
    invalid_green[1, 2] = 0
    no_shot = MODEL.copy()
    no_shot[:, 0] = 0
    nothing = np.array([[0.0, 0.0, 1, 0]] * 3, F)
    all_invalid = np.array([[3e-4, 2e-6, 0, 0]] * 3, F)
    ok = True
    for name, model in (('invalid green', invalid_green), ('a = 0', no_shot), ('a = b = 0', nothing), ('all invalid', all_invalid)):
        ok = run(td, dev, w, h, pattern='GBRG', model=model, what=name) and ok
    for kw in (dict(pixel_threshold=None), dict(thresholds=(0.8, 1.1), pixel_threshold=2.0), dict(variance_floor=1e-5), dict(clip=0.5), dict(clip=2.0)):
        ok = run(td, dev, w, h, what=str(kw), **kw) and ok
    assert ok


@pytest.mark.parametrize('nf', sorted(SHUTTER))
def test_exposures_that_are_no_whole_stops(td, dev, tile, nf):
    tw, th = tile
    ok = True
    for (w, h), src in (((tw + 2, th + 2), np.float32), ((3 * tw - 2, 2 * th + 2), np.float16)):
        for ref, radius in ((None, 2), (nf - 1, 3)):
            ok = run(td, dev, w, h, nf=nf, src=src, ref=ref, radius=radius, exposures=SHUTTER, what='shutter times') and ok
    assert ok


# ------------------------------------------------------------------ 3. graphs
def test_a_captured_call_reads_exposures_and_model_at_every_replay(td, dev, tile):
    tw, th = tile
    w, h = tw + 2, th + 2
    exposures = EXPOSURES[3]
    frames = bracket(w, h, exposures, tile=tile)
    m = td.NoiseModel(torch.from_numpy(MODEL).to(dev))
    merge = td.HdrMerge(dev, (w, h), td.BayerPattern.RGGB, m)
    xs = [upload(x, dev) for x in frames]
    exp = torch.tensor(exposures, dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):   # capturable from the first call: nothing ran before
            out, mask = merge.process(xs, exp, return_mask=True)
    torch.cuda.synchronize()
    other_model = MODEL.copy()
    other_model[:, 0] *= 3
    other_model[2, 2] = 0
    # (three replays: whole stops, other whole stops and another model, then shutter times -- the captured kernel takes the branch of each)
    for new_exposures, model in ((exposures, MODEL), ((1.0, 0.5, 0.125), other_model), ((1 / 30, 1 / 125, 1 / 500), MODEL)):
        exp.copy_(torch.tensor(new_exposures, dtype=torch.float32))
        m.model.copy_(torch.from_numpy(model))
        graph.replay()
        torch.cuda.synchronize()
        want, want_mask = spec.merge(frames, new_exposures, model, spec.RGGB)
        assert same(out, mask, want, want_mask, f'replay with {new_exposures}')
    eager, eager_mask = merge.process(xs, exp, return_mask=True)   # bit-reproducible
    assert torch.equal(eager.view(torch.int32), out.view(torch.int32)) and torch.equal(eager_mask, mask)


# ------------------------------------------------------------------ 4. pipeline
def _processor(td, dev, w, h, **kw):
    from torch_darktable.pipeline import ImageProcessingSettings, ImageProcessor, ImageTransform, ToneMapper
    settings = ImageProcessingSettings(moving_average=0.3, postprocess=False, enable_denoise=True, enable_bilateral=True, tone_mapping=ToneMapper.reinhard)
    return ImageProcessor((w, h), td.BayerPattern.RGGB, td.PackedFormat.Packed12, settings, dev, (1.4, 1.0, 1.3), transforms=ImageTransform.none, **kw)


def _packed_bracket(td, dev, w, h, exposures, sigma=0.004):
    from torch_darktable.synthetic import synthetic_bayer
    base = synthetic_bayer(h, w, seed=104, device='cpu', noise_sigma=0.0) * 3.0 + 0.05   # the longest frame clips most of it
    g = torch.Generator(device='cpu').manual_seed(7)
    return [td.encode12_float((base * e + sigma * torch.randn(base.shape, generator=g)).clamp(0.0, 1.0).to(dev).reshape(-1)) for e in exposures]


def test_process_bracket_is_the_stages_called_by_hand(td, dev):
    from torch_darktable import tonemap
    from torch_darktable.pipeline.util import lerp

    w, h = 96, 64
    exposures = (1.0, 0.25, 1 / 16)
    payloads = _packed_bracket(td, dev, w, h, exposures)
    m = td.NoiseModel.from_values(0.0, 1.6e-5, dev)
    make = lambda: td.HdrMerge(dev, (w, h), td.BayerPattern.RGGB, m)
    piped, plain, c, by_hand = _processor(td, dev, w, h, hdr=make()), _processor(td, dev, w, h), _processor(td, dev, w, h), make()
    bounds = metrics = None
    for step in range(2):   # the second call: the moving averages of bounds and metrics
        out = piped.process_bracket(payloads, exposures, 'cam')
        merged = by_hand.process([c.load_bytes(p) for p in payloads], exposures)
        rgb = c._demosaic(td.apply_white_balance(merged, c.white_balance, td.BayerPattern.RGGB)).to(c.storage_dtype)
        now = tonemap.compute_image_bounds([rgb], stride=8)
        bounds = lerp(bounds if bounds is not None else now, now, 0.3)
        acc = tonemap.MetricsAccumulator(dev, stride=8)
        rgb = c.process_rgb(rgb, bounds, acc)
        now = acc.finish()
        metrics = lerp(metrics if metrics is not None else now, now, 0.3)
        assert out.dtype == torch.uint8 and tuple(out.shape) == (h, w, 3) and torch.equal(out, c.tonemap(rgb, metrics)), step
    # the merge did something: the longest frame alone is clipped where the bracket is not
    assert not torch.equal(out, plain.process(payloads[0], 'cam'))
    # `process` of a processor with the stage is what it is without it
    fresh, with_hdr = _processor(td, dev, w, h), _processor(td, dev, w, h, hdr=make())
    for p in payloads[:2]:
        assert torch.equal(fresh.process(p, 'cam'), with_hdr.process(p, 'cam'))
