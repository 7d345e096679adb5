"""GPU: the reduced-size demosaic (include/tdk_hip_scaled.h, csrc/scaled_demosaic.hip, torch_darktable.ScaledDemosaic) against
tests/scaled_demosaic_spec.py, the float32 restatement of the header, and ImageProcessor.preview against the chain composed by hand.
Every comparison is on raw bits (all NaNs count as one pattern: which NaN an operation returns is not specified).

Geometry: the smallest frames, the ratios exactly 2 and exactly 16, fractional ratios, a different ratio per axis, and output sizes
T - 1, T, T + 1 and 2 T + 1 of the kernel's tile T on both axes at ratio 2 and at a fractional one; the largest source has 0.04 MP."""

import ctypes
import functools

import numpy as np
import pytest
import torch

import pipeline_stack as stack
import scaled_demosaic_spec as spec

pytestmark = pytest.mark.gpu

f32, f16 = np.float32, np.float16
GAINS = np.array([1.9, 1.0, 1.6], dtype=f32)
SMALL = [((2, 2), (1, 1)), ((4, 4), (2, 2)), ((7, 5), (3, 2)), ((64, 32), (4, 2)), ((37, 22), (13, 9)), ((33, 17), (16, 8)), ((40, 66), (20, 5)),
         ((23, 3), (2, 1))]   # (W, H) -> (w, h)
KINDS = ('f32', 'f16', 'p12', 'p12ids')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a visible MI355X'
    return torch.device('cuda', 0)


def boundary(ratio, kx, ky):
    """((W, H), (w, h)) whose output is the tile's T + k per axis (k = 'double': 2 T + 1) at about `ratio`; the tile follows from the sizes,
    so the sizes are iterated to their fixed point."""
    tw, th = 64, 30
    for _ in range(6):
        ow, oh = (2 * tw + 1 if kx == 'double' else tw + kx), (2 * th + 1 if ky == 'double' else th + ky)
        w, h = int(ow * ratio) + (ratio != int(ratio)), int(oh * ratio) + (ratio != int(ratio))
        tw, th = spec.tile(w, h, ow, oh)
    return (w, h), (ow, oh)


# several tiles with rows of whole 16-byte segments in every source kind; the widest footprints of a 32-column and of a 64-column tile
WIDE = [((288, 70), (130, 33)), ((544, 32), (34, 2)), ((1024, 16), (128, 2)), ((64, 32), (4, 2))]
EDGES = [(-1, -1), (0, 0), (1, 1), ('double', 'double'), (1, -1)]
BOUNDARIES = [boundary(r, kx, ky) for r in (2, 2.6) for kx, ky in EDGES]


def test_boundary_cases_sit_on_the_tile(td, dev):
    for ((w, h), (ow, oh)), (r, (kx, ky)) in zip(BOUNDARIES, [(r, e) for r in (2, 2.6) for e in EDGES]):
        tw, th = spec.tile(w, h, ow, oh)
        assert td.ScaledDemosaic(dev, (w, h), td.BayerPattern.RGGB, (ow, oh)).tile == (tw, th)
        assert ow == (2 * tw + 1 if kx == 'double' else tw + kx) and oh == (2 * th + 1 if ky == 'double' else th + ky), (w, h, ow, oh, tw, th)
        assert w * h < 300_000 and 2 * ow <= w <= 16 * ow and 2 * oh <= h <= 16 * oh
    for (w, h), (ow, oh) in SMALL + WIDE:
        assert td.ScaledDemosaic(dev, (w, h), td.BayerPattern.RGGB, (ow, oh)).tile == spec.tile(w, h, ow, oh)
    assert spec.tile(64, 32, 4, 2) == (32, 6) and spec.tile(4096, 3072, 2048, 1536) == (64, 30) and spec.tile(4096, 3072, 1024, 768) == (64, 14)
    assert td.ScaledDemosaic(dev, (4096, 3072), td.BayerPattern.RGGB, (1024, 768)).lds_bytes() == spec.LDS_BYTES


# ---- content and the restatement, computed once per case
@functools.lru_cache(maxsize=None)
def codes(w, h, seed=0):
    rng = np.random.default_rng(1000 * w + h + seed)
    c = rng.integers(0, 4096, (h, w))
    c[:: 5, :: 3] = 4095
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def samples(kind, w, h, seed=0):
    """The float32 value of every site as the kernel takes it, before gains: 12-bit codes over 4095 for every kind (exact in none of the
    float kinds: binary16 rounds them), and values up to 2 for the float kinds, which nothing clamps without gains."""
    x = codes(w, h, seed).astype(f32) * (f32(1.0) / f32(4095.0))
    if kind in ('f32', 'f16'):
        x = (x * f32(2.0)).astype(f32) if seed % 2 == 0 else x
        x = x.astype(f16).astype(f32) if kind == 'f16' else x
    x.setflags(write=False)
    return x


def source(dev, kind, w, h, seed=0):
    """The device tensor of a case: the (H, W) mosaic, or the packed bytes."""
    if kind in ('p12', 'p12ids'):
        return torch.from_numpy(spec.encode12(codes(w, h, seed), kind == 'p12ids')).to(dev)
    return torch.from_numpy(samples(kind, w, h, seed).astype(f16 if kind == 'f16' else f32)).to(dev)


@functools.lru_cache(maxsize=None)
def want(kind, w, h, ow, oh, pattern, gains, out, seed=0):
    r = spec.scaled_demosaic(samples(kind, w, h, seed), ow, oh, spec.PATTERNS[pattern], gains=GAINS if gains else None,
                             out_dtype={'f32': f32, 'f16': f16}[out], half_source=kind == 'f16')
    r.setflags(write=False)
    return r


def run(td, dev, kind, w, h, ow, oh, pattern, gains, out, seed=0):
    stage = td.ScaledDemosaic(dev, (w, h), td.BayerPattern[pattern], (ow, oh))
    g = torch.from_numpy(GAINS).to(dev) if gains else None
    dtype = {'f32': torch.float32, 'f16': torch.float16}[out]
    x = source(dev, kind, w, h, seed)
    if kind in ('p12', 'p12ids'):
        return stage.process_packed(x, td.PackedFormat.Packed12_IDS if kind == 'p12ids' else td.PackedFormat.Packed12, g, dtype)
    return stage.process(x, g, dtype)


def same_bits(got, expected, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == expected.dtype and got.shape == expected.shape, (what, got.dtype, expected.dtype, got.shape, expected.shape)
    bad = np.argwhere(stack.bits(got) != stack.bits(expected))
    if len(bad):
        print(f'{what}: {len(bad)} of {expected.size} values differ, first at {bad[0]}: got {got[tuple(bad[0])]!r} want {expected[tuple(bad[0])]!r}')
    assert len(bad) == 0, what


# ------------------------------------------------------------------ 1. geometry
@pytest.mark.parametrize('src,dst', SMALL + BOUNDARIES)
def test_geometry(td, dev, src, dst):
    same_bits(run(td, dev, 'f32', *src, *dst, 'RGGB', False, 'f32'), want('f32', *src, *dst, 'RGGB', False, 'f32'), (src, dst))


@pytest.mark.parametrize('src,dst', [BOUNDARIES[3], BOUNDARIES[8]] + WIDE)
@pytest.mark.parametrize('kind', KINDS)
def test_tile_boundaries_in_every_source_kind(td, dev, src, dst, kind):
    """Sources whose rows start on 16 bytes (the segment path: WIDE, where a tile's first column lies inside a segment and the staged
    row is as long as it gets) and whose rows do not (the element path), by the width."""
    if kind.startswith('p12') and src[0] % 2:
        src = (src[0] + 1, src[1])
    same_bits(run(td, dev, kind, *src, *dst, 'GRBG', True, 'f32'), want(kind, *src, *dst, 'GRBG', True, 'f32'), (src, dst, kind))


# ------------------------------------------------------------------ 2. inputs and outputs
@pytest.mark.parametrize('src,dst', [((38, 22), (13, 9)), ((96, 40), (37, 11))])   # rows of 57 / 144 packed bytes: element path / segment path
@pytest.mark.parametrize('pattern', list(spec.PATTERNS))
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('out', ['f32', 'f16'])
@pytest.mark.parametrize('gains', [False, True])
def test_patterns_sources_outputs_gains(td, dev, src, dst, pattern, kind, out, gains):
    x = samples(kind, *src)
    assert not gains or ((x * GAINS.max() > 1).any() and (x * GAINS.max() < 1).any())   # x*g crosses 1 inside every footprint's reach
    same_bits(run(td, dev, kind, *src, *dst, pattern, gains, out), want(kind, *src, *dst, pattern, gains, out), (src, dst, pattern, kind, out, gains))


# ------------------------------------------------------------------ 3. addressing
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('out', ['f32', 'f16'])
def test_odd_element_offsets_take_the_element_path(td, dev, kind, out):
    from torch_darktable._native import lib

    (w, h), (ow, oh) = (96, 40), (37, 11)
    x = source(dev, kind, w, h)
    result = {}
    for off_src, off_dst in ((0, 0), (1, 3), (3, 1)):
        src = torch.zeros(x.numel() + 8, dtype=x.dtype, device=dev)
        src[off_src: off_src + x.numel()] = x.reshape(-1)
        dst = torch.full((ow * oh * 3 + 8,), -7.0, dtype={'f32': torch.float32, 'f16': torch.float16}[out], device=dev)
        sp, dp = src.data_ptr() + off_src * src.element_size(), dst.data_ptr() + off_dst * dst.element_size()
        g = torch.from_numpy(GAINS).to(dev)
        stream = torch.cuda.current_stream().cuda_stream
        tag = {'f32': 0, 'f16': 1}
        if kind.startswith('p12'):
            rc = lib.tdk_decode12_demosaic_scaled(sp, dp, g.data_ptr(), w, h, ow, oh, spec.GBRG, int(kind == 'p12ids'), tag[out], stream)
        else:
            rc = lib.tdk_demosaic_scaled(sp, dp, g.data_ptr(), w, h, ow, oh, spec.GBRG, tag[kind], tag[out], stream)
        assert rc == 0, lib.tdk_last_error()
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        assert (got[:off_dst] == -7).all() and (got[off_dst + ow * oh * 3:] == -7).all()   # nothing beside the frame is written
        result[off_src, off_dst] = got[off_dst: off_dst + ow * oh * 3].reshape(oh, ow, 3)
    for key, got in result.items():
        same_bits(got, want(kind, w, h, ow, oh, 'GBRG', True, out), (kind, out, key))


# ------------------------------------------------------------------ 4. identities
def test_pattern_swap_on_the_device(td, dev):
    (w, h), (ow, oh) = (96, 40), (37, 11)
    for a, b in (('RGGB', 'BGGR'), ('GRBG', 'GBRG')):
        u, v = run(td, dev, 'f32', w, h, ow, oh, a, False, 'f32').cpu().numpy(), run(td, dev, 'f32', w, h, ow, oh, b, False, 'f32').cpu().numpy()
        same_bits(u[..., ::-1].copy(), v, (a, b))


@pytest.mark.parametrize('src,dst', [((38, 22), (13, 9)), ((96, 40), (37, 11))])
def test_fused_forms_equal_the_two_step_calls(td, dev, src, dst):
    g = torch.from_numpy(GAINS).to(dev)
    stage = td.ScaledDemosaic(dev, src, td.BayerPattern.GRBG, dst)
    for ids, fmt in ((False, td.PackedFormat.Packed12), (True, td.PackedFormat.Packed12_IDS)):
        packed = source(dev, 'p12ids' if ids else 'p12', *src)
        mosaic = td.decode12_float(packed, ids_format=ids).view(src[1], src[0])
        for out in (torch.float32, torch.float16):
            assert torch.equal(stage.process_packed(packed, fmt, None, out), stage.process(mosaic, None, out))
            assert torch.equal(stage.process_packed(packed, fmt, g, out), stage.process(td.apply_white_balance(mosaic, g, td.BayerPattern.GRBG), None, out))
    for kind in ('f32', 'f16'):
        mosaic = source(dev, kind, *src)
        balanced = td.apply_white_balance(mosaic, g, td.BayerPattern.GRBG)
        assert balanced.dtype == mosaic.dtype
        assert torch.equal(stage.process(mosaic, g), stage.process(balanced))
        assert stage.process(mosaic, g).dtype == mosaic.dtype and stage.process(mosaic.unsqueeze(-1)).shape == (dst[1], dst[0], 3)


# ------------------------------------------------------------------ 5. streams and graphs
def test_streams_and_two_at_once(td, dev):
    (w, h), (ow, oh) = BOUNDARIES[3]
    first, second = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    stage = td.ScaledDemosaic(dev, (w, h), td.BayerPattern.RGGB, (ow, oh))
    x32, x16 = source(dev, 'f32', w, h), source(dev, 'f16', w, h)
    g = torch.from_numpy(GAINS).to(dev)
    torch.cuda.synchronize()
    outs = []
    for _ in range(4):
        with torch.cuda.stream(first):
            a = stage.process(x32)
        with torch.cuda.stream(second):
            b = stage.process(x16, g, torch.float32)
        outs.append((a, b))
    first.synchronize()
    second.synchronize()
    for a, b in outs:
        same_bits(a, want('f32', w, h, ow, oh, 'RGGB', False, 'f32'), 'first stream')
        same_bits(b, want('f16', w, h, ow, oh, 'RGGB', True, 'f32'), 'second stream')


def test_graph_follows_rewritten_samples_and_gains(td, dev):
    """Captured without a warm-up call (the stage owns no buffer and reads the gains on the device)."""
    (w, h), (ow, oh) = (96, 40), (37, 11)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        stage = td.ScaledDemosaic(dev, (w, h), td.BayerPattern.BGGR, (ow, oh))
        buffer, gains = source(dev, 'f32', w, h).clone(), torch.from_numpy(GAINS).to(dev)
        with torch.cuda.graph(graph, stream=stream):
            captured = stage.process(buffer, gains)
        for seed, g in ((1, (1.2, 1.0, 2.5)), (0, (1.9, 1.0, 1.6)), (1, (1.9, 1.0, 1.6))):
            buffer.copy_(source(dev, 'f32', w, h, seed))
            gains.copy_(torch.tensor(g, dtype=torch.float32))
            graph.replay()
            stream.synchronize()
            expected = spec.scaled_demosaic(samples('f32', w, h, seed), ow, oh, spec.BGGR, gains=np.array(g, dtype=f32))
            same_bits(captured, expected, ('replay', seed, g))


# ------------------------------------------------------------------ 6. special samples
@pytest.mark.parametrize('kind', ['f32', 'f16'])
@pytest.mark.parametrize('bad', [np.nan, np.inf, -np.inf, 65504.0])
def test_special_samples_at_single_sites(td, dev, kind, bad):
    (w, h), (ow, oh) = (37, 22), (13, 9)
    x = samples(kind, w, h).copy()
    for sy, sx in ((0, 0), (7, 12), (8, 13), (21, 36)):
        x[sy, sx] = bad
    stage = td.ScaledDemosaic(dev, (w, h), td.BayerPattern.RGGB, (ow, oh))
    t = torch.from_numpy(x.astype(f16 if kind == 'f16' else f32)).to(dev)
    expected = spec.scaled_demosaic(x, ow, oh, spec.RGGB)
    assert np.isfinite(expected).any() and (not np.isfinite(bad)) == (not np.isfinite(expected).all())
    same_bits(stage.process(t, None, torch.float32), expected, (kind, bad, 'no gains'))
    same_bits(stage.process(t, torch.from_numpy(GAINS).to(dev), torch.float32),
              spec.scaled_demosaic(x, ow, oh, spec.RGGB, gains=GAINS, half_source=kind == 'f16'), (kind, bad, 'gains'))   # the clamp takes them: NaN -> 0


# ------------------------------------------------------------------ 7. the pipeline
PREVIEW = (48, 36)
BRANCHES = {'plain': (), 'raw_correction': ('raw_correction',), 'highlights': ('highlights',), 'chromatic': ('chromatic',), 'temporal': ('temporal',)}


def reduced_processor(td, dev, storage):
    from torch_darktable.pipeline import ImageProcessor, ImageTransform
    return ImageProcessor(PREVIEW, td.BayerPattern[stack.PATTERN], td.PackedFormat.Packed12, stack.settings(0), dev, None,
                          transforms={n: ImageTransform[t] for n, t in stack.TRANSFORMS.items()}, storage_dtype=getattr(torch, storage))


@pytest.mark.parametrize('branch', list(BRANCHES))
@pytest.mark.parametrize('storage', ['float32', 'float16'])
def test_process_preview_is_the_composition_by_hand(td, dev, branch, storage):
    names = BRANCHES[branch]
    padding = stack.PADDING if 'raw_correction' in names else 0
    p = stack.processor(td, dev, {n: stack.stage(td, dev, n) for n in names}, storage=storage, padding=padding)
    p.preview = td.ScaledDemosaic(dev, (stack.W, stack.H), td.BayerPattern[stack.PATTERN], PREVIEW)
    mine = {n: stack.stage(td, dev, n) for n in names}   # other instances: temporal keeps history
    sd = td.ScaledDemosaic(dev, (stack.W, stack.H), td.BayerPattern[stack.PATTERN], PREVIEW)
    reduced = reduced_processor(td, dev, storage)
    gains, pattern = torch.tensor(stack.GAINS, dtype=torch.float32, device=dev), td.BayerPattern[stack.PATTERN]
    for call in range(2):   # the second call: the moving averages of the preview's bounds and metrics, the temporal history of one key
        for name in stack.NAMES:
            data = torch.from_numpy(stack.payload(stack.codes(name, call), padding)).to(dev)
            got = p.process_preview(data, name)
            body = data[: data.numel() - padding] if padding else data
            if 'raw_correction' in names:
                mosaic = mine['raw_correction'].process_packed(body, td.PackedFormat.Packed12, white_balance=gains)
            else:
                mosaic = td.decode12_float(body).view(stack.H, stack.W)
                if 'temporal' in names:
                    mosaic = mine['temporal'].process(mosaic, key=name)
                if 'chromatic' in names:
                    mosaic = mine['chromatic'].correct(mosaic)
                mosaic = mine['highlights'].process(mosaic, gains) if 'highlights' in names else td.apply_white_balance(mosaic, gains, pattern)
            frame = sd.process(mosaic, None, getattr(torch, storage))
            by_hand = reduced._process_frames([name], [frame], resized=False)[name]
            assert got.dtype == torch.uint8 and got.shape == by_hand.shape and got.numel() == PREVIEW[0] * PREVIEW[1] * 3
            assert torch.equal(got, by_hand), (branch, storage, call, name)
    assert torch.equal(p.preview_processor.bounds, reduced.bounds) and torch.equal(p.preview_processor.metrics, reduced.metrics)
    assert p.bounds is None and p.metrics is None   # the full-size processor's are not touched


def test_existing_methods_do_not_see_the_preview(td, dev):
    plain = stack.processor(td, dev, {})
    with_preview = stack.processor(td, dev, {})
    with_preview.preview = td.ScaledDemosaic(dev, (stack.W, stack.H), td.BayerPattern[stack.PATTERN], PREVIEW)
    for call in range(2):
        data = {n: torch.from_numpy(stack.payload(stack.codes(n, call))).to(dev) for n in stack.NAMES}
        a, b = plain.process_image_set(data), with_preview.process_image_set(data)
        bounds, metrics = with_preview.bounds.clone(), with_preview.metrics.clone()
        small = with_preview.process_image_set_preview(data)
        assert torch.equal(with_preview.bounds, bounds) and torch.equal(with_preview.metrics, metrics)
        assert torch.equal(plain.bounds, bounds) and torch.equal(plain.metrics, metrics)
        c, d = plain.process_image_set_resized(data), with_preview.process_image_set_resized(data)
        for n in stack.NAMES:
            assert torch.equal(a[n], b[n]) and torch.equal(c[n], d[n]) and small[n].numel() == PREVIEW[0] * PREVIEW[1] * 3
        assert torch.equal(plain.process(data['left'], 'left'), with_preview.process(data['left'], 'left'))
        assert torch.equal(plain.process_resized(data['left'], 'left'), with_preview.process_resized(data['left'], 'left'))
    with pytest.raises(ValueError, match='process_preview needs preview'):
        plain.process_preview(data['left'], 'left')


def test_setter_and_settings(td, dev):
    p = stack.processor(td, dev, {'color': stack.stage(td, dev, 'color'), 'look': stack.stage(td, dev, 'look'), 'filmic': stack.stage(td, dev, 'filmic')},
                        storage='float16')
    assert p.preview is None and p.preview_processor is None
    pattern = td.BayerPattern[stack.PATTERN]
    with pytest.raises(TypeError, match='preview must be a ScaledDemosaic or None'):
        p.preview = td.Resize(dev, (stack.W, stack.H), PREVIEW)
    with pytest.raises(ValueError, match=f'preview is for 64x48, the processor for {stack.W}x{stack.H}'):
        p.preview = td.ScaledDemosaic(dev, (64, 48), pattern, (32, 24))
    with pytest.raises(ValueError, match='preview is for GBRG, the processor for RGGB'):
        p.preview = td.ScaledDemosaic(dev, (stack.W, stack.H), td.BayerPattern.GBRG, PREVIEW)
    assert p.preview is None and p.preview_processor is None
    stage = td.ScaledDemosaic(dev, (stack.W, stack.H), pattern, PREVIEW)
    p.preview = stage
    q = p.preview_processor
    assert p.preview is stage and tuple(q.image_size) == PREVIEW and q.bayer_pattern == pattern and q.packed_format == p.packed_format and q.device == p.device
    assert q.storage_dtype == torch.float16 and q.transforms == p.transforms and q.white_balance is None
    assert q.settings == p.settings.model_copy(update={'resize_width': 0}) and p.settings.resize_width == stack.RESIZE_WIDTH and q.resize_workspace is None
    assert q.color is p.color and q.look is p.look and q.filmic is p.filmic and q.preview is None
    assert q.chroma_denoise is None and q.defringe is None and q.dehaze is None and q.sharpen is None
    changed = p.settings.model_copy(update={'tone_gamma': 0.7, 'bil_sigma_spatial': p.settings.bil_sigma_spatial * 1.5})
    old_bilateral = q.bil_workspace
    p.update_settings(changed)
    assert q.settings == changed.model_copy(update={'resize_width': 0}) and q.bil_workspace is not old_bilateral and p.preview_processor is q
    p.preview = None
    assert p.preview is None and p.preview_processor is None
