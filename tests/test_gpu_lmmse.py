"""GPU: the demosaic for noisy frames (include/tdk_hip_lmmse.h, csrc/lmmse.hip, torch_darktable.LMMSE) against tests/lmmse_spec.py,
the float32 restatement of the specification.  Every comparison is on the raw bits of the frame: no tolerance anywhere.

The geometry comes from LMMSE.TILE (TW x TH) and the apron of 11.  Frames, as (width, height): 2 x 2, 3 x 2, 7 x 5, 12 x 9 (smaller
than the apron on both axes, so indices fold more than once), a tile minus one by a tile plus one, three tiles and an odd remainder on
both axes (corner, edge and interior tiles: the middle tile stages without folding), and a single row of seven tiles and a remainder.
Every frame runs with the four patterns, both domains and the four dtype pairs; the restatement of a case is computed once and
shared."""

import functools

import numpy as np
import pytest
import torch

import lmmse_spec as spec

pytestmark = pytest.mark.gpu

f32, f16 = np.float32, np.float16
TW, TH, APRON = 32, 32, spec.APRON
SHAPES = [(2, 2), (3, 2), (7, 5), (12, 9), (TW - 1, TH + 1), (3 * TW + 5, 3 * TH + 3), (7 * TW + 9, 20)]   # (width, height)
PATTERN_IDS = list(spec.PATTERNS)
DOMAINS = {'sqrt': 0, 'linear': spec.LINEAR}
PAIRS = [(f32, f32), (f32, f16), (f16, f32), (f16, f16)]
TORCH = {f32: torch.float32, f16: torch.float16}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a visible MI355X'
    return torch.device('cuda', 0)


# ---- content
@functools.lru_cache(maxsize=None)
def content(kind, w, h, seed=0):
    rng = np.random.default_rng(w * 7 + h + 1000 * seed)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == 'mixed':      # a random mosaic: a fifth negative, a tenth zero (some of them -0), a tenth above 1 and up to 64
        x = rng.uniform(0.0, 1.0, (h, w))
        pick = rng.random((h, w))
        x = np.where(pick < 0.2, -x, x)
        x = np.where((pick >= 0.2) & (pick < 0.25), 0.0, x)
        x = np.where((pick >= 0.25) & (pick < 0.3), -0.0, x)
        x = np.where(pick >= 0.9, rng.uniform(1.0, 64.0, (h, w)), x)
    elif kind == 'ramp':     # a noisy ramp with a colour cast per CFA site
        x = (0.05 + 0.9 * (xx + 0.5 * yy) / (w + 0.5 * h)) * np.array([[1.0, 0.7], [0.8, 0.5]])[yy % 2, xx % 2] + rng.normal(0.0, 0.01, (h, w))
    elif kind == 'constant':
        x = np.full((h, w), 0.3)
    else:
        raise KeyError(kind)
    x = x.astype(f32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def want(kind, w, h, pattern, flags, src_dtype, dst_dtype, seed=0):
    """The restatement of one case, computed once and shared."""
    out = spec.lmmse(content(kind, w, h, seed).astype(src_dtype), spec.PATTERNS[pattern], flags, dst_dtype)
    out.setflags(write=False)
    return out


def bits(a):
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def same_bits(got, expected, what):
    got = got.cpu().numpy()
    assert got.dtype == expected.dtype and got.shape == expected.shape, (what, got.dtype, expected.dtype, got.shape, expected.shape)
    bad = np.argwhere(bits(got) != bits(expected))
    if len(bad):
        print(f'{what}: {len(bad)} of {expected.size} values differ, first at {bad[0]}: got {got[tuple(bad[0])]!r} want {expected[tuple(bad[0])]!r}')
    assert len(bad) == 0, what


def source(dev, kind, w, h, dtype, seed=0):
    return torch.from_numpy(content(kind, w, h, seed).astype(dtype)).to(dev)


def make(td, dev, w, h, pattern, domain='sqrt'):
    return td.LMMSE(dev, (w, h), td.BayerPattern[pattern], domain=domain)


# ------------------------------------------------------------------ 1. every bit, every geometry
def test_geometry_of_the_table(td):
    assert td.LMMSE.TILE == (TW, TH)
    w, h = SHAPES[5]
    # the middle tile of the 3 x 3 (and a remainder) frame stages its whole apron from inside the frame; the corner tiles fold
    assert TW - APRON >= 0 and 2 * TW + APRON <= w and 2 * TH + APRON <= h and w % TW % 2 == 1 and h % TH % 2 == 1 and -(-w // TW) == 4
    assert SHAPES[3][0] <= APRON + 1 and SHAPES[3][1] < APRON and SHAPES[6][1] < TH and -(-SHAPES[6][0] // TW) == 8


@pytest.mark.parametrize('pair', PAIRS, ids=['f32-f32', 'f32-f16', 'f16-f32', 'f16-f16'])
@pytest.mark.parametrize('domain', list(DOMAINS))
@pytest.mark.parametrize('pattern', PATTERN_IDS)
def test_every_bit_of_the_restatement(td, dev, pattern, domain, pair):
    src_dtype, dst_dtype = pair
    for w, h in SHAPES:
        stage = make(td, dev, w, h, pattern, domain)
        for kind in ('mixed', 'ramp'):
            src = source(dev, kind, w, h, src_dtype)
            out = stage.process(src, out_dtype=TORCH[dst_dtype])
            assert out.is_contiguous() and tuple(out.shape) == (h, w, 3)
            same_bits(out, want(kind, w, h, pattern, DOMAINS[domain], src_dtype, dst_dtype), (kind, w, h, pattern, domain, src_dtype.__name__, dst_dtype.__name__))


@pytest.mark.parametrize('pattern', PATTERN_IDS)
def test_identities_on_the_device(td, dev, pattern):
    """A constant frame comes back in the linear domain; the own colour is the input sample, -0 and negative values included; the
    (H, W, 1) form and the default out_dtype."""
    for w, h in ((2, 2), (TW + 3, 2 * TH + 1)):
        src = source(dev, 'constant', w, h, f32)
        out = make(td, dev, w, h, pattern, 'linear').process(src)
        same_bits(out, np.repeat(content('constant', w, h)[:, :, None], 3, axis=2), ('constant', w, h))
        same_bits(make(td, dev, w, h, pattern, 'sqrt').process(src), want('constant', w, h, pattern, 0, f32, f32), ('constant, sqrt', w, h))
    w, h = 2 * TW + 3, TH + 5
    yy, xx = np.mgrid[0:h, 0:w]
    colour = spec.cfa_color(yy, xx, spec.PATTERNS[pattern])
    for dtype in (f32, f16):
        for domain in DOMAINS:
            src = source(dev, 'mixed', w, h, dtype)
            out = make(td, dev, w, h, pattern, domain).process(src.unsqueeze(-1))
            assert out.dtype == src.dtype
            own = np.take_along_axis(out.cpu().numpy(), colour[:, :, None], axis=2)[:, :, 0]
            assert np.array_equal(bits(own), bits(content('mixed', w, h).astype(dtype)))
            same_bits(out, want('mixed', w, h, pattern, DOMAINS[domain], dtype, dtype), ('(H, W, 1)', domain, dtype.__name__))


def test_flips_on_the_device(td, dev):
    w, h = 2 * TW + 6, TH + 3   # an even width and an odd height: the pattern changes under the horizontal flip only
    src = source(dev, 'mixed', w, h, f32)
    out = make(td, dev, w, h, 'GRBG').process(src)
    name = {v: k for k, v in spec.PATTERNS.items()}
    mirrored = make(td, dev, w, h, name[spec.flip_pattern(spec.GRBG, True, w)]).process(src.flip(1).contiguous())
    assert name[spec.flip_pattern(spec.GRBG, True, w)] == 'RGGB' and torch.equal(mirrored.flip(1).view(torch.int32), out.view(torch.int32))
    upside = make(td, dev, w, h, name[spec.flip_pattern(spec.GRBG, False, h)]).process(src.flip(0).contiguous())
    assert name[spec.flip_pattern(spec.GRBG, False, h)] == 'GRBG' and torch.equal(upside.flip(0).view(torch.int32), out.view(torch.int32))


# ------------------------------------------------------------------ 2. buffers, streams, graphs
@pytest.mark.parametrize('pair', PAIRS, ids=['f32-f32', 'f32-f16', 'f16-f32', 'f16-f16'])
def test_views_offset_by_one_element(td, dev, pair):
    """src and dst one element past an aligned allocation, through the C entry point; a width of whole groups (the aligned case
    stores vectors, this one must not) and one with a tail.  Nothing is written outside dst."""
    from torch_darktable._native import lib

    src_dtype, dst_dtype = pair
    for w, h in ((2 * TW + 4, TH + 1), (TW + 3, 7)):
        for offset in (1, 0):
            n = w * h
            src_pool = torch.zeros(n + 16, dtype=TORCH[src_dtype], device=dev)
            dst_pool = torch.zeros(3 * n + 16, dtype=TORCH[dst_dtype], device=dev)
            assert src_pool.data_ptr() % 256 == 0 and dst_pool.data_ptr() % 256 == 0
            src, dst = src_pool[offset:offset + n], dst_pool[offset:offset + 3 * n]
            src.copy_(source(dev, 'mixed', w, h, src_dtype).reshape(-1))
            rc = lib.tdk_lmmse(src.data_ptr(), dst.data_ptr(), w, h, spec.BGGR, PAIRS.index(pair) // 2, PAIRS.index(pair) % 2, spec.LINEAR,
                               torch.cuda.current_stream().cuda_stream)
            assert rc == 0, lib.tdk_last_error()
            torch.cuda.synchronize()
            same_bits(dst.view(h, w, 3), want('mixed', w, h, 'BGGR', spec.LINEAR, src_dtype, dst_dtype), (w, h, offset))
            assert float(dst_pool[:offset].float().abs().sum()) == 0 and float(dst_pool[offset + 3 * n:].float().abs().max()) == 0   # nothing written outside


def test_non_contiguous_and_wrong_inputs(td, dev):
    stage = make(td, dev, 40, 36, 'RGGB')
    wide = torch.rand((36, 48), device=dev)
    same_bits(stage.process(wide[:, :40]), spec.lmmse(wide[:, :40].cpu().numpy(), spec.RGGB), 'a strided view is copied')
    with pytest.raises(RuntimeError, match='expected'):
        stage.process(wide)
    with pytest.raises(RuntimeError, match='float32 or float16'):
        stage.process(torch.zeros((36, 40), dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError, match='CUDA'):
        stage.process(torch.zeros((36, 40)))


def test_a_side_stream_and_two_streams_at_once(td, dev):
    w, h = SHAPES[5]
    a, b = make(td, dev, w, h, 'RGGB', 'sqrt'), make(td, dev, w, h, 'GBRG', 'linear')
    src = source(dev, 'ramp', w, h, f32)
    s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    for s in (s1, s2):
        s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s1):
        alone = a.process(src)
    s1.synchronize()
    same_bits(alone, want('ramp', w, h, 'RGGB', 0, f32, f32), 'a side stream')
    outs = []
    for _ in range(3):
        with torch.cuda.stream(s1):
            oa = a.process(src)
        with torch.cuda.stream(s2):
            ob = b.process(src)
            oc = a.process(src, out_dtype=torch.float16)   # the same object from the other stream
        outs.append((oa, ob, oc))
    torch.cuda.synchronize()
    for oa, ob, oc in outs:
        same_bits(oa, want('ramp', w, h, 'RGGB', 0, f32, f32), 'first object')
        same_bits(ob, want('ramp', w, h, 'GBRG', spec.LINEAR, f32, f32), 'second object')
        same_bits(oc, want('ramp', w, h, 'RGGB', 0, f32, f16), 'first object on the second stream')


def test_graph_follows_rewritten_samples(td, dev):
    """Captured without a warm-up call (the stage owns no buffer); a replay after the input was rewritten equals the restatement of
    the new mosaic."""
    w, h = 2 * TW + 3, TH + 5
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        stage = make(td, dev, w, h, 'GRBG')
        buffer = source(dev, 'mixed', w, h, f16).clone()
        with torch.cuda.graph(graph, stream=stream):
            captured = stage.process(buffer, out_dtype=torch.float32)
        for seed in (0, 1, 0):
            buffer.copy_(source(dev, 'mixed', w, h, f16, seed))
            graph.replay()
            stream.synchronize()
            same_bits(captured, want('mixed', w, h, 'GRBG', 0, f16, f32, seed=seed), ('replay', seed))
    assert not np.array_equal(want('mixed', w, h, 'GRBG', 0, f16, f32, seed=0), want('mixed', w, h, 'GRBG', 0, f16, f32, seed=1))


# ------------------------------------------------------------------ 3. pipeline
def _processor(td, dev, w, h, postprocess, **kw):
    from torch_darktable.pipeline import Debayer, ImageProcessingSettings, ImageProcessor, ImageTransform, ToneMapper
    settings = ImageProcessingSettings(moving_average=0.3, postprocess=postprocess, color_smoothing_passes=1, enable_denoise=True, enable_bilateral=True,
                                       tone_mapping=ToneMapper.reinhard, debayer=Debayer.rcd)
    return ImageProcessor((w, h), td.BayerPattern.RGGB, td.PackedFormat.Packed12, settings, dev, (1.9, 1.0, 1.6), transforms=ImageTransform.none, **kw)


def _packed(td, dev, w, h):
    scene = np.clip(content('ramp', w, h) * 1.4, 0.0, 1.0)   # some clipped highlights
    return {name: td.encode12_float(torch.from_numpy(np.roll(scene, 2 * k, axis=1).copy()).to(dev).reshape(-1)) for k, name in enumerate(('left', 'right'))}


@pytest.mark.parametrize('with_highlights', [False, True], ids=['wb', 'highlights'])
@pytest.mark.parametrize('postprocess', [False, True], ids=['plain', 'postprocess'])
@pytest.mark.parametrize('storage', [torch.float32, torch.float16], ids=['f32', 'f16'])
def test_pipeline_runs_it_in_place_of_the_named_method(td, dev, storage, postprocess, with_highlights):
    w, h = 128, 96
    packed = _packed(td, dev, w, h)
    stage = td.LMMSE(dev, (w, h), td.BayerPattern.RGGB)
    highlights = td.Highlights(dev, (w, h), td.BayerPattern.RGGB) if with_highlights else None

    with_stage = _processor(td, dev, w, h, postprocess, storage_dtype=storage, highlights=highlights)
    assert with_stage.demosaic is None
    with_stage.demosaic = stage
    assert with_stage.demosaic is stage
    got = with_stage.process_image_set(packed)

    # the chain composed by hand: decode, white balance or highlights, the stage writing the storage type, PostProcess, and on from
    # the frames with a processor that has no such stage
    by_hand = _processor(td, dev, w, h, postprocess, storage_dtype=storage)
    frames = []
    for b in packed.values():
        mosaic = by_hand.load_bytes(b)
        if with_highlights:
            mosaic = highlights.process(mosaic, by_hand.white_balance)
        else:
            mosaic = td.apply_white_balance(mosaic, by_hand.white_balance, by_hand.bayer_pattern)
        rgb = stage.process(mosaic, out_dtype=storage)
        assert rgb.dtype == storage
        frames.append(by_hand.postprocess_workspace.process(rgb) if postprocess else rgb)
    for b, frame in zip(packed.values(), frames):
        loaded = with_stage.load_image(b)
        assert loaded.dtype == storage and torch.equal(loaded, frame)
    expected = by_hand._process_frames(list(packed), frames, resized=False)
    assert sorted(got) == sorted(expected) == ['left', 'right']
    for name in packed:
        assert got[name].dtype == torch.uint8 and torch.equal(got[name], expected[name]), name
    assert torch.equal(with_stage.bounds, by_hand.bounds) and torch.equal(with_stage.metrics, by_hand.metrics)   # they saw the stage's result

    # None: the bits of a processor that never had one, and not the stage's result
    never = _processor(td, dev, w, h, postprocess, storage_dtype=storage, highlights=highlights)
    cleared = _processor(td, dev, w, h, postprocess, storage_dtype=storage, highlights=highlights)
    cleared.demosaic = stage
    cleared.demosaic = None
    for b in packed.values():
        assert torch.equal(cleared.load_image(b), never.load_image(b)) and not torch.equal(with_stage.load_image(b), never.load_image(b))
    first, again = never.process_image_set(packed), cleared.process_image_set(packed)
    for name in packed:
        assert torch.equal(again[name], first[name])
    if not with_highlights:   # ... which is the fused decode + white balance + RCD path, PostProcess behind it
        for b in packed.values():
            rgb = never.rcd_workspace.process_packed(b, never.white_balance, never.packed_format, storage)
            assert torch.equal(never.load_image(b), never.postprocess_workspace.process(rgb) if postprocess else rgb)
