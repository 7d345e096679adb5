"""GPU: the capture sharpening (include/tdk_hip_deconv.h, csrc/deconv.hip, torch_darktable.Deconvolve) against tests/deconv_spec.py,
the float32 restatement of the specification.  Every comparison is on the raw bits of the frame and of the mask: no tolerance
anywhere.

The geometry comes from Deconvolve.TILE and fused_iterations (F).  The table is pruned, not a product: per radius 1, 3 and 6 a frame
of one pixel, frames narrower and lower than R and than the apron 2*R*F, a frame one pixel past a tile in each axis, one that
crosses two tile boundaries in both and one of three tiles and a pixel, whose middle tile has its whole apron inside the frame (the
kernel runs its vectorised passes there and the clamping ones in every other tile); N in {1, F, F + 1, 2F + 1}, so that a call is
one launch, whole launches, or ends on a short one; every F that was built, forced, against the same expected bits."""

import ctypes
import functools

import numpy as np
import pytest
import torch

import deconv_spec as spec

pytestmark = pytest.mark.gpu

f32 = np.float32
DTYPES = [np.float32, np.float16]
SIGMAS = {1: 0.3, 3: 0.7, 6: 2.0}          # radius -> a sigma that gives it
BUILT = {1: (1, 2, 4), 3: (1, 2), 6: (1,)}   # radius -> the F that take it
TILE = spec.TILE


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a visible MI355X'
    return torch.device('cuda', 0)


def taps_of(radius):
    taps = spec.gaussian_taps(SIGMAS[radius])
    assert len(taps) == radius + 1
    return taps


def default_fused(radius):
    from torch_darktable._native import lib
    return int(lib.tdk_deconv_fused_iterations(radius))


# ---- content
@functools.lru_cache(maxsize=None)
def content(kind, w, h, channels=3, seed=0):
    rng = np.random.default_rng(w * 7 + h + seed)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == 'chart':   # blocks, a slanted edge and fine stripes, blurred, with a little noise
        sharp = rng.uniform(0.05, 0.9, (-(-h // 5), -(-w // 5), channels)).repeat(5, 0).repeat(5, 1)[:h, :w]
        sharp = sharp * np.where((xx + 2 * yy) % 23 < 11, 1.0, 0.4)[..., None] + 0.1 * ((xx // 2) % 2)[..., None]
        taps = spec.gaussian_taps(0.7)
        x = np.stack([spec.blur(sharp[..., c].astype(f32), taps) for c in range(channels)], axis=-1) + rng.normal(0.0, 0.004, (h, w, channels))
    elif kind == 'zeros':
        x = np.zeros((h, w, channels))
    elif kind == 'constant':
        x = np.ones((h, w, channels)) * np.array([0.4, 0.5, 0.6])[:channels]
    elif kind == 'negative':   # a third of the samples negative, a region that is negative throughout
        x = content('chart', w, h, channels) * np.where(rng.random((h, w, channels)) < 0.3, -1.0, 1.0)
        x[: h // 3] = -np.abs(x[: h // 3])
    elif kind == 'half_max':   # near the largest binary16 value, with dark pixels that make the gain leave 1
        x = rng.uniform(50000.0, 65504.0, (h, w, channels))
        x[rng.random((h, w)) < 0.1] *= 0.01
    elif kind == 'steps':   # vertical bands whose square roots differ by exactly t = 1/64 and 2t, on exact squares
        roots = np.array([0.5, 0.5 + 1 / 64, 0.5 + 3 / 64, 0.5 + 3 / 64, 0.5 + 3 / 64 + 1 / 256])
        x = np.repeat((roots[(xx // 7) % 5] ** 2)[..., None], channels, axis=2)
    else:
        raise KeyError(kind)
    x = x.astype(f32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def want(kind, w, h, channels, dtype, radius, iterations, threshold=0.02, max_gain=4.0, weights=spec.REC709, seed=0):
    """The restatement of one case, computed once and shared: (frame, m)."""
    out, m = spec.process(content(kind, w, h, channels, seed).astype(dtype), taps_of(radius), iterations, threshold, max_gain, weights)
    out.setflags(write=False), m.setflags(write=False)
    return out, m


def bits(a):
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def same_bits(got, expected, what):
    got = got.cpu().numpy()
    assert got.dtype == expected.dtype and got.shape == expected.shape, (what, got.dtype, expected.dtype, got.shape, expected.shape)
    bad = np.argwhere(bits(got) != bits(expected))
    if len(bad):
        print(f'{what}: {len(bad)} of {expected.size} values differ, first at {bad[0]}: got {got[tuple(bad[0])]!r} want {expected[tuple(bad[0])]!r}')
    assert len(bad) == 0, what


def make(td, dev, w, h, radius, iterations, threshold=0.02, max_gain=4.0, weights=None, fused=None):
    d = td.Deconvolve.from_weights(dev, (w, h), taps_of(radius), iterations=iterations, threshold=threshold, max_gain=max_gain, weights=weights)
    d.fused_iterations = fused
    return d


def source(dev, kind, w, h, channels, dtype, seed=0):
    return torch.from_numpy(content(kind, w, h, channels, seed).astype(dtype)).to(dev)


def check_case(td, dev, kind, w, h, channels, dtype, radius, iterations, fused=None, **kw):
    d = make(td, dev, w, h, radius, iterations, fused=fused, **kw)
    src = source(dev, kind, w, h, channels, dtype)
    out, m = d.process(src, return_mask=True)
    assert out.dtype == src.dtype and out.is_contiguous() and out.data_ptr() != src.data_ptr() and m.dtype == torch.float32 and tuple(m.shape) == (h, w)
    out_w, m_w = want(kind, w, h, channels, dtype, radius, iterations, **kw)
    what = (kind, w, h, channels, dtype.__name__, radius, iterations, fused, kw)
    same_bits(m, m_w, (*what, 'mask'))
    same_bits(out, out_w, what)
    return d, src, out, m


def sizes(radius, fused):
    apron = 2 * radius * fused
    return [(1, 1), (max(radius - 1, 1), apron + 5), (apron + 5, max(radius - 1, 1)), (apron - 1, apron - 1), (TILE + 1, TILE), (TILE, TILE + 1),
            (2 * TILE + 3, 2 * TILE + 3), (3 * TILE + 1, 3 * TILE + 1)]


# ------------------------------------------------------------------ 1. geometry
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('radius', [1, 3, 6])
def test_geometry_and_launch_counts_give_the_restatements_bits(td, dev, radius, dtype):
    fused = default_fused(radius)
    assert fused in BUILT[radius]
    for k, (w, h) in enumerate(sizes(radius, fused)):
        for j, iterations in enumerate((1, fused, fused + 1, 2 * fused + 1)):
            channels, threshold = (3, 1)[(k + j) % 2], (0.02, None)[(k + j // 2) % 2]   # both channel counts and both mask settings meet every size
            d, *_ = check_case(td, dev, 'chart', w, h, channels, dtype, radius, iterations, threshold=threshold)
            assert d.launches == -(-iterations // fused) and d.fused_iterations == fused


def test_the_table_meets_its_cases():
    for radius in (1, 3, 6):
        for fused in BUILT[radius]:
            table = sizes(radius, fused)
            assert (1, 1) in table and any(w < radius or radius == 1 for w, _ in table) and any(h < radius or radius == 1 for _, h in table)
            assert any(w < 2 * radius * fused and h < 2 * radius * fused for w, h in table)
            assert any(w == TILE + 1 for w, _ in table) and any(h == TILE + 1 for _, h in table)
            assert any(w > 2 * TILE and h > 2 * TILE for w, h in table)
            assert any(min(w, h) >= 2 * TILE + 2 * radius * fused for w, h in table)   # a tile whose apron lies inside the frame: the kernel's other body
    assert max(BUILT[1]) == spec.MAX_FUSED and BUILT[6] == (1,)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('radius', [1, 3, 6])
def test_every_built_fused_count_gives_the_same_bits(td, dev, radius, dtype):
    """F forced through the flags: one launch, whole launches and a short last one per F, all against the bits the restatement has."""
    w = h = 2 * TILE + 3
    for fused in BUILT[radius]:
        for iterations in sorted({1, fused, fused + 1, 2 * fused + 1}):
            d, *_ = check_case(td, dev, 'chart', w, h, 3, dtype, radius, iterations, fused=fused)
            assert d.fused_iterations == fused and d.launches == -(-iterations // fused)
            check_case(td, dev, 'chart', 3 * TILE + 1, 3 * TILE + 1, 1, dtype, radius, iterations, fused=fused, threshold=None)   # with a tile inside the frame
        check_case(td, dev, 'chart', 2 * radius * fused - 1, 5, 1, dtype, radius, 2 * fused + 1, fused=fused, threshold=None)   # narrower than the apron
        check_case(td, dev, 'chart', TILE + 1, 2 * radius * fused - 1, 3, dtype, radius, fused + 1, fused=fused)                 # lower than it
    d = make(td, dev, w, h, radius, 8)
    for bad in (3, 8, *(f for f in (1, 2, 4) if f not in BUILT[radius])):
        with pytest.raises(ValueError, match='fused_iterations must be'):
            d.fused_iterations = bad


# ------------------------------------------------------------------ 2. parameters and content
@pytest.mark.parametrize('dtype', DTYPES)
def test_parameters_at_their_ends(td, dev, dtype):
    w, h = TILE + 9, TILE + 2
    for kw in (dict(max_gain=1.0), dict(max_gain=16.0), dict(max_gain=1.05), dict(threshold=1e-4), dict(threshold=0.5), dict(weights=(0.25, 0.5, 0.25)),
               dict(weights=(0.0, 1.0, 0.0)), dict(weights=(0.0, 0.0, 0.0))):
        check_case(td, dev, 'chart', w, h, 3, dtype, 3, 5, **kw)
    _, src, out, _ = check_case(td, dev, 'chart', w, h, 3, dtype, 3, 5, max_gain=1.0)
    assert torch.equal(out.view(torch.uint8), src.view(torch.uint8))   # a gain held at 1: the input's bits
    check_case(td, dev, 'chart', w, h, 3, dtype, 1, 50)   # the most iterations


@pytest.mark.parametrize('dtype', DTYPES)
def test_no_iterations_return_the_inputs_bits_and_the_mask(td, dev, dtype):
    for channels in (1, 3):
        for kind in ('chart', 'negative'):
            _, src, out, m = check_case(td, dev, kind, TILE + 1, TILE + 3, channels, dtype, 3, 0)
            assert torch.equal(out.view(torch.uint8), src.view(torch.uint8))
    assert float(m.max()) > 0.0


@pytest.mark.parametrize('dtype', DTYPES)
def test_zeros_constant_and_negative_frames(td, dev, dtype):
    w, h = TILE + 5, TILE + 1
    for channels in (1, 3):
        _, src, out, m = check_case(td, dev, 'zeros', w, h, channels, dtype, 3, 3)
        assert float(out.float().abs().max()) == 0.0 and float(m.max()) == 0.0
        _, src, out, m = check_case(td, dev, 'constant', w, h, channels, dtype, 3, 3)
        assert float(m.max()) == 0.0 and torch.equal(out.view(torch.uint8), src.view(torch.uint8))   # m = 0: the input's bits
        check_case(td, dev, 'constant', w, h, channels, dtype, 3, 3, threshold=None)
        check_case(td, dev, 'negative', w, h, channels, dtype, 3, 3)
        check_case(td, dev, 'negative', w, h, channels, dtype, 6, 2, threshold=None)
    assert (content('negative', w, h) < 0).mean() > 0.3


def test_binary16_values_near_the_largest(td, dev):
    w, h = TILE + 5, TILE + 1
    for channels in (1, 3):
        _, _, out, _ = check_case(td, dev, 'half_max', w, h, channels, np.float16, 3, 4, threshold=None, max_gain=16.0)
        assert torch.isinf(out).any() and not torch.isnan(out).any()   # rounded to infinity, as the restatement has it
    check_case(td, dev, 'half_max', w, h, 3, np.float16, 1, 2)


@pytest.mark.parametrize('dtype', DTYPES)
def test_steps_exactly_at_the_masks_threshold_and_twice_it(td, dev, dtype):
    w, h, t = TILE + 10, 9, 1.0 / 64
    for channels in (1, 3):
        check_case(td, dev, 'steps', w, h, channels, dtype, 3, 3, threshold=t, weights=(0.25, 0.5, 0.25))
    m = want('steps', w, h, 1, np.float32, 3, 3, threshold=t, weights=(0.25, 0.5, 0.25))[1]
    assert (m == 0).any() and (m == 1).any() and m[4, 6] == 0 and m[4, 13] == 1   # a step of t: nothing; of 2t: everything


# ------------------------------------------------------------------ 3. mechanics
def at_offset(t, elements):
    """A contiguous copy of CUDA tensor `t` that starts `elements` elements past an aligned allocation."""
    pool = torch.zeros(t.numel() + elements + 16, dtype=t.dtype, device=t.device)
    assert pool.data_ptr() % 256 == 0
    v = pool[elements:elements + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() == pool.data_ptr() + elements * t.element_size()
    return v


@pytest.mark.parametrize('dtype', DTYPES)
def test_offset_and_non_contiguous_views(td, dev, dtype):
    """A contiguous view at an odd element offset is taken (the accesses go element by element); a non-contiguous one is refused."""
    for (w, h), channels in (((2 * TILE + 4, TILE + 1), 3), ((TILE + 4, TILE + 2), 1), ((TILE + 3, 7), 3)):
        d = make(td, dev, w, h, 3, 5)
        src = source(dev, 'chart', w, h, channels, dtype)
        out_w, m_w = want('chart', w, h, channels, dtype, 3, 5)
        for offset in (0, 1, 2, 3):
            view = at_offset(src, offset)
            out, m = d.process(view, return_mask=True)
            same_bits(out, out_w, (w, h, channels, offset))
            same_bits(m, m_w, (w, h, channels, offset, 'mask'))
    d = make(td, dev, 40, 36, 3, 5)
    wide = torch.zeros((36, 48, 3), dtype=src.dtype, device=dev)
    with pytest.raises(RuntimeError, match='contiguous'):
        d.process(wide[:, :40])
    with pytest.raises(RuntimeError, match='expected'):
        d.process(wide)
    with pytest.raises(ValueError, match='float32 or float16'):
        d.process(torch.zeros((36, 40, 3), dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match='channels must be 1 or 3'):
        d.process(torch.zeros((36, 40, 2), dtype=src.dtype, device=dev))


def test_outputs_at_odd_offsets_through_the_c_entry_point(td, dev):
    from torch_darktable._native import lib

    for (w, h, channels, radius, iterations), dtype, tag in (((2 * TILE + 4, TILE + 1, 3, 3, 5), np.float32, 0), ((TILE + 4, TILE + 2, 1, 1, 9), np.float16, 1)):
        src = source(dev, 'chart', w, h, channels, dtype)
        n = w * h
        pool = torch.zeros(channels * n + 40, dtype=src.dtype, device=dev)
        m_pool = torch.zeros(n + 40, dtype=torch.float32, device=dev)
        out, m = pool[3:3 + channels * n], m_pool[1:1 + n]
        need = int(lib.tdk_deconv_workspace_bytes(w, h, radius, iterations))
        assert need == spec.workspace_bytes(w, h, spec.launches(iterations, default_fused(radius))) > 0
        ws_pool = torch.zeros(need + 16, dtype=torch.uint8, device=dev)
        ws = ws_pool[5:5 + need]
        taps = (ctypes.c_float * (radius + 1))(*taps_of(radius))
        luma = (ctypes.c_float * 3)(*spec.REC709)
        rc = lib.tdk_deconv(src.data_ptr(), out.data_ptr(), m.data_ptr(), ws.data_ptr(), w, h, channels, tag, taps, radius, iterations, 0.02, 4.0, luma, spec.MASK,
                            torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.tdk_last_error()
        torch.cuda.synchronize()
        out_w, m_w = want('chart', w, h, channels, dtype, radius, iterations)
        same_bits(out.view(h, w, channels), out_w, (w, h, 'frame'))
        same_bits(m.view(h, w), m_w, (w, h, 'mask'))
        assert float(pool[:3].float().abs().max()) == 0 and float(pool[3 + channels * n:].float().abs().max()) == 0   # nothing written outside
        assert float(m_pool[:1].abs().max()) == 0 and float(m_pool[1 + n:].abs().max()) == 0
        assert int(ws_pool[:5].max()) == 0 and int(ws_pool[5 + need:].max()) == 0


def test_workspace_filled_with_nan_gives_the_same_bits(td, dev):
    for dtype, (w, h, radius, iterations) in zip(DTYPES, ((2 * TILE + 3, TILE + 3, 3, 7), (TILE + 4, 2 * TILE + 1, 6, 3))):
        d, src, out, m = check_case(td, dev, 'chart', w, h, 3, dtype, radius, iterations)
        assert len(d._workspaces) == 1 and d.launches >= 3 and d.workspace_bytes() == spec.workspace_bytes(w, h, d.launches)
        for buf in d._workspaces._buffers.values():
            assert buf.numel() == d.workspace_bytes()
            buf.fill_(0xFF)   # every float32 a NaN
        again, m_again = d.process(src, return_mask=True)
        assert torch.equal(again.view(torch.uint8), out.view(torch.uint8)) and torch.equal(m_again.view(torch.int32), m.view(torch.int32))
    one = make(td, dev, w, h, 3, default_fused(3))
    assert one.launches == 1 and one.workspace_bytes() == 0


def test_two_objects_on_two_streams_at_once(td, dev):
    w, h = 2 * TILE + 3, 2 * TILE + 3
    a, b = make(td, dev, w, h, 3, 7), make(td, dev, w, h, 1, 9, threshold=None)
    src = source(dev, 'chart', w, h, 3, np.float32)
    s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    for s in (s1, s2):
        s.wait_stream(torch.cuda.current_stream())
    outs = []
    for _ in range(3):
        with torch.cuda.stream(s1):
            oa = a.process(src)
        with torch.cuda.stream(s2):
            ob = b.process(src)
        with torch.cuda.stream(s2):
            oc = a.process(src)   # the same object from the other stream: a workspace of its own
        outs.append((oa, ob, oc))
    torch.cuda.synchronize()
    assert len(a._workspaces) == 3   # the stream of construction and the two
    for oa, ob, oc in outs:
        same_bits(oa, want('chart', w, h, 3, np.float32, 3, 7)[0], 'first object')
        same_bits(ob, want('chart', w, h, 3, np.float32, 1, 9, threshold=None)[0], 'second object')
        same_bits(oc, want('chart', w, h, 3, np.float32, 3, 7)[0], 'first object on the second stream')


def test_graph_follows_rewritten_pixels(td, dev):
    """An object built on the side stream and captured there without a warm-up call (the workspace exists since construction); a
    replay after the input buffer was rewritten equals the restatement of the new frame."""
    w, h = 2 * TILE + 3, TILE + 5
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        d = make(td, dev, w, h, 3, 8)
        assert d.launches == 8 // d.fused_iterations
        buffer = source(dev, 'chart', w, h, 3, np.float16).clone()
        with torch.cuda.graph(graph, stream=stream):
            captured, captured_m = d.process(buffer, return_mask=True)
        for seed in (0, 1, 0):
            buffer.copy_(source(dev, 'chart', w, h, 3, np.float16, seed))
            graph.replay()
            stream.synchronize()
            out_w, m_w = want('chart', w, h, 3, np.float16, 3, 8, seed=seed)
            same_bits(captured, out_w, ('replay', seed))
            same_bits(captured_m, m_w, ('replayed mask', seed))
    assert not np.array_equal(want('chart', w, h, 3, np.float16, 3, 8, seed=0)[0], want('chart', w, h, 3, np.float16, 3, 8, seed=1)[0])


# ------------------------------------------------------------------ 4. pipeline
def _processor(td, dev, w, h, **kw):
    from torch_darktable.pipeline import Debayer, ImageProcessingSettings, ImageProcessor, ImageTransform, ToneMapper
    settings = ImageProcessingSettings(moving_average=0.3, postprocess=False, enable_denoise=True, enable_bilateral=True, tone_mapping=ToneMapper.reinhard,
                                       debayer=Debayer.bilinear)
    return ImageProcessor((w, h), td.BayerPattern.RGGB, td.PackedFormat.Packed12, settings, dev, (1.9, 1.0, 1.6), transforms=ImageTransform.none, **kw)


@pytest.mark.parametrize('storage', [torch.float32, torch.float16])
def test_pipeline_runs_it_in_front_of_color(td, dev, storage):
    w, h = 128, 96
    scene = content('chart', w, h)[..., 1]
    packed = {name: td.encode12_float(torch.from_numpy(np.clip(np.roll(scene, k, axis=1), 0, 1)).to(dev).reshape(-1)) for k, name in enumerate(('left', 'right'))}
    d = td.Deconvolve(dev, (w, h), sigma=0.7, iterations=5)
    color = td.ColorLUT(dev, matrix=((0.9, 0.1, 0.0), (0.05, 0.9, 0.05), (0.0, 0.2, 0.8)))

    with_stage = _processor(td, dev, w, h, storage_dtype=storage, color=color)
    assert with_stage.capture_sharpen is None
    with_stage.capture_sharpen = d
    assert with_stage.capture_sharpen is d
    got = with_stage.process_image_set(packed)

    # the chain composed by hand: demosaic, deconvolution, colour, and on from the frames with a processor that has neither
    by_hand = _processor(td, dev, w, h, storage_dtype=storage)
    frames = [color.process(d.process(by_hand.load_image(b))) for b in packed.values()]
    assert frames[0].dtype == storage
    expected = by_hand._process_frames(list(packed), frames, resized=False)
    assert sorted(got) == sorted(expected) == ['left', 'right']
    for name in packed:
        assert got[name].dtype == torch.uint8 and torch.equal(got[name], expected[name]), name
    assert torch.equal(with_stage.bounds, by_hand.bounds) and torch.equal(with_stage.metrics, by_hand.metrics)   # they saw the stage's result
    # ... and not the other order
    swapped = [d.process(color.process(by_hand.load_image(b))) for b in packed.values()]
    assert not torch.equal(swapped[0], frames[0])

    # None: the processor that never had one, and not the stage's result
    never = _processor(td, dev, w, h, storage_dtype=storage, color=color).process_image_set(packed)
    cleared = _processor(td, dev, w, h, storage_dtype=storage, color=color)
    cleared.capture_sharpen = d
    cleared.capture_sharpen = None
    again = cleared.process_image_set(packed)
    for name in packed:
        assert torch.equal(again[name], never[name]) and not torch.equal(got[name], never[name])
