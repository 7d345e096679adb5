"""GPU: the purple-fringe removal (include/tdk_hip_defringe.h, csrc/defringe.hip, torch_darktable.Defringe) against
tests/defringe_spec.py, the float32 restatement of the specification.  Every comparison is on raw bits -- of the frame, of the mask's
bytes, of E, of S and of th: no tolerance anywhere.

The table is pruned, not a product.  Sizes: one pixel and 5 x 3 (smaller than either apron), one tile, a pixel past and short of a
tile, 2 x 2 tiles, 3 x 3 tiles with remainders, a wide low frame.  Radii: the corners of R in {1, 12} x S_r in {1, 8} and the
default (6, 6); every size meets every corner, dtype, domain and mode rotate through them, and one size takes their whole product."""

import ctypes
import functools

import numpy as np
import pytest
import torch

import defringe_spec as spec

pytestmark = pytest.mark.gpu

f32 = np.float32
DTYPES = [np.float32, np.float16]
TILE = spec.TILE
TAPS = {1: (f32(0.5), f32(0.25)), 2: spec.gaussian_taps(0.5), 6: spec.gaussian_taps(2.0), 12: spec.gaussian_taps(4.0)}   # R -> taps
SIZES = [(1, 1), (5, 3), (32, 32), (33, 31), (64, 64), (70, 75), (200, 40)]   # (width, height)
CORNERS = [(1, 1), (1, 8), (12, 1), (12, 8), (6, 6)]   # (R, S_r)
FLOOR = 1e-4


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a visible MI355X'
    return torch.device('cuda', 0)


# ---- content
@functools.lru_cache(maxsize=None)
def content(kind, w, h, seed=0):
    rng = np.random.default_rng(w * 7 + h + seed)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == 'scene':   # coloured blocks under stripes, a bright block up to 64, negative samples, -0
        x = rng.uniform(0.02, 1.0, (-(-h // 5), -(-w // 5), 3)).repeat(5, 0).repeat(5, 1)[:h, :w]
        x = x * np.where((xx + 2 * yy) % 23 < 11, 1.0, 0.3)[..., None] + rng.normal(0.0, 0.01, (h, w, 3))
        x[h // 3: h // 3 + 9, w // 2: w // 2 + 11] = rng.uniform(8.0, 64.0, 3)
        x[rng.random((h, w, 3)) < 0.05] *= -1.0
        x[rng.random((h, w, 3)) < 0.02] = -0.0
    elif kind == 'flat':
        x = np.ones((h, w, 3)) * np.array([0.9, 0.1, 0.4])
    elif kind == 'contrast':   # samples of 0 and 64 side by side: in the linear domain E passes the cap of 1024
        x = np.where(rng.random((h, w, 3)) < 0.5, 0.0, 64.0)
    else:
        raise KeyError(kind)
    x = x.astype(f32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def want(kind, w, h, dtype, radius, sample_radius, strength=1.0, mode='global', domain='sqrt', seed=0):
    """The restatement of one case, computed once and shared: (frame, mask, E, S, th)."""
    out = spec.process(content(kind, w, h, seed).astype(dtype), TAPS[radius], sample_radius, strength, FLOOR, mode, domain)
    for a in out[:3]:
        a.setflags(write=False)
    return out


def bits(a):
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def same_bits(got, expected, what):
    got = got.cpu().numpy()
    assert got.dtype == expected.dtype and got.shape == expected.shape, (what, got.dtype, expected.dtype, got.shape, expected.shape)
    bad = np.argwhere(bits(got) != bits(expected))
    if len(bad):
        print(f'{what}: {len(bad)} of {expected.size} values differ, first at {bad[0]}: got {got[tuple(bad[0])]!r} want {expected[tuple(bad[0])]!r}')
    assert len(bad) == 0, what


def same_record(record, expected, what):
    """(S, th) as device tensors against the restatement's."""
    s, th = int(record[0].cpu()), record[1].cpu().numpy()
    assert s == expected[3], (what, 'S', s, expected[3])
    assert th.dtype == f32 and bits(th.reshape(1))[0] == bits(np.asarray(expected[4], dtype=f32).reshape(1))[0], (what, 'th', th, expected[4])


def make(td, dev, w, h, radius, sample_radius, strength=1.0, mode='global', domain='sqrt', groups=None):
    d = td.Defringe.from_weights(dev, (w, h), TAPS[radius], radius=sample_radius, strength=strength, floor=FLOOR, mode=mode, domain=domain)
    d.max_groups = groups
    return d


def source(dev, kind, w, h, dtype, seed=0):
    return torch.from_numpy(content(kind, w, h, seed).astype(dtype)).to(dev)


def check_all(d, src, expected, what):
    """The frame, the mask, the record and E of one object on one frame."""
    h, w = src.shape[:2]
    out, m = d.process(src, return_mask=True)
    record = tuple(t.clone() for t in d.threshold())
    assert out.dtype == src.dtype and out.is_contiguous() and out.data_ptr() != src.data_ptr() and m.dtype == torch.uint8 and tuple(m.shape) == (h, w)
    e = d.edge(src)
    assert e.dtype == torch.float32 and tuple(e.shape) == (h, w)
    same_bits(e, expected[2], (*what, 'E'))
    same_record(record, expected, what)
    same_record(d.threshold(), expected, (*what, 'after edge()'))
    same_bits(m, expected[1], (*what, 'mask'))
    same_bits(out, expected[0], what)
    return out, m


def check_case(td, dev, kind, w, h, dtype, radius, sample_radius, groups=None, **kw):
    d = make(td, dev, w, h, radius, sample_radius, groups=groups, **kw)
    src = source(dev, kind, w, h, dtype)
    expected = want(kind, w, h, dtype, radius, sample_radius, **kw)
    out, m = check_all(d, src, expected, (kind, w, h, dtype.__name__, radius, sample_radius, groups, kw))
    return d, src, out, m, expected


# ------------------------------------------------------------------ 1. geometry
@pytest.mark.parametrize('size', SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_sizes_and_radius_corners_give_the_restatements_bits(td, dev, size):
    w, h = size
    both = 0
    for k, (radius, sample_radius) in enumerate(CORNERS):
        k += SIZES.index(size)
        dtype, domain, mode = DTYPES[k % 2], ('sqrt', 'linear')[(k // 2) % 2], ('global', 'static')[(k // 3) % 2]
        strength = 1.0 if mode == 'global' else (0.02 if domain == 'sqrt' else 0.01)
        *_, expected = check_case(td, dev, 'scene', w, h, dtype, radius, sample_radius, strength=strength, mode=mode, domain=domain)
        both += int(0 < expected[1].sum() < w * h)
    assert both >= (4 if w * h > 15 else 0)   # fringed and untouched pixels in the same frame


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('domain', ['sqrt', 'linear'])
@pytest.mark.parametrize('mode', ['global', 'static'])
def test_every_dtype_domain_and_mode_on_three_by_three_tiles(td, dev, dtype, domain, mode):
    strength = 1.5 if mode == 'global' else 0.01
    *_, expected = check_case(td, dev, 'scene', 70, 75, dtype, 6, 6, strength=strength, mode=mode, domain=domain)
    assert 0.02 < expected[1].mean() < 0.9
    # tiles without a fringed pixel (they stream the input through) and tiles with one
    tiles = [expected[1][y:y + TILE, x:x + TILE].any() for y in range(0, 75, TILE) for x in range(0, 70, TILE)]
    assert any(tiles) and (not all(tiles) or (domain, mode) != ('linear', 'global'))


def test_the_table_meets_its_cases():
    assert any(w < 2 and h < 2 for w, h in SIZES) and any(w < 8 and h < 8 and w * h > 1 for w, h in SIZES)   # smaller than either apron
    assert (TILE, TILE) in SIZES and (TILE + 1, TILE - 1) in SIZES and (2 * TILE, 2 * TILE) in SIZES
    assert any(2 * TILE < w < 3 * TILE and 2 * TILE < h < 3 * TILE and w % 4 and h % 4 for w, h in SIZES)   # 3 x 3 tiles with remainders
    assert any(w % 4 == 0 for w, h in SIZES) and any(w % 4 for w, h in SIZES)   # rows of whole vectors and rows with a tail
    assert {r for r, _ in CORNERS} == {1, 6, 12} and {s for _, s in CORNERS} == {1, 6, 8} and len(CORNERS) == 5
    assert all(len(TAPS[r]) == r + 1 for r in TAPS) and spec.MAX_RADIUS == 12 and spec.MAX_SAMPLE_RADIUS == 8


# ------------------------------------------------------------------ 2. content
@pytest.mark.parametrize('dtype', DTYPES)
def test_flat_frame_returns_its_bits(td, dev, dtype):
    for mode, domain in (('global', 'sqrt'), ('static', 'linear')):
        d, src, out, m, expected = check_case(td, dev, 'flat', 45, 37, dtype, 6, 6, strength=0.0, mode=mode, domain=domain)
        assert torch.equal(out.view(torch.uint8), src.view(torch.uint8)) and not m.any() and expected[3] == 0 and expected[4] == f32(FLOOR)


def test_edge_chroma_above_the_cap_of_the_statistic(td, dev):
    w, h = 41, 35
    *_, expected = check_case(td, dev, 'contrast', w, h, np.float32, 1, 6, strength=0.5, domain='linear')
    e = expected[2]
    assert (e > 1024).any() and (e < 1024).any() and expected[3] < int(np.floor(e.astype(np.float64) * 1048576.0).sum())   # the cap took something
    assert 0 < expected[1].sum() < w * h
    check_case(td, dev, 'contrast', w, h, np.float16, 1, 6, strength=0.5, domain='linear')


@pytest.mark.parametrize('dtype', DTYPES)
def test_static_threshold_at_and_just_below_the_largest_edge_chroma(td, dev, dtype):
    """A static strength equal to the largest E returns the input's bits; the float32 below it rewrites exactly that pixel."""
    w, h = 70, 37
    e = want('scene', w, h, dtype, 6, 6, strength=0.0, mode='static')[2]
    top = float(e.max())
    assert (e == e.max()).sum() == 1
    d, src, out, m, _ = check_case(td, dev, 'scene', w, h, dtype, 6, 6, strength=top, mode='static')
    assert torch.equal(out.view(torch.uint8), src.view(torch.uint8)) and not m.any()
    below = float(np.nextafter(e.max(), f32(0)))
    d, src, out, m, expected = check_case(td, dev, 'scene', w, h, dtype, 6, 6, strength=below, mode='static')
    y, x = np.unravel_index(int(e.argmax()), e.shape)
    assert int(m.sum()) == 1 and int(m[y, x]) == 1
    changed = (out.view(torch.uint8) != src.view(torch.uint8)).view(h, w, -1).any(dim=2)
    assert int(changed.sum()) == 1 and bool(changed[y, x])


# ------------------------------------------------------------------ 3. mechanics
@pytest.mark.parametrize('groups', [1, 2])
def test_capped_workgroups_give_the_same_bits(td, dev, groups):
    for dtype, domain in zip(DTYPES, ('sqrt', 'linear')):
        d, *_ = check_case(td, dev, 'scene', 70, 75, dtype, 6, 6, groups=groups, strength=1.5, domain=domain)
        assert d.max_groups == groups


def test_more_tiles_than_workgroups(td, dev):
    """33 x 32 tiles for 1024 workgroups: thirty-two workgroups walk on to a second tile, and the last record is the 1024th."""
    w, h = 1056, 1024
    assert (w // TILE) * (h // TILE) == spec.MAX_GROUPS + 32
    d, *_ , expected = check_case(td, dev, 'scene', w, h, np.float32, 2, 2)
    assert d.max_groups == spec.MAX_GROUPS and 0.01 < expected[1].mean() < 0.9


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
    for w, h in ((2 * TILE + 4, TILE + 1), (TILE + 3, 7)):
        d = make(td, dev, w, h, 6, 6)
        src = source(dev, 'scene', w, h, dtype)
        expected = want('scene', w, h, dtype, 6, 6)
        for offset in (0, 1, 2, 3):
            out, m = d.process(at_offset(src, offset), return_mask=True)
            same_bits(out, expected[0], (w, h, offset))
            same_bits(m, expected[1], (w, h, offset, 'mask'))
    d = make(td, dev, 40, 36, 6, 6)
    wide = torch.zeros((36, 48, 3), dtype=src.dtype, device=dev)
    with pytest.raises(RuntimeError, match='contiguous'):
        d.process(wide[:, :40])
    with pytest.raises(RuntimeError, match='expected'):
        d.process(wide)
    with pytest.raises(ValueError, match='float32 or float16'):
        d.process(torch.zeros((36, 40, 3), dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match='3 channels'):
        d.process(torch.zeros((36, 40, 1), dtype=src.dtype, device=dev))


def test_outputs_at_odd_offsets_through_the_c_entry_point(td, dev):
    """Every output inside a larger zeroed buffer at the least alignment the header allows: the bits are the restatement's and nothing
    is written outside; then the same call without the optional outputs."""
    from torch_darktable._native import lib

    for (w, h, radius, sample_radius), dtype, tag in (((2 * TILE + 4, TILE + 1, 6, 6), np.float32, 0), ((TILE + 5, TILE + 2, 12, 8), np.float16, 1)):
        src = source(dev, 'scene', w, h, dtype)
        n = w * h
        pool = torch.zeros(3 * n + 40, dtype=src.dtype, device=dev)
        m_pool = torch.zeros(n + 40, dtype=torch.uint8, device=dev)
        e_pool = torch.zeros(n + 40, dtype=torch.float32, device=dev)
        s_pool = torch.zeros(48, dtype=torch.uint8, device=dev)
        out, m, e, stats = pool[3:3 + 3 * n], m_pool[1:1 + n], e_pool[1:1 + n], s_pool[8:24]
        need = int(lib.tdk_defringe_workspace_bytes(w, h))
        assert need == spec.workspace_bytes(w, h)
        ws_pool = torch.zeros(need + 16, dtype=torch.uint8, device=dev)
        ws = ws_pool[5:5 + need]
        taps = (ctypes.c_float * (radius + 1))(*TAPS[radius])
        stream = torch.cuda.current_stream().cuda_stream
        rc = lib.tdk_defringe(src.data_ptr(), out.data_ptr(), m.data_ptr(), e.data_ptr(), stats.data_ptr(), ws.data_ptr(), w, h, tag, taps, radius, sample_radius, 1.0,
                              FLOOR, 0, stream)
        assert rc == 0, lib.tdk_last_error()
        torch.cuda.synchronize()
        expected = want('scene', w, h, dtype, radius, sample_radius)
        same_bits(out.view(h, w, 3), expected[0], (w, h, 'frame'))
        same_bits(m.view(h, w), expected[1], (w, h, 'mask'))
        same_bits(e.view(h, w), expected[2], (w, h, 'E'))
        same_record((stats[:8].view(torch.int64)[0], stats[8:12].view(torch.float32)[0]), expected, (w, h))
        assert int(stats[12:16].max()) == 0
        assert float(pool[:3].float().abs().max()) == 0 and float(pool[3 + 3 * n:].float().abs().max()) == 0   # nothing written outside
        assert int(m_pool[:1].max()) == 0 and int(m_pool[1 + n:].max()) == 0
        assert float(e_pool[:1].abs().max()) == 0 and float(e_pool[1 + n:].abs().max()) == 0
        assert int(s_pool[:8].max()) == 0 and int(s_pool[24:].max()) == 0
        assert int(ws_pool[:5].max()) == 0 and int(ws_pool[5 + need:].max()) == 0
        plain = torch.zeros(3 * n, dtype=src.dtype, device=dev)
        rc = lib.tdk_defringe(src.data_ptr(), plain.data_ptr(), None, None, None, ws.data_ptr(), w, h, tag, taps, radius, sample_radius, 1.0, FLOOR, 0, stream)
        assert rc == 0, lib.tdk_last_error()
        same_bits(plain.view(h, w, 3), expected[0], (w, h, 'no optional outputs'))


def test_workspace_filled_with_nan_gives_the_same_bits(td, dev):
    for dtype, (w, h) in zip(DTYPES, ((2 * TILE + 3, TILE + 3), (TILE + 4, 2 * TILE + 1))):
        d, src, out, m, _ = check_case(td, dev, 'scene', w, h, dtype, 6, 6)
        assert len(d._workspaces) == 1 and d.launches == 2 and d.workspace_bytes() == spec.workspace_bytes(w, h)
        for buf in d._workspaces._buffers.values():
            assert buf.numel() == d.workspace_bytes() + 16
            buf.fill_(0xFF)   # every float32 a NaN, every partial sum 2^64 - 1
        again, m_again = d.process(src, return_mask=True)
        assert torch.equal(again.view(torch.uint8), out.view(torch.uint8)) and torch.equal(m_again, m)


def test_one_object_on_two_streams_at_once(td, dev):
    """Interleaved calls on two frames with different thresholds: each stream has its own plane of E, partial sums and record."""
    w, h = 2 * TILE + 3, 2 * TILE + 3
    d = make(td, dev, w, h, 6, 6)
    frames = [source(dev, 'scene', w, h, np.float32, seed) for seed in (0, 1)]
    streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    outs, records = [], []
    for _ in range(3):
        for s, frame in zip(streams, frames):
            with torch.cuda.stream(s):
                outs.append(d.process(frame))
    for s in streams:
        with torch.cuda.stream(s):
            records.append(d.threshold())
    torch.cuda.synchronize()
    assert len(d._workspaces) == 3   # the stream of construction and the two
    expected = [want('scene', w, h, np.float32, 6, 6, seed=seed) for seed in (0, 1)]
    assert expected[0][3] != expected[1][3]
    for k, out in enumerate(outs):
        same_bits(out, expected[k % 2][0], ('stream', k % 2, 'round', k // 2))
    for k in (0, 1):
        same_record(records[k], expected[k], ('stream', k))


def test_graph_follows_the_new_threshold(td, dev):
    """An object built on the side stream and captured there without a warm-up call (the workspace exists since construction); a
    replay after the input buffer was rewritten gathers the new statistic and equals the restatement of the new frame."""
    w, h = 2 * TILE + 3, TILE + 5
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        d = make(td, dev, w, h, 6, 6)
        buffer = source(dev, 'scene', w, h, np.float16).clone()
        with torch.cuda.graph(graph, stream=stream):
            captured, captured_m = d.process(buffer, return_mask=True)
        for seed in (0, 1, 0):
            buffer.copy_(source(dev, 'scene', w, h, np.float16, seed))
            graph.replay()
            stream.synchronize()
            expected = want('scene', w, h, np.float16, 6, 6, seed=seed)
            same_bits(captured, expected[0], ('replay', seed))
            same_bits(captured_m, expected[1], ('replayed mask', seed))
            same_record(d.threshold(), expected, ('replayed record', seed))
    a, b = want('scene', w, h, np.float16, 6, 6, seed=0), want('scene', w, h, np.float16, 6, 6, seed=1)
    assert a[4] != b[4] and not np.array_equal(a[1], b[1])


# ------------------------------------------------------------------ 4. pipeline
def _processor(td, dev, w, h, **kw):
    from torch_darktable.pipeline import Debayer, ImageProcessingSettings, ImageProcessor, ImageTransform, ToneMapper
    settings = ImageProcessingSettings(moving_average=0.3, postprocess=False, enable_denoise=True, enable_bilateral=True, tone_mapping=ToneMapper.reinhard,
                                       debayer=Debayer.bilinear)
    return ImageProcessor((w, h), td.BayerPattern.RGGB, td.PackedFormat.Packed12, settings, dev, (1.9, 1.0, 1.6), transforms=ImageTransform.none, **kw)


@pytest.mark.parametrize('storage', [torch.float32, torch.float16])
def test_pipeline_runs_it_in_front_of_capture_sharpen(td, dev, storage):
    w, h = 128, 96
    scene = content('scene', w, h)[..., 1]
    packed = {name: td.encode12_float(torch.from_numpy(np.clip(np.roll(scene, k, axis=1), 0, 1)).to(dev).reshape(-1)) for k, name in enumerate(('left', 'right'))}
    d = td.Defringe(dev, (w, h), strength=1.0)
    sharpen = td.Deconvolve(dev, (w, h), sigma=0.7, iterations=3)

    with_stage = _processor(td, dev, w, h, storage_dtype=storage)
    with_stage.capture_sharpen = sharpen
    assert with_stage.defringe is None
    with_stage.defringe = d
    assert with_stage.defringe is d
    got = with_stage.process_image_set(packed)

    # the chain with the restatement spliced in: demosaic, the restatement on the host, and on from the frames with a processor
    # that has capture_sharpen only
    by_hand = _processor(td, dev, w, h, storage_dtype=storage)
    by_hand.capture_sharpen = sharpen
    frames, share = [], []
    for b in packed.values():
        rgb = by_hand.load_image(b)
        assert rgb.dtype == storage
        restated = spec.process(rgb.cpu().numpy(), spec.gaussian_taps(2.0), 6, 1.0, FLOOR)
        same_bits(d.process(rgb), restated[0], 'the stage on a demosaiced frame')
        frames.append(torch.from_numpy(restated[0]).to(dev))
        share.append(restated[1].mean())
    assert all(0.01 < s < 0.9 for s in share)
    expected = by_hand._process_frames(list(packed), frames, resized=False)
    assert sorted(got) == sorted(expected) == ['left', 'right']
    for name in packed:
        assert got[name].dtype == torch.uint8 and torch.equal(got[name], expected[name]), name
    assert torch.equal(with_stage.bounds, by_hand.bounds) and torch.equal(with_stage.metrics, by_hand.metrics)   # they saw the stage's result
    # ... and not the other order
    swapped = d.process(sharpen.process(by_hand.load_image(packed['left'])))
    assert not torch.equal(swapped, sharpen.process(frames[0]))

    # None: the processor that never had one, and not the stage's result
    never = _processor(td, dev, w, h, storage_dtype=storage)
    never.capture_sharpen = sharpen
    never = never.process_image_set(packed)
    cleared = _processor(td, dev, w, h, storage_dtype=storage)
    cleared.capture_sharpen = sharpen
    cleared.defringe = d
    cleared.defringe = None
    again = cleared.process_image_set(packed)
    for name in packed:
        assert torch.equal(again[name], never[name]) and not torch.equal(got[name], never[name])
