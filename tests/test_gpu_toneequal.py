"""GPU: the tone equalizer (include/tdk_hip_toneeq.h, csrc/toneequal.hip, torch_darktable.ToneEqualizer) against
tests/toneequal_spec.py, the float32 restatement of the specification.  Every comparison is on the raw bits of the frame and of the
mask: no tolerance anywhere.

The geometry table is pruned, not a product: every cell size and every radius meets a frame smaller than a cell, a frame that is no
multiple of the cell, a grid smaller than the window (radius 0 has no such grid) and a frame that crosses a tile boundary of each
kernel -- te_cells: 256 (float32) or 512 (binary16) columns and 16 rows per wave, 64 per workgroup; te_coeff: 32 x 32 cells;
te_apply: 128 x 32 pixels."""

import functools

import numpy as np
import pytest
import torch

import toneequal_spec as spec

pytestmark = pytest.mark.gpu

f32 = np.float32
DTYPES = [np.float32, np.float16]
GAINS = (3, 3, 3, 2.5, 2, 1.5, 1, 0.5, 0)
BURN = (2, 2, 1.5, 1, 0.5, 0, 0, -0.5, -1)

# (width, height, cell, radius)
SMALLER_THAN_A_CELL = [(1, 1, 2, 0), (1, 1, 4, 1), (1, 1, 8, 3), (1, 1, 16, 8), (5, 3, 8, 8), (5, 3, 16, 0)]
NO_MULTIPLE = [(33, 17, 2, 8), (33, 17, 4, 3), (33, 17, 8, 1), (33, 17, 16, 0), (5, 3, 2, 3), (5, 3, 4, 0)]
GRID_SMALLER_THAN_WINDOW = [(5, 3, 2, 1), (33, 17, 4, 3), (130, 70, 8, 8), (130, 70, 16, 3), (257, 131, 16, 8), (33, 17, 8, 3), (5, 3, 4, 1)]
TILE_BOUNDARIES = [(517, 67, 2, 3), (517, 67, 4, 8), (517, 67, 8, 0), (517, 67, 16, 1), (130, 70, 2, 0), (257, 131, 4, 1), (257, 131, 8, 3), (130, 70, 2, 8)]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a visible MI355X'
    return torch.device('cuda', 0)


# ---- content
def lognormal(h, w, seed=0, lo=-12.0, hi=2.0):
    rng = np.random.default_rng(seed)
    base = np.exp2(rng.uniform(lo, hi, (-(-h // 24), -(-w // 24), 1)))   # regions of 24 x 24 pixels, so that the mask has a range too
    base = np.repeat(np.repeat(base, 24, axis=0), 24, axis=1)[:h, :w]
    return (base * np.exp2(rng.normal(0.0, 0.5, (h, w, 3)))).astype(f32)


@functools.lru_cache(maxsize=None)
def content(kind, w, h, cell):
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == 'lognormal':
        x = lognormal(h, w, w * 7 + h)
    elif kind == 'constant':
        x = np.full((h, w, 3), 0.18, dtype=f32)
    elif kind == 'zeros':
        x = np.zeros((h, w, 3), dtype=f32)
    elif kind == 'negative':
        x = lognormal(h, w, 3)
        rng = np.random.default_rng(4)
        x = x * np.where(rng.random((h, w, 3)) < 0.3, -1.0, 1.0).astype(f32)
        x[: h // 3] = -np.abs(x[: h // 3])   # a region whose luminance is 0 throughout
    elif kind == 'clamps':   # 2^-20 .. 2^6: a third of the frame below the table, a third above it
        ev = np.where(xx < w // 3, -18.5, np.where(xx >= w - w // 3, 5.0, -6.0))[..., None]
        x = np.exp2(ev + np.random.default_rng(5).uniform(-1.5, 1.0, (h, w, 3))).astype(f32)
    elif kind == 'edge_on':
        x = (np.where(xx < (w // 2) // cell * cell, 2.0 ** -7, 2.0 ** -2)[..., None] * np.ones(3)).astype(f32)
    elif kind == 'edge_off':
        x = (np.where(xx < (w // 2) // cell * cell + cell // 2 + 1, 2.0 ** -7, 2.0 ** -2)[..., None] * np.ones(3)).astype(f32)
    elif kind == 'checker':
        x = (np.where((xx // cell + yy // cell) % 2 == 0, 0.02, 0.6)[..., None] * np.array([1.0, 0.9, 1.1])).astype(f32)
    elif kind == 'half_max':
        x = np.random.default_rng(6).uniform(60000.0, 65504.0, (h, w, 3)).astype(f32)
    else:
        raise KeyError(kind)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def table_of(gains, mask_exposure=0.0):
    t = spec.make_table(gains, mask_exposure)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def want(kind, w, h, cell, radius, dtype, gains=GAINS, mask_exposure=0.0, eps=1e-4, weights=spec.REC709):
    """The restatement of one case, computed once and shared: (frame, mask)."""
    out, m = spec.process(content(kind, w, h, cell).astype(dtype), table_of(gains, mask_exposure), cell, radius, eps, weights)
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


def make(td, dev, w, h, cell, radius, gains=GAINS, mask_exposure=0.0, eps=1e-4, weights=None):
    te = td.ToneEqualizer(dev, (w, h), gains_ev=gains, cell=cell, radius=radius, eps=eps, mask_exposure=mask_exposure, weights=weights)
    assert np.array_equal(te.table.cpu().numpy(), table_of(tuple(gains), mask_exposure))
    return te


def source(dev, kind, w, h, cell, dtype):
    return torch.from_numpy(content(kind, w, h, cell).astype(dtype)).to(dev)


def check_case(td, dev, kind, w, h, cell, radius, dtype, **kw):
    te = make(td, dev, w, h, cell, radius, **kw)
    src = source(dev, kind, w, h, cell, dtype)
    out, mask = te.process(src, return_mask=True)
    assert out.dtype == src.dtype and out.is_contiguous() and out.data_ptr() != src.data_ptr() and mask.dtype == torch.float32
    spec_kw = {k: (tuple(v) if k in ('gains', 'weights') else v) for k, v in kw.items()}
    out_w, mask_w = want(kind, w, h, cell, radius, dtype, **spec_kw)
    what = (kind, w, h, cell, radius, dtype.__name__, kw)
    same_bits(mask, mask_w, (*what, 'mask'))
    same_bits(out, out_w, what)
    return te, src, out, mask


def at_offset(t, elements):
    """A contiguous copy of CUDA tensor `t` that starts `elements` elements past an aligned allocation."""
    pool = torch.zeros(t.numel() + elements + 16, dtype=t.dtype, device=t.device)
    assert pool.data_ptr() % 256 == 0
    v = pool[elements:elements + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() == pool.data_ptr() + elements * t.element_size()
    return v


# ------------------------------------------------------------------ 1. geometry
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('cases', [SMALLER_THAN_A_CELL, NO_MULTIPLE, GRID_SMALLER_THAN_WINDOW, TILE_BOUNDARIES], ids=['smaller_than_a_cell', 'no_multiple', 'grid_smaller_than_window', 'tile_boundaries'])
def test_geometry_gives_the_restatements_bits(td, dev, cases, dtype):
    assert {c[2] for c in cases} == {2, 4, 8, 16} and {c[3] for c in cases} >= {1, 3, 8}
    for w, h, cell, radius in cases:
        check_case(td, dev, 'lognormal', w, h, cell, radius, dtype)


def test_the_table_meets_its_cases():
    """The rows do what their list's name says."""
    for w, h, cell, _ in SMALLER_THAN_A_CELL:
        assert w < cell and h < cell
    for w, h, cell, _ in NO_MULTIPLE:
        assert w % cell and h % cell
    for w, h, cell, radius in GRID_SMALLER_THAN_WINDOW:
        assert min(-(-w // cell), -(-h // cell)) < 2 * radius + 1
    for cell in (2, 4, 8, 16):
        rows = [c for c in TILE_BOUNDARIES if c[2] == cell]
        assert any(w > 512 and h > 64 for w, h, _, _ in rows)                                # te_cells, either storage type
        assert any(-(-w // cell) > 32 for w, h, _, _ in rows)                                  # te_coeff
        assert any(w > 128 and h > 32 for w, h, _, _ in rows)                                  # te_apply
    assert any(-(-h // 2) > 32 for w, h, cell, _ in TILE_BOUNDARIES if cell == 2)             # te_coeff along y


# ------------------------------------------------------------------ 2. content
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kind', ['constant', 'zeros', 'negative', 'clamps', 'edge_on', 'edge_off', 'checker'])
def test_content_classes(td, dev, kind, dtype):
    for w, h, cell, radius in ((130, 70, 8, 4), (257, 131, 4, 1), (33, 17, 2, 0)):
        gains, exposure = (BURN, -1.0) if kind in ('clamps', 'negative') else (GAINS, 0.0)
        check_case(td, dev, kind, w, h, cell, radius, dtype, gains=gains, mask_exposure=exposure)
    if kind == 'clamps':
        m = want(kind, 257, 131, 4, 1, dtype, gains=BURN, mask_exposure=-1.0)[1]
        assert (m < spec.M_LO).sum() > 500 and (m > spec.M_HI).sum() > 500   # both ends of the table are met
    if kind == 'negative':
        assert (want(kind, 130, 70, 8, 4, dtype, gains=BURN, mask_exposure=-1.0)[0] < 0).any()


def test_constant_frame_has_zero_variance(td, dev):
    """Radius 0: var = L*L - L*L is exactly 0, a = 0, and the mask is the luminance."""
    for dtype in DTYPES:
        _, src, _, mask = check_case(td, dev, 'constant', 130, 70, 8, 0, dtype)
        lum = spec.luminance(content('constant', 130, 70, 8).astype(dtype))
        same_bits(mask, lum, 'mask of a constant frame')


def test_binary16_values_near_the_largest(td, dev):
    for cell, radius in ((8, 4), (2, 1)):
        _, _, out, _ = check_case(td, dev, 'half_max', 130, 70, cell, radius, np.float16, gains=(0,) * 8 + (1,), mask_exposure=-4.0)
        assert torch.isinf(out).any() and not torch.isnan(out).any()   # x2 leaves binary16: rounded to infinity, as the restatement has it
        check_case(td, dev, 'half_max', 130, 70, cell, radius, np.float16, gains=BURN, mask_exposure=-4.0)


@pytest.mark.parametrize('dtype', DTYPES)
def test_zero_gains_return_the_inputs_bits(td, dev, dtype):
    for kind, w, h, cell, radius in (('negative', 130, 70, 8, 4), ('clamps', 257, 131, 2, 3), ('lognormal', 517, 67, 16, 8)):
        te = make(td, dev, w, h, cell, radius, gains=(0,) * 9)
        src = source(dev, kind, w, h, cell, dtype)
        assert torch.equal(te.process(src).view(torch.uint8), src.view(torch.uint8))


def test_mask_only_and_return_mask_agree(td, dev):
    for dtype in DTYPES:
        te, src, _, mask = check_case(td, dev, 'lognormal', 257, 131, 8, 3, dtype)
        alone = te.mask(src)
        assert alone.dtype == torch.float32 and tuple(alone.shape) == (131, 257)
        assert torch.equal(alone.view(torch.int32), mask.view(torch.int32))


@pytest.mark.parametrize('eps', [1e-8, 1.0])
def test_eps(td, dev, eps):
    for dtype in DTYPES:
        check_case(td, dev, 'lognormal', 130, 70, 4, 3, dtype, eps=eps)
        check_case(td, dev, 'edge_off', 130, 70, 8, 1, dtype, eps=eps)


def test_custom_weights(td, dev):
    for weights in ((0.25, 0.5, 0.25), (0.0, 1.0, 0.0), (1.5, 0.0, 0.3)):
        check_case(td, dev, 'negative', 130, 70, 8, 4, np.float32, weights=weights)
        check_case(td, dev, 'lognormal', 33, 17, 2, 1, np.float16, weights=weights)


# ------------------------------------------------------------------ 3. workspace, streams, graphs
def test_workspace_filled_with_nan_gives_the_same_bits(td, dev):
    for dtype, (w, h, cell, radius) in zip(DTYPES, ((257, 131, 4, 3), (130, 70, 16, 8))):
        te, src, out, mask = check_case(td, dev, 'lognormal', w, h, cell, radius, dtype)
        assert len(te._workspaces) == 1
        for buf in te._workspaces._buffers.values():
            assert buf.numel() == te.workspace_bytes()
            buf.fill_(0xFF)   # every float32 a NaN
        again, mask_again = te.process(src, return_mask=True)
        assert torch.equal(again.view(torch.uint8), out.view(torch.uint8)) and torch.equal(mask_again.view(torch.int32), mask.view(torch.int32))


def test_two_streams_each_with_its_own_workspace(td, dev):
    w, h, cell, radius = 257, 131, 8, 3
    te = make(td, dev, w, h, cell, radius)
    src = source(dev, 'lognormal', w, h, cell, np.float32)
    one = te.process(src)
    s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    for s in (s1, s2):
        s.wait_stream(torch.cuda.current_stream())
    outs = []
    for _ in range(3):
        with torch.cuda.stream(s1):
            oa = te.process(src)
        with torch.cuda.stream(s2):
            ob = te.process(src)
        outs.append((oa, ob))
    torch.cuda.synchronize()
    assert len(te._workspaces) == 3   # the stream of construction and the two
    for oa, ob in outs:
        assert torch.equal(oa.view(torch.int32), one.view(torch.int32)) and torch.equal(ob.view(torch.int32), one.view(torch.int32))
    same_bits(one, want('lognormal', w, h, cell, radius, np.float32)[0], 'two streams')


def test_graph_replays_and_follows_set_gains(td, dev):
    """An object built on the side stream and captured there without a warm-up call (table and workspace exist since construction);
    a replay equals the restatement, and after set_gains the restatement of the new table."""
    w, h, cell, radius = 130, 70, 8, 4
    src = source(dev, 'lognormal', w, h, cell, np.float16)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        te = make(td, dev, w, h, cell, radius)
        with torch.cuda.graph(graph, stream=stream):
            captured, captured_mask = te.process(src, return_mask=True)
        table_ptr = te.table.data_ptr()
        graph.replay()
        stream.synchronize()
        same_bits(captured, want('lognormal', w, h, cell, radius, np.float16)[0], 'replay')
        same_bits(captured_mask, want('lognormal', w, h, cell, radius, np.float16)[1], 'replayed mask')
        te.set_gains(BURN, mask_exposure=-1.0)
        assert te.table.data_ptr() == table_ptr and te.gains_ev == tuple(float(v) for v in BURN) and te.mask_exposure == -1.0
        graph.replay()
        stream.synchronize()
        same_bits(captured, want('lognormal', w, h, cell, radius, np.float16, gains=BURN, mask_exposure=-1.0)[0], 'replay after set_gains')
        te.set_gains(GAINS)   # mask_exposure stays
        graph.replay()
        stream.synchronize()
        same_bits(captured, want('lognormal', w, h, cell, radius, np.float16, gains=GAINS, mask_exposure=-1.0)[0], 'replay after the second set_gains')


# ------------------------------------------------------------------ 4. views
@pytest.mark.parametrize('dtype', DTYPES)
def test_offset_and_non_contiguous_views(td, dev, dtype):
    """A contiguous view at an odd element offset is taken (the accesses go element by element); a non-contiguous one is refused."""
    for w, h, cell, radius in ((130, 70, 8, 4), (257, 131, 2, 1)):
        te = make(td, dev, w, h, cell, radius)
        src = source(dev, 'lognormal', w, h, cell, dtype)
        out_w, mask_w = want('lognormal', w, h, cell, radius, dtype)
        for offset in (1, 2, 3):
            view = at_offset(src, offset)
            assert view.data_ptr() % 16 != 0
            out, mask = te.process(view, return_mask=True)
            same_bits(out, out_w, (w, h, offset))
            same_bits(mask, mask_w, (w, h, offset, 'mask'))
    wide = torch.zeros((70, 140, 3), dtype=src.dtype, device=dev)
    te = make(td, dev, 130, 70, 8, 4)
    with pytest.raises(RuntimeError, match='contiguous'):
        te.process(wide[:, :130])
    with pytest.raises(RuntimeError, match='contiguous'):
        te.process(torch.zeros((130, 70, 3), dtype=src.dtype, device=dev).transpose(0, 1))
    with pytest.raises(RuntimeError, match='expected'):
        te.process(wide)
    with pytest.raises(ValueError, match='channels must be 3'):
        te.mask(torch.zeros((70, 130, 1), dtype=src.dtype, device=dev))
    with pytest.raises(ValueError, match='float32 or float16'):
        te.process(torch.zeros((70, 130, 3), dtype=torch.uint8, device=dev))


def test_outputs_at_odd_offsets_through_the_c_entry_point(td, dev):
    from torch_darktable._native import lib

    import ctypes
    for (w, h, cell, radius), dtype, tag in (((257, 131, 4, 3), np.float32, 0), ((130, 70, 8, 4), np.float16, 1)):
        te = make(td, dev, w, h, cell, radius)
        src = source(dev, 'lognormal', w, h, cell, dtype)
        n = w * h
        pool = torch.zeros(3 * n + 40, dtype=src.dtype, device=dev)
        mask_pool = torch.zeros(n + 40, dtype=torch.float32, device=dev)
        out, mask = pool[3:3 + 3 * n], mask_pool[1:1 + n]
        ws = torch.zeros(te.workspace_bytes() + 16, dtype=torch.uint8, device=dev)[5:]
        weights = (ctypes.c_float * 3)(*te.weights)
        rc = lib.tdk_toneeq(src.data_ptr(), out.data_ptr(), mask.data_ptr(), ws.data_ptr(), te.table.data_ptr(), w, h, tag, cell, radius, te.eps, weights, 0,
                            torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.tdk_last_error()
        torch.cuda.synchronize()
        out_w, mask_w = want('lognormal', w, h, cell, radius, dtype)
        same_bits(out.view(h, w, 3), out_w, (w, h, 'frame'))
        same_bits(mask.view(h, w), mask_w, (w, h, 'mask'))
        assert float(pool[:3].float().abs().max()) == 0 and float(pool[3 + 3 * n:].float().abs().max()) == 0   # nothing written outside
        assert float(mask_pool[:1].abs().max()) == 0 and float(mask_pool[1 + n:].abs().max()) == 0


# ------------------------------------------------------------------ 5. pipeline
def _processor(td, dev, w, h, **kw):
    from torch_darktable.pipeline import Debayer, ImageProcessingSettings, ImageProcessor, ImageTransform, ToneMapper
    settings = ImageProcessingSettings(moving_average=0.3, postprocess=False, enable_denoise=True, enable_bilateral=True, tone_mapping=ToneMapper.reinhard,
                                       debayer=Debayer.bilinear)
    return ImageProcessor((w, h), td.BayerPattern.RGGB, td.PackedFormat.Packed12, settings, dev, (1.9, 1.0, 1.6), transforms=ImageTransform.none, **kw)


@pytest.mark.parametrize('storage', [torch.float32, torch.float16])
def test_pipeline_runs_it_behind_color_and_in_front_of_the_bounds(td, dev, storage):
    w, h = 128, 96
    lum = lognormal(h, w, 11, -9.0, -0.5)[..., 0]
    packed = {name: td.encode12_float(torch.from_numpy(np.clip(np.roll(lum, k, axis=1), 0, 1)).to(dev).reshape(-1)) for k, name in enumerate(('left', 'right'))}
    te = td.ToneEqualizer(dev, (w, h), gains_ev=GAINS, cell=8, radius=2)
    color = td.ColorLUT(dev, matrix=((0.9, 0.1, 0.0), (0.05, 0.9, 0.05), (0.0, 0.2, 0.8)))

    with_stage = _processor(td, dev, w, h, storage_dtype=storage, color=color)
    assert with_stage.tone_equalizer is None
    with_stage.tone_equalizer = te
    assert with_stage.tone_equalizer is te
    got = with_stage.process_image_set(packed)

    # the chain composed by hand: demosaic, colour, the stage, and on from the frames with a processor that has no such stage
    by_hand = _processor(td, dev, w, h, storage_dtype=storage)
    frames = [te.process(color.process(by_hand.load_image(b))) for b in packed.values()]
    assert frames[0].dtype == storage
    expected = by_hand._process_frames(list(packed), frames, resized=False)
    assert sorted(got) == sorted(expected) == ['left', 'right']
    for name in packed:
        assert got[name].dtype == torch.uint8 and torch.equal(got[name], expected[name]), name
    assert torch.equal(with_stage.bounds, by_hand.bounds) and torch.equal(with_stage.metrics, by_hand.metrics)   # they saw the stage's result

    # None: the processor that never had one, and not the stage's result
    never = _processor(td, dev, w, h, storage_dtype=storage, color=color).process_image_set(packed)
    cleared = _processor(td, dev, w, h, storage_dtype=storage, color=color)
    cleared.tone_equalizer = te
    cleared.tone_equalizer = None
    again = cleared.process_image_set(packed)
    for name in packed:
        assert torch.equal(again[name], never[name]) and not torch.equal(got[name], never[name])
