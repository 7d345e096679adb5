"""GPU: the haze removal (include/tdk_hip_dehaze.h, csrc/dehaze.hip, torch_darktable.Dehaze) against tests/dehaze_spec.py, the
float32 restatement of the specification.  Every comparison is on the raw bits of the frame, of the transmission tp and of the four
ambient values: no tolerance anywhere.

The geometry table is pruned, not a product: every cell size meets a frame smaller than a cell, a grid narrower than both windows, a
frame one past a multiple of the cell, and a frame that crosses a tile boundary of each kernel -- dh_cells: 256 (float32) or 512
(binary16) columns and 16 rows per wave, 64 per workgroup; dh_dark and dh_coeff: 32 x 32 cells; dh_apply: 128 x 32 pixels."""

import ctypes
import functools

import numpy as np
import pytest
import torch

import dehaze_spec as spec

pytestmark = pytest.mark.gpu

f32 = np.float32
DTYPES = [np.float32, np.float16]
DEFAULTS = dict(strength=0.9, floor=0.1, cell=8, dark_radius=1, radius=4, eps=1e-3, quantile=0.01, weights=None)

# (width, height, cell, dark_radius, radius)
SMALLER_THAN_A_CELL = [(1, 1, 2, 0, 0), (1, 1, 4, 1, 1), (1, 1, 16, 4, 8), (7, 5, 8, 1, 4), (5, 3, 16, 2, 0)]
GRID_NARROWER_THAN_THE_WINDOWS = [(7, 5, 2, 4, 8), (33, 17, 8, 3, 3), (33, 17, 16, 4, 8), (7, 5, 4, 2, 2)]
ONE_PAST_A_MULTIPLE = [(33, 17, 2, 1, 2), (33, 17, 4, 2, 3), (33, 17, 8, 1, 1), (33, 17, 16, 0, 1)]
TILE_BOUNDARIES = [(257, 67, 2, 1, 2), (257, 67, 8, 4, 8), (257, 67, 16, 0, 4), (130, 34, 4, 2, 8), (130, 66, 2, 4, 3), (257, 67, 4, 1, 0), (517, 67, 8, 1, 4)]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a visible MI355X'
    return torch.device('cuda', 0)


# ---- content
@functools.lru_cache(maxsize=None)
def content(kind, w, h, cell=8, seed=0):
    rng = np.random.default_rng(w * 7 + h + seed)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == 'hazy':   # a textured scene behind a veil that thins from the top to the bottom, some black pixels
        clear = rng.uniform(0.1, 0.8, (-(-h // 6), -(-w // 6), 3)).repeat(6, 0).repeat(6, 1)[:h, :w] * rng.uniform(0.5, 1.0, (h, w, 1))
        clear[rng.random((h, w)) < 0.05] = 0.0
        t = np.linspace(0.15, 0.95, h)[:, None, None]
        x = clear * t + np.array([0.8, 0.85, 0.9]) * (1 - t)
    elif kind == 'constant':
        x = np.ones((h, w, 3)) * np.array([0.4, 0.5, 0.6])
    elif kind == 'black':
        x = np.zeros((h, w, 3))
    elif kind == 'negative':   # a third of the samples negative, a region that is negative throughout
        x = content('hazy', w, h, cell) * np.where(rng.random((h, w, 3)) < 0.3, -1.0, 1.0)
        x[: h // 3] = -np.abs(x[: h // 3])
    elif kind == 'ties':   # constant cells of a few levels: the dark channel ties, at the threshold too
        levels = rng.integers(1, 5, (-(-h // cell), -(-w // cell), 1)).repeat(cell, 0).repeat(cell, 1)[:h, :w] / 8.0
        x = levels * np.array([1.0, 1.25, 1.5]) + rng.uniform(0.0, 0.25, (h, w, 3)) * (rng.random((h, w, 1)) < 0.5)
    elif kind == 'huge':   # float32 cell means above 65536: the clamp of fix
        x = content('hazy', w, h, cell) * np.where(yy < h // 2, 400000.0, 1.0)[..., None]
    elif kind == 'half_max':
        x = rng.uniform(60000.0, 65504.0, (h, w, 3))
        x[rng.random((h, w)) < 0.1] *= 0.01
    else:
        raise KeyError(kind)
    x = x.astype(f32)
    x.setflags(write=False)
    return x


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


@functools.lru_cache(maxsize=None)
def want(kind, w, h, dtype, amb=None, seed=0, **kw):
    """The restatement of one case, computed once and shared: (frame, tp, ambient).  amb: a tuple of four values, or None to estimate."""
    p = params(**kw)
    count = spec.count_of(p['quantile'], w, h, p['cell'])
    out, tp, used = spec.process(content(kind, w, h, p['cell'], seed).astype(dtype), None if amb is None else np.array(amb, dtype=f32), p['strength'], p['floor'],
                                 p['cell'], p['dark_radius'], p['radius'], p['eps'], count, spec.REC709 if p['weights'] is None else p['weights'])
    for a in (out, tp, used):
        a.setflags(write=False)
    return out, tp, used


def bits(a):
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def same_bits(got, expected, what):
    got = got.cpu().numpy()
    assert got.dtype == expected.dtype and got.shape == expected.shape, (what, got.dtype, expected.dtype, got.shape, expected.shape)
    bad = np.argwhere(bits(got) != bits(expected))
    if len(bad):
        print(f'{what}: {len(bad)} of {expected.size} values differ, first at {bad[0]}: got {got[tuple(bad[0])]!r} want {expected[tuple(bad[0])]!r}')
    assert len(bad) == 0, what


def make(td, dev, w, h, **kw):
    return td.Dehaze(dev, (w, h), **params(**kw))


def source(dev, kind, w, h, cell, dtype, seed=0):
    return torch.from_numpy(content(kind, w, h, cell, seed).astype(dtype)).to(dev)


def check_case(td, dev, kind, w, h, dtype, **kw):
    """An estimating call: frame, transmission and ambient light against the restatement."""
    dh = make(td, dev, w, h, **kw)
    src = source(dev, kind, w, h, dh.cell, dtype)
    out, t = dh.process(src, return_transmission=True)
    assert out.dtype == src.dtype and out.is_contiguous() and out.data_ptr() != src.data_ptr() and t.dtype == torch.float32
    out_w, t_w, amb_w = want(kind, w, h, dtype, **kw)
    what = (kind, w, h, dtype.__name__, kw)
    same_bits(dh.ambient, amb_w, (*what, 'ambient'))
    same_bits(t, t_w, (*what, 'transmission'))
    same_bits(out, out_w, what)
    return dh, src, out, t


# ------------------------------------------------------------------ 1. geometry
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('cases', [SMALLER_THAN_A_CELL, GRID_NARROWER_THAN_THE_WINDOWS, ONE_PAST_A_MULTIPLE, TILE_BOUNDARIES],
                         ids=['smaller_than_a_cell', 'grid_narrower_than_the_windows', 'one_past_a_multiple', 'tile_boundaries'])
def test_geometry_gives_the_restatements_bits(td, dev, cases, dtype):
    for w, h, cell, rd, rg in cases:
        check_case(td, dev, 'hazy', w, h, dtype, cell=cell, dark_radius=rd, radius=rg, quantile=0.05)


def test_the_table_meets_its_cases():
    """The rows do what their list's name says."""
    for w, h, cell, _, _ in SMALLER_THAN_A_CELL:
        assert w < cell and h < cell
    for w, h, cell, rd, rg in GRID_NARROWER_THAN_THE_WINDOWS:
        assert min(-(-w // cell), -(-h // cell)) <= min(rd, rg) and rd > 0 and rg > 0
    for w, h, cell, _, _ in ONE_PAST_A_MULTIPLE:
        assert w % cell == 1 and h % cell == 1
    assert {c[2] for c in ONE_PAST_A_MULTIPLE} == {c[2] for c in TILE_BOUNDARIES} == {2, 4, 8, 16}
    assert {c[3] for c in TILE_BOUNDARIES} >= {0, 4} and {c[4] for c in TILE_BOUNDARIES} >= {0, 8}
    assert any(w == 2 * 128 + 1 and h > 2 * 32 for w, h, *_ in TILE_BOUNDARIES)                       # dh_apply: a pixel past its tile
    assert any(w > 512 and h > 64 for w, h, *_ in TILE_BOUNDARIES)                                       # dh_cells, either storage type
    assert any(-(-w // cell) % 32 == 1 for w, h, cell, _, _ in TILE_BOUNDARIES)                         # dh_dark, dh_coeff: a cell past their tile along x
    assert any(-(-h // cell) % 32 == 1 and -(-h // cell) > 32 for w, h, cell, _, _ in TILE_BOUNDARIES)  # ... and along y


# ------------------------------------------------------------------ 2. parameters
@pytest.mark.parametrize('dtype', DTYPES)
def test_parameters_at_their_ends(td, dev, dtype):
    w, h = 130, 66
    for kw in (dict(strength=0.0), dict(strength=1.0), dict(floor=2.0 ** -6, strength=1.0), dict(floor=0.5, strength=1.0), dict(floor=1.0), dict(dark_radius=0, radius=0), dict(dark_radius=4, radius=8),
               dict(eps=1e-8), dict(eps=1.0), dict(weights=(0.25, 0.5, 0.25)), dict(weights=(0.0, 1.0, 0.0)), dict(weights=(1.5, 0.0, 0.3), cell=4)):
        check_case(td, dev, 'hazy', w, h, dtype, **kw)
    _, _, out, t = check_case(td, dev, 'hazy', w, h, dtype, floor=1.0)
    assert float(t.min()) == 1.0   # floor 1: nothing is divided
    _, t_w, _ = want('hazy', w, h, dtype, floor=0.5, strength=1.0)
    assert (t_w == 0.5).sum() > 500 and t_w.max() > 0.8   # the lower clamp is met too, and not everywhere


# ------------------------------------------------------------------ 3. selection
@pytest.mark.parametrize('dtype', DTYPES)
def test_selection(td, dev, dtype):
    w, h, cell = 130, 66, 4
    cells = 33 * 17
    # a constant frame: every cell ties, all are selected whatever K is
    for quantile in (0.01, 0.5):
        dh, *_ = check_case(td, dev, 'constant', w, h, dtype, cell=cell, quantile=quantile)
        assert float(dh.ambient[3]) == cells
    # K = 1 and K = CW*CH
    dh, *_ = check_case(td, dev, 'hazy', w, h, dtype, cell=cell, dark_radius=0, quantile=1e-6)   # (no window: the largest value is one cell's)
    assert dh.count == 1 and float(dh.ambient[3]) == 1
    dh, *_ = check_case(td, dev, 'hazy', w, h, dtype, cell=cell, quantile=1.0)
    assert dh.count == cells and float(dh.ambient[3]) == cells
    # ties exactly at the threshold: more cells than K are averaged
    for quantile in (0.1, 0.3, 0.6):
        dh, *_ = check_case(td, dev, 'ties', w, h, dtype, cell=cell, dark_radius=0, quantile=quantile)
        assert dh.count < float(dh.ambient[3]) < cells, (quantile, dh.count, dh.ambient)
    # a black frame: the ambient light is 0 and floors at 2^-10
    dh, _, out, t = check_case(td, dev, 'black', w, h, dtype, cell=cell)
    assert dh.ambient.tolist() == [0.0, 0.0, 0.0, float(cells)] and float(out.float().abs().max()) == 0.0


def test_select_takes_whole_rounds_and_a_rest(td, dev):
    """dh_select asks for 32 keys per thread at once while 32 * 1024 keys remain and goes key by key over the rest: a grid of one
    such round and a rest, with ties (K at the threshold's plateau) and without."""
    w, h, cell = 517, 260, 2
    assert 32 * 1024 < -(-w // cell) * -(-h // cell) < 2 * 32 * 1024
    for dtype in DTYPES:
        check_case(td, dev, 'hazy', w, h, dtype, cell=cell, quantile=0.01)
    dh, *_ = check_case(td, dev, 'ties', w, h, np.float32, cell=cell, dark_radius=0, quantile=0.3)
    assert dh.count < float(dh.ambient[3])


def test_cell_means_above_the_clamp_of_fix(td, dev):
    dh, *_ = check_case(td, dev, 'huge', 130, 66, np.float32, cell=8, quantile=0.05)
    assert dh.ambient[:3].tolist() == [65536.0] * 3 and float(dh.ambient[3]) >= dh.count
    check_case(td, dev, 'huge', 33, 17, np.float32, cell=2, quantile=0.3)


# ------------------------------------------------------------------ 4. content
@pytest.mark.parametrize('dtype', DTYPES)
def test_negative_samples(td, dev, dtype):
    for w, h, cell in ((130, 66, 8), (33, 17, 2)):
        check_case(td, dev, 'negative', w, h, dtype, cell=cell, quantile=0.05)
    assert (content('negative', 130, 66, 8) < 0).mean() > 0.3


def test_binary16_values_near_the_largest(td, dev):
    for cell, rd, rg in ((8, 1, 4), (2, 0, 1)):
        _, _, out, _ = check_case(td, dev, 'half_max', 130, 66, np.float16, cell=cell, dark_radius=rd, radius=rg, quantile=0.05)
        assert not torch.isnan(out).any()
    # an ambient light far below the samples: the result leaves binary16 and is rounded to infinity, as the restatement has it
    dh = make(td, dev, 130, 66, strength=1.0)
    src = source(dev, 'half_max', 130, 66, 8, np.float16)
    amb = (100.0, 100.0, 100.0, 0.0)
    out = dh.process(src, ambient=torch.tensor(amb, device=dev))
    same_bits(out, want('half_max', 130, 66, np.float16, amb=amb, strength=1.0)[0], 'half_max with a low ambient light')
    assert torch.isinf(out).any() and not torch.isnan(out).any()


@pytest.mark.parametrize('dtype', DTYPES)
def test_an_ambient_tensor_holding_nan_and_zero(td, dev, dtype):
    w, h = 130, 66
    dh = make(td, dev, w, h)
    src = source(dev, 'hazy', w, h, 8, dtype)
    for amb in ((float('nan'), 0.0, 0.7, 0.0), (0.0, 0.0, 0.0, 0.0), (float('nan'),) * 4, (-1.0, 2.0 ** -11, 0.9, 5.0)):
        out, t = dh.process(src, ambient=torch.tensor(amb, device=dev), return_transmission=True)
        out_w, t_w, _ = want('hazy', w, h, dtype, amb=amb)
        same_bits(t, t_w, (amb, 'transmission'))
        same_bits(out, out_w, amb)
        assert not torch.isnan(out).any() and not torch.isnan(t).any()


# ------------------------------------------------------------------ 5. calls
@pytest.mark.parametrize('dtype', DTYPES)
def test_a_given_ambient_against_the_estimate(td, dev, dtype):
    w, h = 257, 67
    dh, src, out, t = check_case(td, dev, 'hazy', w, h, dtype, quantile=0.05)
    amb = dh.estimate_ambient(src)
    assert amb.data_ptr() != dh.ambient.data_ptr() and amb.dtype == torch.float32 and tuple(amb.shape) == (4,) and amb.device == src.device
    same_bits(amb, want('hazy', w, h, dtype, quantile=0.05)[2], 'estimate_ambient')
    given, t_given = dh.process(src, ambient=amb, return_transmission=True)
    assert torch.equal(given.view(torch.uint8), out.view(torch.uint8)) and torch.equal(t_given.view(torch.int32), t.view(torch.int32))
    # return_transmission against transmission(), with and without the ambient light given
    for alone in (dh.transmission(src), dh.transmission(src, ambient=amb)):
        assert alone.dtype == torch.float32 and tuple(alone.shape) == (h, w) and torch.equal(alone.view(torch.int32), t.view(torch.int32))
    # another ambient light: the object's tensor stays what the last estimate left
    other = (0.6, 0.65, 0.7, 0.0)
    same_bits(dh.process(src, ambient=torch.tensor(other, device=dev)), want('hazy', w, h, dtype, amb=other)[0], 'another ambient light')
    same_bits(dh.ambient, want('hazy', w, h, dtype, quantile=0.05)[2], 'the ambient light of the object')


def test_set_ambient_fixes_it_and_none_estimates_again(td, dev):
    w, h = 130, 66
    dh, src, out, _ = check_case(td, dev, 'hazy', w, h, np.float32)
    ptr = dh.ambient.data_ptr()
    fixed = (0.75, 0.8, 0.85)
    dh.set_ambient(fixed)
    assert dh.ambient_is_fixed and dh.ambient.data_ptr() == ptr and dh.ambient.tolist()[:3] == [float(f32(v)) for v in fixed]
    same_bits(dh.process(src), want('hazy', w, h, np.float32, amb=(*fixed, 0.0))[0], 'a fixed ambient light')
    assert dh.ambient.tolist()[:3] == [float(f32(v)) for v in fixed]   # not estimated over
    dh.set_ambient(torch.tensor((0.5, 0.6, 0.7, 9.0), device=dev))
    same_bits(dh.process(src), want('hazy', w, h, np.float32, amb=(0.5, 0.6, 0.7, 9.0))[0], 'a fixed ambient light from a tensor')
    dh.set_ambient(None)
    assert not dh.ambient_is_fixed
    assert torch.equal(dh.process(src).view(torch.int32), out.view(torch.int32))
    same_bits(dh.ambient, want('hazy', w, h, np.float32)[2], 'estimated again')


def test_workspace_filled_with_nan_gives_the_same_bits(td, dev):
    for dtype, (w, h, cell, rd, rg) in zip(DTYPES, ((257, 67, 4, 2, 3), (130, 66, 16, 4, 8))):
        dh, src, out, t = check_case(td, dev, 'hazy', w, h, dtype, cell=cell, dark_radius=rd, radius=rg, quantile=0.05)
        assert len(dh._workspaces) == 1
        amb = dh.ambient.clone()
        for given in (None, amb):
            for buf in dh._workspaces._buffers.values():
                assert buf.numel() == dh.workspace_bytes()
                buf.fill_(0xFF)   # every float32 a NaN
            dh.ambient.fill_(float('nan'))
            again, t_again = dh.process(src, ambient=given, return_transmission=True)
            assert torch.equal(again.view(torch.uint8), out.view(torch.uint8)) and torch.equal(t_again.view(torch.int32), t.view(torch.int32))
        for buf in dh._workspaces._buffers.values():
            buf.fill_(0xFF)
        assert torch.equal(dh.estimate_ambient(src).view(torch.int32), amb.view(torch.int32))


def test_two_streams_each_with_its_own_workspace(td, dev):
    w, h = 257, 67
    dh = make(td, dev, w, h, quantile=0.05)
    src = source(dev, 'hazy', w, h, 8, np.float32)
    amb = dh.estimate_ambient(src)
    one = dh.process(src, ambient=amb)
    s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    for s in (s1, s2):
        s.wait_stream(torch.cuda.current_stream())
    outs = []
    for _ in range(3):
        with torch.cuda.stream(s1):
            oa = dh.process(src, ambient=amb)
        with torch.cuda.stream(s2):
            ob = dh.process(src, ambient=amb)
        outs.append((oa, ob))
    torch.cuda.synchronize()
    assert len(dh._workspaces) == 3   # the stream of construction and the two
    for oa, ob in outs:
        assert torch.equal(oa.view(torch.int32), one.view(torch.int32)) and torch.equal(ob.view(torch.int32), one.view(torch.int32))
    same_bits(one, want('hazy', w, h, np.float32, quantile=0.05)[0], 'two streams')


# ------------------------------------------------------------------ 6. graphs
def test_graph_follows_a_rewritten_ambient(td, dev):
    """An object built on the side stream and captured there without a warm-up call (ambient and workspace exist since construction);
    a replay equals the restatement, and after the tensor is rewritten the restatement of the new ambient light."""
    w, h = 130, 66
    first, second = (0.8, 0.85, 0.9, 0.0), (0.5, float('nan'), 0.7, 3.0)
    src = source(dev, 'hazy', w, h, 8, np.float16)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        dh = make(td, dev, w, h)
        amb = torch.tensor(first, device=dev)
        with torch.cuda.graph(graph, stream=stream):
            captured, captured_t = dh.process(src, ambient=amb, return_transmission=True)
        graph.replay()
        stream.synchronize()
        same_bits(captured, want('hazy', w, h, np.float16, amb=first)[0], 'replay')
        same_bits(captured_t, want('hazy', w, h, np.float16, amb=first)[1], 'replayed transmission')
        amb.copy_(torch.tensor(second, device=dev))
        graph.replay()
        stream.synchronize()
        same_bits(captured, want('hazy', w, h, np.float16, amb=second)[0], 'replay after the ambient light was rewritten')
        same_bits(captured_t, want('hazy', w, h, np.float16, amb=second)[1], 'replayed transmission after the ambient light was rewritten')


def test_graph_of_an_estimating_call_follows_new_pixels(td, dev):
    w, h = 257, 67
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        dh = make(td, dev, w, h, quantile=0.05)
        buffer = source(dev, 'hazy', w, h, 8, np.float32).clone()
        with torch.cuda.graph(graph, stream=stream):
            captured = dh.process(buffer)
        for seed in (0, 1, 0):
            buffer.copy_(source(dev, 'hazy', w, h, 8, np.float32, seed))
            graph.replay()
            stream.synchronize()
            out_w, _, amb_w = want('hazy', w, h, np.float32, seed=seed, quantile=0.05)
            same_bits(captured, out_w, ('replay', seed))
            same_bits(dh.ambient, amb_w, ('replayed ambient', seed))
    assert not np.array_equal(want('hazy', w, h, np.float32, seed=0, quantile=0.05)[2], want('hazy', w, h, np.float32, seed=1, quantile=0.05)[2])


# ------------------------------------------------------------------ 7. views
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
    for w, h, cell in ((130, 66, 8), (257, 67, 2)):
        dh = make(td, dev, w, h, cell=cell, quantile=0.05)
        src = source(dev, 'hazy', w, h, cell, dtype)
        out_w, t_w, amb_w = want('hazy', w, h, dtype, cell=cell, quantile=0.05)
        for offset in (1, 2, 3):
            view = at_offset(src, offset)
            assert view.data_ptr() % 16 != 0
            out, t = dh.process(view, return_transmission=True)
            same_bits(out, out_w, (w, h, offset))
            same_bits(t, t_w, (w, h, offset, 'transmission'))
            same_bits(dh.ambient, amb_w, (w, h, offset, 'ambient'))
    wide = torch.zeros((66, 140, 3), dtype=src.dtype, device=dev)
    dh = make(td, dev, 130, 66)
    with pytest.raises(RuntimeError, match='contiguous'):
        dh.process(wide[:, :130])
    with pytest.raises(RuntimeError, match='contiguous'):
        dh.process(torch.zeros((130, 66, 3), dtype=src.dtype, device=dev).transpose(0, 1))
    with pytest.raises(RuntimeError, match='expected'):
        dh.process(wide)
    with pytest.raises(ValueError, match='channels must be 3'):
        dh.transmission(torch.zeros((66, 130, 1), dtype=src.dtype, device=dev))
    with pytest.raises(ValueError, match='float32 or float16'):
        dh.process(torch.zeros((66, 130, 3), dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match='ambient must be'):
        dh.process(torch.zeros((66, 130, 3), dtype=src.dtype, device=dev), ambient=torch.zeros(3, device=dev))
    with pytest.raises(RuntimeError, match='ambient is on'):
        dh.process(torch.zeros((66, 130, 3), dtype=src.dtype, device=dev), ambient=torch.zeros(4))


def test_outputs_at_odd_offsets_through_the_c_entry_point(td, dev):
    from torch_darktable._native import lib

    for (w, h, cell, rd, rg), dtype, tag in (((257, 67, 4, 2, 3), np.float32, 0), ((130, 66, 8, 1, 4), np.float16, 1)):
        dh = make(td, dev, w, h, cell=cell, dark_radius=rd, radius=rg, quantile=0.05)
        src = source(dev, 'hazy', w, h, cell, dtype)
        n = w * h
        pool = torch.zeros(3 * n + 40, dtype=src.dtype, device=dev)
        t_pool = torch.zeros(n + 40, dtype=torch.float32, device=dev)
        amb_pool = torch.zeros(8, dtype=torch.float32, device=dev)
        out, t, amb = pool[3:3 + 3 * n], t_pool[1:1 + n], amb_pool[1:5]
        ws = torch.zeros(dh.workspace_bytes() + 16, dtype=torch.uint8, device=dev)[5:]
        weights = (ctypes.c_float * 3)(*dh.weights)
        stream = torch.cuda.current_stream().cuda_stream
        rc = lib.tdk_dehaze(src.data_ptr(), out.data_ptr(), t.data_ptr(), ws.data_ptr(), amb.data_ptr(), w, h, tag, cell, rd, rg, dh.count, dh.eps, dh.strength, dh.floor,
                            weights, 0, stream)
        assert rc == 0, lib.tdk_last_error()
        torch.cuda.synchronize()
        out_w, t_w, amb_w = want('hazy', w, h, dtype, cell=cell, dark_radius=rd, radius=rg, quantile=0.05)
        same_bits(out.view(h, w, 3), out_w, (w, h, 'frame'))
        same_bits(t.view(h, w), t_w, (w, h, 'transmission'))
        same_bits(amb, amb_w, (w, h, 'ambient'))
        assert float(pool[:3].float().abs().max()) == 0 and float(pool[3 + 3 * n:].float().abs().max()) == 0   # nothing written outside
        assert float(t_pool[:1].abs().max()) == 0 and float(t_pool[1 + n:].abs().max()) == 0
        assert float(amb_pool[:1].abs().max()) == 0 and float(amb_pool[5:].abs().max()) == 0
        # the estimate alone, and a transmission-only call that reads it
        amb_pool.zero_(), t_pool.zero_()
        assert lib.tdk_dehaze_ambient(src.data_ptr(), amb.data_ptr(), ws.data_ptr(), w, h, tag, cell, rd, dh.count, 0, stream) == 0, lib.tdk_last_error()
        assert lib.tdk_dehaze(src.data_ptr(), None, t.data_ptr(), ws.data_ptr(), amb.data_ptr(), w, h, tag, cell, rd, rg, 0, dh.eps, dh.strength, dh.floor, weights, 0,
                              stream) == 0, lib.tdk_last_error()
        torch.cuda.synchronize()
        same_bits(amb, amb_w, (w, h, 'ambient alone'))
        same_bits(t.view(h, w), t_w, (w, h, 'transmission alone'))
        assert float(amb_pool[:1].abs().max()) == 0 and float(amb_pool[5:].abs().max()) == 0


# ------------------------------------------------------------------ 8. pipeline
def _processor(td, dev, w, h, **kw):
    from torch_darktable.pipeline import Debayer, ImageProcessingSettings, ImageProcessor, ImageTransform, ToneMapper
    settings = ImageProcessingSettings(moving_average=0.3, postprocess=False, enable_denoise=True, enable_bilateral=True, tone_mapping=ToneMapper.reinhard,
                                       debayer=Debayer.bilinear)
    return ImageProcessor((w, h), td.BayerPattern.RGGB, td.PackedFormat.Packed12, settings, dev, (1.9, 1.0, 1.6), transforms=ImageTransform.none, **kw)


@pytest.mark.parametrize('storage', [torch.float32, torch.float16])
def test_pipeline_runs_it_behind_color_and_in_front_of_the_tone_equalizer(td, dev, storage):
    w, h = 128, 96
    scene = content('hazy', w, h)[..., 1]
    packed = {name: td.encode12_float(torch.from_numpy(np.clip(np.roll(scene, k, axis=1), 0, 1)).to(dev).reshape(-1)) for k, name in enumerate(('left', 'right'))}
    dh = td.Dehaze(dev, (w, h), quantile=0.05)
    te = td.ToneEqualizer(dev, (w, h), gains_ev=(3, 3, 3, 2.5, 2, 1.5, 1, 0.5, 0), cell=8, radius=2)
    color = td.ColorLUT(dev, matrix=((0.9, 0.1, 0.0), (0.05, 0.9, 0.05), (0.0, 0.2, 0.8)))

    with_stage = _processor(td, dev, w, h, storage_dtype=storage, color=color)
    assert with_stage.dehaze is None
    with_stage.dehaze, with_stage.tone_equalizer = dh, te
    assert with_stage.dehaze is dh
    got = with_stage.process_image_set(packed)

    # the chain composed by hand: demosaic, colour, haze removal, tone equalizer, and on from the frames with a processor that has neither
    by_hand = _processor(td, dev, w, h, storage_dtype=storage)
    frames = [te.process(dh.process(color.process(by_hand.load_image(b)))) for b in packed.values()]
    assert frames[0].dtype == storage
    expected = by_hand._process_frames(list(packed), frames, resized=False)
    assert sorted(got) == sorted(expected) == ['left', 'right']
    for name in packed:
        assert got[name].dtype == torch.uint8 and torch.equal(got[name], expected[name]), name
    assert torch.equal(with_stage.bounds, by_hand.bounds) and torch.equal(with_stage.metrics, by_hand.metrics)   # they saw the stage's result
    # ... and not the other order
    swapped = [dh.process(te.process(color.process(by_hand.load_image(b)))) for b in packed.values()]
    assert not torch.equal(swapped[0], frames[0])

    # None: the processor that never had one, and not the stage's result
    without = _processor(td, dev, w, h, storage_dtype=storage, color=color)
    without.tone_equalizer = te
    never = without.process_image_set(packed)
    cleared = _processor(td, dev, w, h, storage_dtype=storage, color=color)
    cleared.tone_equalizer, cleared.dehaze = te, dh
    cleared.dehaze = None
    again = cleared.process_image_set(packed)
    for name in packed:
        assert torch.equal(again[name], never[name]) and not torch.equal(got[name], never[name])
