"""GPU: the raw stage (torch_darktable.RawPrepare, include/tdk_hip_raw.h) against the float32 restatement of its specification,
`raw_prepare_ref` of tests/test_rawprepare_spec.py.

The criterion is bit equality of the result (float32 and float16) and equality of the mask: the restatement uses only correctly
rounded float32 operations in the order of the specification, and the library is built without contraction.  A differing bit is a
finding to explain, not a tolerance to widen.  Floats are compared as bit patterns, so NaN positions and the sign of zero count.

The workgroup tile is 128 x 16 pixels and a thread owns 8 adjacent ones.  Shapes (width x height): 70 x 46 and 134 x 34 (partial
tiles, rows that are no multiple of 8: the per-element loads and stores), 136 x 36 and 264 x 52 (rows of whole groups of 8: the
vector loads and stores; 264 x 52 has a tile whose apron lies inside the frame in x, 3 tile columns and 4 tile rows) and 24 x 20
(narrower than a tile).  Every parity check prints its figures (pytest -s) before it asserts."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location('rawprepare_spec', Path(__file__).resolve().parent / 'test_rawprepare_spec.py')
spec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(spec)
raw_prepare_ref, pack12, scale_of, smooth_field, PATTERNS = spec.raw_prepare_ref, spec.pack12, spec.scale_of, spec.smooth_field, spec.PATTERNS

TILE_W, TILE_H = 128, 16   # csrc/rawprepare.hip
SHAPES = [(70, 46), (134, 34), (136, 36), (264, 52), (24, 20)]
BLACK4 = [240.0, 256.0, 250.0, 260.0]
GAINS = [1.9, 1.0, 1.6]
TORCH = {'float32': torch.float32, 'float16': torch.float16}
NP = {'float32': np.float32, 'float16': np.float16}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a visible MI355X'
    return torch.device('cuda', 0)


def bits(a):
    return a.view({4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def at_offset(t, elements):
    """A contiguous copy of CUDA tensor `t` that starts `elements` elements into a larger buffer."""
    pool = torch.zeros(t.numel() + elements + 16, dtype=t.dtype, device=t.device)
    v = pool[elements:elements + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() == pool.data_ptr() + elements * t.element_size()
    return v


def defect_sites(w, h):
    """Hot and dead sites on the frame's edges and corners (rows and columns 0, 1, h-2, h-1), on both sides of every tile boundary,
    two hot ones next to each other, and a few in the open."""
    hot, dead = set(), set()
    rows = [0, 1, h - 2, h - 1] + [r for b in range(TILE_H, h, TILE_H) for r in (b - 2, b - 1, b, b + 1)]
    cols = [0, 1, w - 2, w - 1] + [c for b in range(TILE_W, w, TILE_W) for c in (b - 2, b - 1, b, b + 1)]
    k = 0
    for r in rows:
        for c in sorted({0, 1, 7, w // 2, w - 2, w - 1} | set(cols)):
            (hot if k % 2 == 0 else dead).add((r, c))
            k += 1
    for c in cols:
        for r in (5, h // 2, h - 6):
            (hot if k % 2 == 0 else dead).add((r, c))
            k += 1
    for r in range(3, h - 3, 4):   # in the open, four same-colour neighbours each
        (hot if k % 2 == 0 else dead).add((r, 3 + (r * 37) % (w - 6)))
        k += 1
    hot |= {(h // 2, w // 2), (h // 2, w // 2 + 2)}
    dead -= hot
    return sorted(hot), sorted(dead)


def codes_frame(w, h, seed, defects=True):
    """12-bit codes of a dark smooth field above a pedestal of about 250, with planted defects."""
    L = smooth_field(h, w, seed)
    codes = np.rint(250.0 + L * 3800.0).astype(np.int64)
    if defects:
        hot, dead = defect_sites(w, h)
        for r, c in hot:
            codes[r, c] = 4090
        for r, c in dead:
            codes[r, c] = 252
    return np.clip(codes, 0, 4095)


def shading_grid(gw, gh, seed):
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.linspace(-1, 1, gh), np.linspace(-1, 1, gw), indexing='ij')
    g = 1.0 + 0.6 * (x * x + y * y)[:, :, None] * np.array([1.0, 0.9, 0.95, 1.1]) + 0.02 * rng.random((gh, gw, 4))
    return g.astype(np.float32)


def densest(w, h):
    return min((w - 1) // 4 + 1, 257), min((h - 1) // 4 + 1, 257)


def make_input(codes, form, black, white):
    """(numpy raw values as the restatement takes them, numpy array to upload, black, white in the input's units)."""
    if form in ('Packed12', 'Packed12_IDS'):
        return codes, pack12(codes, form == 'Packed12_IDS'), black, white
    if form == 'uint16':
        return codes, codes.astype(np.uint16), black, white
    # float input in its own units; the restatement takes the stored floats (binary16 rounds codes above 2048)
    x = (codes / 4096.0).astype(NP[form])
    return x.astype(np.float32), x, [b / 4096.0 for b in np.broadcast_to(np.asarray(black, dtype=np.float64).reshape(-1), (4,))], white / 4096.0


def run_case(td, dev, w, h, pattern, form, out_dtype, black=BLACK4, white=4095.0, hot=False, dead=False, grid=None, wb=False, clip=True, min_count=3,
             offset=0, seed=1, want_mask=None, codes=None, what=''):
    codes = codes_frame(w, h, seed) if codes is None else codes
    raw, upload, black_u, white_u = make_input(codes, form, black, white)
    shading = shading_grid(*grid, seed + 1) if grid else None
    gains = np.array(GAINS, dtype=np.float32) if wb else None
    want_mask = (hot or dead) if want_mask is None else want_mask
    rp = td.RawPrepare(dev, (w, h), td.BayerPattern[pattern], black=black_u, white=white_u, shading=None if shading is None else torch.from_numpy(shading),
                       hot=hot, dead=dead, threshold=0.02, ratio=0.5, min_count=min_count, clip=clip)
    ref_black, ref_scale = scale_of(black_u, white_u)
    assert np.array_equal(rp.black, ref_black) and np.array_equal(rp.scale, ref_scale)
    want, want_m = raw_prepare_ref(raw, PATTERNS[pattern], ref_black, ref_scale, hot=hot, dead=dead, threshold=0.02, ratio=0.5, min_count=min_count,
                                   shading=shading, gains=gains, clip=clip, out_dtype=NP[out_dtype])
    t = torch.from_numpy(upload).to(dev)
    if offset:
        t = at_offset(t, offset)
    mask = torch.full((h, w), 77, dtype=torch.uint8, device=dev) if want_mask else None
    if want_mask and offset:
        mask = at_offset(mask, offset)
    g = torch.from_numpy(gains).to(dev) if wb else None
    if form in ('Packed12', 'Packed12_IDS'):
        out = rp.process_packed(t, td.PackedFormat[form], white_balance=g, out_dtype=TORCH[out_dtype], mask_out=mask)
    else:
        out = rp.process(t, white_balance=g, out_dtype=TORCH[out_dtype], mask_out=mask)
    assert tuple(out.shape) == (h, w) and out.dtype == TORCH[out_dtype] and out.is_contiguous()
    got = out.cpu().numpy()
    differ = bits(got) != bits(want)
    worst = float(np.nanmax(np.abs(got.astype(np.float64) - want.astype(np.float64))))
    line = f'rawprepare {what}{w}x{h} {pattern} {form} -> {out_dtype}: {int(differ.sum())} of {differ.size} values differ in a bit, largest difference {worst:.3e}'
    if want_mask:
        got_m = mask.cpu().numpy()
        line += f'; mask: {int((got_m != want_m).sum())} differ, {int((want_m == 1).sum())} hot, {int((want_m == 2).sum())} dead'
    print(line)
    assert not differ.any(), line
    if want_mask:
        assert np.array_equal(got_m, want_m), line
    return got, want_m


# ------------------------------------------------------------------ 1. identity and white balance against today's two kernels
@pytest.mark.parametrize('form', ['Packed12', 'Packed12_IDS'])
@pytest.mark.parametrize('size', [(70, 46), (136, 36)])
def test_identity_equals_decode12_float(td, dev, size, form):
    w, h = size
    rng = np.random.default_rng(2)
    codes = rng.integers(0, 4096, (h, w))
    data = torch.from_numpy(pack12(codes, form == 'Packed12_IDS')).to(dev)
    fmt = td.PackedFormat[form]
    rp = td.RawPrepare(dev, (w, h), td.BayerPattern.RGGB, clip=False)
    assert rp.lds_bytes() == 0   # the plain streaming form
    want = td.decode12_float(data, ids_format=form == 'Packed12_IDS').view(h, w)
    got = rp.process_packed(data, fmt)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert np.array_equal(got.cpu().numpy(), codes.astype(np.float32) * (np.float32(1.0) / np.float32(4095.0)))
    half = rp.process_packed(data, fmt, out_dtype=torch.float16)
    assert torch.equal(half.view(torch.int16), td.decode12_half(data, ids_format=form == 'Packed12_IDS').view(h, w).view(torch.int16))


@pytest.mark.parametrize('pattern', list(PATTERNS))
@pytest.mark.parametrize('form', ['Packed12', 'Packed12_IDS'])
def test_white_balance_only_equals_apply_white_balance(td, dev, pattern, form):
    w, h = 136, 36
    rng = np.random.default_rng(3)
    codes = rng.integers(0, 4096, (h, w))
    data = torch.from_numpy(pack12(codes, form == 'Packed12_IDS')).to(dev)
    gains = torch.tensor(GAINS, device=dev)
    rp = td.RawPrepare(dev, (w, h), td.BayerPattern[pattern])
    want = td.apply_white_balance(td.decode12_float(data, ids_format=form == 'Packed12_IDS').view(h, w), gains, td.BayerPattern[pattern])
    got = rp.process_packed(data, td.PackedFormat[form], white_balance=gains)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert (got == 1).any() and (got < 1).any()


# ------------------------------------------------------------------ 2. the restatement: patterns x forms x output types, all steps
@pytest.mark.parametrize('out_dtype', ['float32', 'float16'])
@pytest.mark.parametrize('form', ['Packed12', 'Packed12_IDS'])
@pytest.mark.parametrize('pattern', list(PATTERNS))
def test_all_steps_packed_every_pattern(td, dev, pattern, form, out_dtype):
    for w, h in ((70, 46), (136, 36)):
        _, m = run_case(td, dev, w, h, pattern, form, out_dtype, hot=True, dead=True, grid=(17, 9), wb=True, what='all steps ')
        assert (m == 1).sum() > 10 and (m == 2).sum() > 10


@pytest.mark.parametrize('out_dtype', ['float32', 'float16'])
@pytest.mark.parametrize('form', ['uint16', 'float32', 'float16'])
def test_all_steps_unpacked_inputs(td, dev, form, out_dtype):
    for w, h in ((134, 34), (264, 52)):
        run_case(td, dev, w, h, 'GRBG', form, out_dtype, hot=True, dead=True, grid=(17, 9) if h > 34 else (17, 8), wb=True, what='all steps ')


@pytest.mark.parametrize('size', SHAPES)
def test_all_steps_every_shape(td, dev, size):
    w, h = size
    grid = (min(17, densest(w, h)[0]), min(9, densest(w, h)[1]))
    run_case(td, dev, w, h, 'BGGR', 'Packed12', 'float32', hot=True, dead=True, grid=grid, wb=True, what='shape ')
    run_case(td, dev, w, h, 'BGGR', 'Packed12', 'float16', hot=True, dead=True, grid=grid, wb=False, clip=False, what='shape, no clip ')


# ------------------------------------------------------------------ 3. each step alone
STEPS = {
    'black_white': dict(),
    'black_white_clip_off': dict(clip=False),
    'hot': dict(hot=True), 'dead': dict(dead=True), 'hot_dead': dict(hot=True, dead=True), 'hot_min4': dict(hot=True, min_count=4),
    'dead_min1': dict(dead=True, min_count=1),
    'mask_without_rules': dict(want_mask=True),
    'shading': dict(grid=(17, 9)), 'white_balance': dict(wb=True),
}


@pytest.mark.parametrize('step', list(STEPS))
def test_each_step_alone(td, dev, step):
    for (w, h), form in (((70, 46), 'Packed12'), ((264, 52), 'Packed12_IDS'), ((136, 36), 'uint16')):
        _, m = run_case(td, dev, w, h, 'RGGB', form, 'float32', what=step + ' ', **STEPS[step])
        if step == 'mask_without_rules':
            assert not m.any()


def test_defects_on_edges_corners_and_tile_boundaries(td, dev):
    """What the planted sites of every case are: on rows and columns 0, 1, n-2, n-1, on both sides of every tile boundary.  A corner
    site (two neighbours) stays at min_count = 3, an edge site (three) goes, and sites across a tile boundary are decided alike."""
    w, h = 264, 52
    hot, dead = defect_sites(w, h)
    for r in (0, 1, h - 2, h - 1):
        for c in (0, 1, w - 2, w - 1):
            assert (r, c) in hot or (r, c) in dead
    for b in (TILE_W, 2 * TILE_W):
        assert all(any((r, c) in hot or (r, c) in dead for r in range(h)) for c in (b - 2, b - 1, b, b + 1))
    _, m = run_case(td, dev, w, h, 'RGGB', 'Packed12', 'float32', hot=True, dead=True, what='planted ')
    for r in (0, 1, h - 2, h - 1):
        for c in (0, 1, w - 2, w - 1):
            assert m[r, c] == 0, (r, c)                       # two neighbours
    assert m[0, w // 2] in (1, 2) and m[1, 7] in (1, 2)        # three neighbours
    assert m[5, TILE_W - 2] != 0 and m[5, TILE_W] != 0 and m[TILE_H - 1, w // 2] != 0 and m[TILE_H, w // 2] != 0
    assert m[h // 2, w // 2] == 1 and m[h // 2, w // 2 + 2] == 1   # two hot sites side by side: three members each
    _, m4 = run_case(td, dev, w, h, 'RGGB', 'Packed12', 'float32', hot=True, dead=True, min_count=4, what='planted, min_count 4 ')
    assert m4[h // 2, w // 2] == 0 and m4[h // 2, w // 2 + 2] == 0 and m4[0, w // 2] == 0 and m4[1, 7] == 0


def test_nan_and_negative_input(td, dev):
    """float32 input with NaN, infinities and values below black: a NaN is never corrected and never counts, the clamp turns it to 0."""
    w, h = 136, 36
    x = smooth_field(h, w, 9)
    x[4, 8], x[4, 10], x[20, 127], x[20, 129], x[21, 3], x[30, 64] = np.nan, 0.99, np.nan, 0.99, -0.5, np.inf
    for clip in (False, True):
        rp = td.RawPrepare(dev, (w, h), td.BayerPattern.RGGB, black=0.05, white=1.0, hot=True, dead=True, min_count=4, clip=clip)
        mask = torch.zeros((h, w), dtype=torch.uint8, device=dev)
        got = rp.process(torch.from_numpy(x).to(dev), mask_out=mask).cpu().numpy()
        want, want_m = raw_prepare_ref(x, PATTERNS['RGGB'], rp.black, rp.scale, hot=True, dead=True, min_count=4, clip=clip)
        assert np.array_equal(bits(got), bits(want)) and np.array_equal(mask.cpu().numpy(), want_m)
        assert want_m[4, 8] == 0 and want_m[4, 10] == 0 and (np.isnan(want[4, 8]) if not clip else want[4, 8] == 0)


# ------------------------------------------------------------------ 4. grids
@pytest.mark.parametrize('size', [(70, 46), (264, 52)])
@pytest.mark.parametrize('grid', ['2x2', '17x9', 'densest'])
def test_shading_grids(td, dev, size, grid):
    w, h = size
    g = {'2x2': (2, 2), '17x9': (17, 9), 'densest': densest(w, h)}[grid]
    for out_dtype in ('float32', 'float16'):
        run_case(td, dev, w, h, 'GBRG', 'Packed12', out_dtype, grid=g, clip=False, what=f'grid {g[0]}x{g[1]} ')
    run_case(td, dev, w, h, 'GBRG', 'uint16', 'float32', hot=True, dead=True, grid=g, what=f'grid {g[0]}x{g[1]} + defects ')


def test_shading_from_rgb_expands_to_cfa_positions(td, dev):
    rgb = torch.arange(2 * 3 * 3, dtype=torch.float32).view(2, 3, 3)
    for name, word in PATTERNS.items():
        g4 = td.RawPrepare.shading_from_rgb(rgb, td.BayerPattern[name])
        assert tuple(g4.shape) == (2, 3, 4)
        for p in range(4):
            assert torch.equal(g4[:, :, p], rgb[:, :, (word >> (2 * p)) & 3])


# ------------------------------------------------------------------ 5. misaligned frames, determinism, capture
@pytest.mark.parametrize('form', ['Packed12', 'uint16', 'float32', 'float16'])
@pytest.mark.parametrize('out_dtype', ['float32', 'float16'])
def test_frames_one_element_into_a_buffer(td, dev, form, out_dtype):
    for kw in (dict(hot=True, dead=True, grid=(17, 9), wb=True), dict(wb=True)):
        run_case(td, dev, 136, 36, 'RGGB', form, out_dtype, offset=1, what='offset view ', **kw)


def test_output_one_element_into_a_buffer(td, dev):
    """The library call on an output (and mask) that starts one element into its buffer: the per-element stores."""
    import ctypes

    from torch_darktable._native import lib

    w, h = 136, 36
    codes = codes_frame(w, h, 5)
    black, scale = scale_of(BLACK4, 4095.0)
    data = torch.from_numpy(pack12(codes, False)).to(dev)
    gains = torch.tensor(GAINS, device=dev)
    c_black, c_scale = (ctypes.c_float * 4)(*black.tolist()), (ctypes.c_float * 4)(*scale.tolist())
    for tag, dtype in ((0, torch.float32), (1, torch.float16)):
        for defects in (0, 3):
            pool = torch.zeros(w * h + 17, dtype=dtype, device=dev)
            mpool = torch.zeros(w * h + 17, dtype=torch.uint8, device=dev)
            out, mask = pool[1:1 + w * h].view(h, w), mpool[1:1 + w * h].view(h, w)
            rc = lib.tdk_raw_prepare(data.data_ptr(), 0, out.data_ptr(), tag, mask.data_ptr() if defects else None, w, h, PATTERNS['RGGB'],
                                     ctypes.addressof(c_black), ctypes.addressof(c_scale), defects, 0.02, 0.5, 3, None, 0, 0, gains.data_ptr(), 1,
                                     torch.cuda.current_stream().cuda_stream)
            assert rc == 0, lib.tdk_last_error()
            want, want_m = raw_prepare_ref(codes, PATTERNS['RGGB'], black, scale, hot=defects != 0, dead=defects != 0, gains=np.array(GAINS, np.float32),
                                           out_dtype=NP['float32' if tag == 0 else 'float16'])
            assert np.array_equal(bits(out.cpu().numpy()), bits(want)) and np.array_equal(mask.cpu().numpy(), want_m)
            assert pool[0] == 0 and pool[1 + w * h:].eq(0).all() and mpool[0] == 0 and mpool[1 + w * h:].eq(0).all()


def test_two_calls_give_equal_bits(td, dev):
    w, h = 264, 52
    data = torch.from_numpy(pack12(codes_frame(w, h, 6), False)).to(dev)
    rp = td.RawPrepare(dev, (w, h), td.BayerPattern.RGGB, black=BLACK4, hot=True, dead=True, shading=torch.from_numpy(shading_grid(17, 9, 1)))
    gains = torch.tensor(GAINS, device=dev)
    for dtype in (torch.float32, torch.float16):
        ma, mb = torch.zeros((h, w), dtype=torch.uint8, device=dev), torch.ones((h, w), dtype=torch.uint8, device=dev)
        a = rp.process_packed(data, white_balance=gains, out_dtype=dtype, mask_out=ma)
        b = rp.process_packed(data, white_balance=gains, out_dtype=dtype, mask_out=mb)
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)) and torch.equal(ma, mb)


@pytest.mark.parametrize('out_dtype', ['float32', 'float16'])
def test_graph_capture_from_the_first_call(td, dev, out_dtype):
    """A fresh object captured on one stream without a warm-up call; the replay equals the eager result bit for bit, also after the
    input buffer's contents change."""
    w, h = 264, 52
    shading = shading_grid(17, 9, 2)
    rp = td.RawPrepare(dev, (w, h), td.BayerPattern.GRBG, black=BLACK4, hot=True, dead=True, shading=torch.from_numpy(shading))
    codes = codes_frame(w, h, 7)
    x = torch.from_numpy(pack12(codes, False)).to(dev)
    gains = torch.tensor(GAINS, device=dev)
    mask = torch.zeros((h, w), dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            captured = rp.process_packed(x, white_balance=gains, out_dtype=TORCH[out_dtype], mask_out=mask)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, rp.process_packed(x, white_balance=gains, out_dtype=TORCH[out_dtype]))
    codes = codes_frame(w, h, 8)
    x.copy_(torch.from_numpy(pack12(codes, False)).to(dev))
    graph.replay()
    torch.cuda.synchronize()
    black, scale = scale_of(BLACK4, 4095.0)
    want, want_m = raw_prepare_ref(codes, PATTERNS['GRBG'], black, scale, hot=True, dead=True, shading=shading, gains=np.array(GAINS, np.float32),
                                   out_dtype=NP[out_dtype])
    assert np.array_equal(bits(captured.cpu().numpy()), bits(want)) and np.array_equal(mask.cpu().numpy(), want_m)


# ------------------------------------------------------------------ 6. the pipeline
def _processor(td, dev, size, fmt, wb, debayer, rp=None):
    from torch_darktable.pipeline.config import Debayer, ImageProcessingSettings
    from torch_darktable.pipeline.image_processor import ImageProcessor

    settings = ImageProcessingSettings(debayer=Debayer[debayer])
    return ImageProcessor(size, td.BayerPattern.RGGB, fmt, settings, dev, wb, raw_correction=rp)


@pytest.mark.parametrize('debayer', ['rcd', 'bilinear'])
def test_image_processor_with_raw_correction(td, dev, debayer):
    w, h = 256, 192
    codes = codes_frame(w, h, 10)
    data = torch.from_numpy(pack12(codes, False)).to(dev)
    fmt, wb = td.PackedFormat.Packed12, (1.9, 1.0, 1.6)
    rp = td.RawPrepare(dev, (w, h), td.BayerPattern.RGGB, black=BLACK4, hot=True, dead=True, shading=torch.from_numpy(shading_grid(17, 9, 3)))
    got = _processor(td, dev, (w, h), fmt, wb, debayer, rp).process(data, 'cam')
    # by hand: the corrected, balanced mosaic into the demosaic of a processor that has no white balance of its own
    manual = _processor(td, dev, (w, h), fmt, None, debayer)
    gains = torch.tensor(wb, device=dev)
    manual.load_image = lambda b: manual.debayer(rp.process_packed(b, fmt, white_balance=gains)).to(manual.storage_dtype)
    want = manual.process(data, 'cam')
    assert got.dtype == torch.uint8 and tuple(got.shape) == (h, w, 3) and torch.equal(got, want)
    # the correction changes the picture, and raw_correction=None is today's chain
    plain = _processor(td, dev, (w, h), fmt, wb, debayer).process(data, 'cam')
    assert not torch.equal(plain, got)
    none = _processor(td, dev, (w, h), fmt, wb, debayer, None)
    by_hand = none.debayer(none.load_bytes(data))
    assert torch.equal(none.load_image(data), by_hand)
    assert torch.equal(none.process(data, 'cam'), plain)
    # with the correction at identity the processor gives today's picture
    ident = td.RawPrepare(dev, (w, h), td.BayerPattern.RGGB)
    assert torch.equal(_processor(td, dev, (w, h), fmt, wb, debayer, ident).process(data, 'cam'), plain)
    with pytest.raises(ValueError, match='raw_correction'):
        _processor(td, dev, (w, h), fmt, wb, debayer, td.RawPrepare(dev, (w + 2, h), td.BayerPattern.RGGB))


def test_error_handling(td, dev):
    rp = td.RawPrepare(dev, (64, 48), td.BayerPattern.RGGB)
    with pytest.raises(RuntimeError, match='shape'):
        rp.process(torch.zeros(48, 60, device=dev))
    with pytest.raises(RuntimeError, match='uint16, float32 or float16'):
        rp.process(torch.zeros(48, 64, device=dev, dtype=torch.float64))
    with pytest.raises(RuntimeError, match='contiguous'):
        rp.process(torch.zeros(64, 48, device=dev).t())
    with pytest.raises(RuntimeError, match='bytes'):
        rp.process_packed(torch.zeros(64 * 48 * 3 // 2 + 3, dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError, match='mask'):
        rp.process(torch.zeros(48, 64, device=dev), mask_out=torch.zeros(48, 60, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match='out_dtype'):
        rp.process(torch.zeros(48, 64, device=dev), out_dtype=torch.float64)
    with pytest.raises(ValueError, match='3 elements'):
        rp.process(torch.zeros(48, 64, device=dev), white_balance=torch.ones(4, device=dev))
    x = torch.zeros(48, 64, device=dev)
    with pytest.raises(RuntimeError, match='overlap'):   # reported by the library: a mask inside the input
        rp.process(x, mask_out=x.view(torch.uint8).view(-1)[:48 * 64].view(48, 64))
    assert tuple(rp.process(x).shape) == (48, 64)
