"""CPU-only: which tiles the constant-geometry bilateral tile kernel runs its interior body on (csrc/tdk_bilateral_tile.h:
tile_is_interior), and the kernel's resource contract with both bodies in it.

The interior body is the general body with every guard against the frame's edge made a compile-time constant, so it may only run
on a tile whose two axis records and sample window are the constant ones.  tdk_bilateral_tile_interior restates the kernel's test on
the host, per tile column and per tile row; this compares it with a plain Python restatement of the same conditions over a sweep
of frame sizes, and reads the gfx950 metadata of the kernel that holds both bodies: 8 waves per SIMD, no spill, no scratch."""
import ctypes
import math
import re

import numpy as np
import pytest

from kernel_isa import device_asm, metadata

FIELDS = ('tiles', 'constant', 'sz', 'rs', 'plane', 'usize', 'lw', 'lh', 'ncx', 'ncy', 'hx', 'hy')
SIGMA_S, SIGMA_R = 2.0, 0.2
f32 = np.float32


@pytest.fixture(scope='module')
def lib(td):
    from torch_darktable._native import lib

    lib.tdk_bilateral_tile_geometry.restype = ctypes.c_int
    lib.tdk_bilateral_tile_geometry.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.POINTER(ctypes.c_int),
                                                ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    lib.tdk_bilateral_tile_interior.restype = ctypes.c_int
    lib.tdk_bilateral_tile_interior.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.POINTER(ctypes.c_int),
                                                ctypes.POINTER(ctypes.c_ubyte), ctypes.POINTER(ctypes.c_ubyte)]
    lib.tdk_bilateral_grid_size.restype = ctypes.c_int
    lib.tdk_bilateral_grid_size.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.POINTER(ctypes.c_int)]
    return lib


def geometry(lib, w, h, sigma_s=SIGMA_S, sigma_r=SIGMA_R):
    planned, minimal, constant = (ctypes.c_int * len(FIELDS))(), (ctypes.c_int * 6)(), (ctypes.c_int * len(FIELDS))()
    assert lib.tdk_bilateral_tile_geometry(w, h, sigma_s, sigma_r, planned, minimal, constant) == 0
    return dict(zip(FIELDS, planned)), dict(zip(FIELDS, constant))


def interior(lib, w, h, sigma_s=SIGMA_S, sigma_r=SIGMA_R, tiles=(64, 32)):
    counts = (ctypes.c_int * 5)()
    cols, rows = (ctypes.c_ubyte * -(-w // tiles[0]))(), (ctypes.c_ubyte * -(-h // tiles[1]))()
    assert lib.tdk_bilateral_tile_interior(w, h, sigma_s, sigma_r, counts, cols, rows) == 0
    return list(counts), list(cols), list(rows)


def tile_size(constant, sigma_s=SIGMA_S):
    """The pixel tile the constant geometry was made for: it slices from tile / sigma_s + 1 cells, kept with 2 cells of halo a side."""
    return int((constant['ncx'] - 5) * sigma_s), int((constant['ncy'] - 5) * sigma_s)


def axis_interior(ti, tile, size_px, size_cells, sigma_s, nc, halo, lp, nm):
    """One axis of tile_is_interior, from the definitions: the cells the tile's pixels slice from with 2 cells of halo are nc cells,
    all inside the grid; the longest run of pixels with a positive weight on one of them is nm pixels; the sample window
    [p0 - halo, p0 - halo + lp) lies inside the frame.  float32 arithmetic as the library's."""
    s, top = f32(sigma_s), f32(size_cells - 1)
    g = lambda p: min(max(f32(p) / s, f32(0)), top)
    base = lambda p: min(int(g(p)), size_cells - 2)
    p0, p1 = ti * tile, min(ti * tile + tile, size_px) - 1
    c_lo, c_hi = base(p0) - 2, base(p1) + 1 + 2  # first and last cell kept
    if c_lo < 0 or c_hi >= size_cells or c_hi - c_lo + 1 != nc:
        return False
    lo = p0 - halo
    if lo < 0 or lo + lp > size_px:
        return False
    px = [(p, base(p), g(p) - f32(base(p))) for p in range(lo, lo + lp)]
    longest = 0
    for cell in range(c_lo, c_hi + 1):
        run = [p for p, b, f in px if (b == cell and f32(1) - f > 0) or (b == cell - 1 and f > 0)]
        if run:
            assert run == list(range(run[0], run[-1] + 1))  # the pixels with a positive weight on a cell are consecutive
            longest = max(longest, len(run))
    return longest == nm


WIDTHS = [64, 128, 136, 137, 191, 192, 193, 196, 200, 208, 250, 256, 257, 264, 320, 1000, 1024, 4096]
HEIGHTS = [32, 64, 71, 72, 95, 96, 97, 100, 104, 128, 131, 136, 1080, 3072]


def test_classification_equals_its_restatement_over_a_sweep(lib):
    _, constant = geometry(lib, 4096, 3072)
    tw, th = tile_size(constant)
    seen = set()
    size = (ctypes.c_int * 3)()
    restated = {}  # one axis depends on (pixels, cells, axis) only; the cells of one axis depend a little on the other axis' pixels

    def want(axis, px, cells):
        if (axis, px, cells) not in restated:
            t, nc, halo, lp = (tw, constant['ncx'], constant['hx'], constant['lw']) if axis == 'x' else (th, constant['ncy'], constant['hy'], constant['lh'])
            restated[axis, px, cells] = [int(axis_interior(i, t, px, cells, SIGMA_S, nc, halo, lp, 3)) for i in range(-(-px // t))]
        return restated[axis, px, cells]

    for w in WIDTHS:
        for h in HEIGHTS:
            planned, _ = geometry(lib, w, h)
            assert planned['constant'] == 1, (w, h)
            assert lib.tdk_bilateral_grid_size(w, h, SIGMA_S, SIGMA_R, size) == 0
            counts, cols, rows = interior(lib, w, h, tiles=(tw, th))
            assert counts[:2] == [-(-w // tw), -(-h // th)], (w, h, counts)
            want_c, want_r = want('x', w, size[0]), want('y', h, size[1])
            assert cols == want_c and rows == want_r, (w, h, cols, want_c, rows, want_r)
            assert counts[2:] == [sum(cols), sum(rows), sum(cols) * sum(rows)], (w, h, counts)
            # an interior tile is never on the outer ring, and its window ends inside the frame
            assert not cols[0] and not cols[-1] and not rows[0] and not rows[-1], (w, h, cols, rows)
            seen.add((sum(cols) > 0, sum(rows) > 0))
    assert seen == {(False, False), (False, True), (True, False), (True, True)}


def test_12mp_interior_tiles_are_the_tiles_off_the_outer_ring(lib):
    _, constant = geometry(lib, 4096, 3072)
    tw, th = tile_size(constant)
    counts, cols, rows = interior(lib, 4096, 3072, tiles=(tw, th))
    tx, ty = 4096 // tw, 3072 // th
    assert counts == [tx, ty, tx - 2, ty - 2, (tx - 2) * (ty - 2)], counts
    assert cols == [0] + [1] * (tx - 2) + [0] and rows == [0] + [1] * (ty - 2) + [0]


@pytest.mark.parametrize('w,h,want', [(192, 96, 1), (191, 95, 1), (193, 97, 1), (188, 92, 1), (196, 100, 1), (200, 96, 2), (250, 104, 4), (136, 72, 1), (135, 72, 0),
                                      (136, 71, 0), (128, 64, 0), (256, 32, 0)], ids=lambda v: str(v))
def test_small_frames(lib, w, h, want):
    """A tile column is interior when its sample window, which ends 8 pixels beyond the tile, still ends inside the frame (and it
    is not the first): 3 x 3 tiles, a few pixels more or fewer, have one interior tile; the second column of 200 pixels ends its
    window on the frame's last pixel; 136 x 72 is the smallest frame with an interior tile; 2 x 2 tiles and a single row have none."""
    _, constant = geometry(lib, 4096, 3072)
    counts, _, _ = interior(lib, w, h, tiles=tile_size(constant))
    assert counts[4] == want, counts


def test_other_sigmas_have_no_interior_tiles(lib):
    for ss, sr in ((3.0, 0.2), (2.0, 0.1), (8.0, 0.1)):
        counts = (ctypes.c_int * 5)()
        assert lib.tdk_bilateral_tile_interior(4096, 3072, ss, sr, counts, None, None) == 0
        assert list(counts)[2:] == [0, 0, 0], (ss, sr, list(counts))


@pytest.fixture(scope='module')
def asm():
    return device_asm('bilateral')


def test_kernel_with_both_bodies_keeps_eight_waves_and_spills_nothing(asm):
    """Code-object metadata of bt_fast MODE 3 VEC 4 GeomConst with the interior body (last template argument true), both output
    types: 64 VGPRs at most and no AGPRs is 8 waves per SIMD of the 512-entry file; no spill, no private segment."""
    meta = metadata(asm)
    both = {n: m for n, m in meta.items() if re.search(r'bt_fast21bilateral_tile_kernelIf(f|6__half)Li3ELi4ENS_9GeomConst\w+?EELb1EEE', n)}
    assert len(both) == 2, sorted(meta)
    general = {n: m for n, m in meta.items() if re.search(r'bt_fast21bilateral_tile_kernelIf(f|6__half)Li3ELi4ENS_9GeomConst\w+?EELb0EEE', n)}
    assert len(general) == 2, sorted(meta)
    for name, m in {**both, **general}.items():
        print(name, {k: m[k] for k in ('vgpr_count', 'sgpr_count', 'agpr_count', 'private_segment_fixed_size')})
        assert m['vgpr_count'] <= 64 and m.get('agpr_count', 0) == 0, (name, m)
        assert m['sgpr_spill_count'] == 0 and m['vgpr_spill_count'] == 0, (name, m)
        assert m['private_segment_fixed_size'] == 0, (name, m)
        assert m['max_flat_workgroup_size'] == 512, (name, m)
        # the compiler's own statement of the occupancy it reached, in the kernel's trailer
        trailer = asm[re.search(r'\.size\s+' + re.escape(name), asm).end():]
        occ = re.search(r'; Occupancy: (\d+)', trailer)
        assert occ and int(occ.group(1)) == 8, (name, occ and occ.group(0))
        assert re.search(r'; ScratchSize: (\d+)', trailer).group(1) == '0', name
