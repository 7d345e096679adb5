"""CPU-only: the rule that selects the constant-geometry bilateral tile kernel (csrc/tdk_bilateral_geometry.h), on the host.

The kernel is compiled for one LDS grid geometry, typed into csrc/bilateral.hip (GeomDefault).  launch_tiles runs it only where the
geometry the host planner computes for the image equals that set field by field; this sweeps the planner over image sizes at the
default sigmas (2, 0.2) and checks that the two can never disagree, that the set is what a 12 MP frame plans on its own, and that
other sigmas decline."""

import ctypes

import pytest

FIELDS = ('tiles', 'constant', 'sz', 'rs', 'plane', 'usize', 'lw', 'lh', 'ncx', 'ncy', 'hx', 'hy')
MINIMAL = ('ncx', 'ncy', 'hx', 'hy', 'lw', 'lh')


@pytest.fixture(scope='module')
def geometry(td):
    from torch_darktable._native import lib

    fn = lib.tdk_bilateral_tile_geometry
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                   ctypes.POINTER(ctypes.c_int)]

    def query(w, h, sigma_s=2.0, sigma_r=0.2):
        planned, minimal, constant = (ctypes.c_int * len(FIELDS))(), (ctypes.c_int * 6)(), (ctypes.c_int * len(FIELDS))()
        assert fn(w, h, sigma_s, sigma_r, planned, minimal, constant) == 0
        return dict(zip(FIELDS, planned)), dict(zip(MINIMAL, minimal)), dict(zip(FIELDS, constant))

    return query


def test_constant_set_is_what_a_12mp_frame_plans_on_its_own(geometry):
    planned, minimal, constant = geometry(4096, 3072)
    assert planned == constant and planned['tiles'] == 1 and planned['constant'] == 1
    assert minimal == {k: constant[k] for k in MINIMAL}  # nothing was widened to get there
    # the layout that follows from the window shape (plan_tiles): odd row stride, planes of whole 64-float lines, sample tile | blur temp
    assert constant['rs'] == constant['ncx'] | 1 and constant['plane'] == -(-constant['rs'] * constant['ncy'] // 64) * 64
    lt = constant['lw'] * constant['lh'] + (constant['ncx'] + constant['ncy']) * 9
    assert constant['usize'] == -(-max(lt, constant['sz'] * constant['plane']) // 64) * 64
    assert (constant['sz'], constant['ncx'], constant['ncy']) == (6, 64 // 2 + 5, 32 // 2 + 5)
    # four workgroups per CU: the 160 KiB of LDS hold four of them
    assert 4 * 4 * (constant['sz'] * constant['plane'] + constant['usize'] + constant['lw'] + constant['lh']) <= 160 * 1024


def test_sweep_planner_equals_the_constant_set_or_the_dispatcher_declines(geometry):
    sizes = sorted({64, 65, 68, 96, 100, 127, 128, 132, 136, 192, 196, 200, 250, 256, 320, 1000, 1024, 1920, 2048, 3072, 4096, 6000, 8192})
    heights = sorted({64, 66, 72, 96, 100, 128, 131, 136, 256, 1080, 1536, 3072, 4000, 8192})
    seen = 0
    for w in sizes:
        for h in heights:
            planned, minimal, constant = geometry(w, h)
            if max(w, h) > 6000:  # beyond 3000 cells per axis the grid is coarser than sigma_s and the four-kernel path runs
                assert planned['tiles'] == 0 and planned['constant'] == 0, (w, h, planned)
                continue
            assert planned['tiles'] == 1, (w, h)
            same = all(planned[k] == constant[k] for k in FIELDS[2:])
            assert bool(planned['constant']) == same, (w, h, planned, constant)
            # the planned shape contains what the image's own tiles need
            assert all(minimal[k] <= planned[k] for k in MINIMAL), (w, h, minimal, planned)
            seen += planned['constant']
    # every image of at least one tile that runs the tile kernel at these sigmas has the constant geometry
    assert seen == sum(1 for w in sizes for h in heights if max(w, h) <= 6000)


def test_images_smaller_than_a_tile_and_single_tiles(geometry):
    planned, minimal, constant = geometry(64, 32)
    assert planned['constant'] == 1 and (minimal['lw'], minimal['lh']) == (64, 32)  # the windows end at the image's edge: planned wider
    for w, h in ((16, 8), (4, 4), (40, 500), (500, 12)):
        planned, minimal, constant = geometry(w, h)
        same = all(planned[k] == constant[k] for k in FIELDS[2:])
        assert bool(planned['constant']) == same and all(minimal[k] <= planned[k] for k in MINIMAL), (w, h, planned)


@pytest.mark.parametrize('sigma_s,sigma_r', [(3.0, 0.2), (2.0, 0.1), (1.5, 0.2), (2.5, 0.2), (4.0, 0.2), (2.0, 0.05), (8.0, 0.1)])
def test_other_sigmas_decline(geometry, sigma_s, sigma_r):
    for w, h in ((256, 128), (4096, 3072), (200, 100)):
        planned, minimal, constant = geometry(w, h, sigma_s, sigma_r)
        assert planned['constant'] == 0, (w, h, planned)
        if planned['tiles']:
            assert any(planned[k] != constant[k] for k in FIELDS[2:])
            assert minimal == {k: planned[k] for k in MINIMAL}  # planned exactly as the image needs it
