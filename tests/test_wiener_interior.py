"""CPU-only: the interior rule of the Wiener strip kernel (csrc/tdk_wiener_ystream.h: interior_range / is_interior / launch_order,
reached through the host queries of include/tdk_hip_wiener.h) against a restatement from the tile geometry of tests/wiener_cases.py.

A workgroup = (strip gx, segment gy).  Restated from strip_geometry, condition by condition:
  columns: the strip's 152 sample columns start at px0 = 8 (16 gx - 3) and must lie in [0, W);
  tiles:   all 16 tiles of the strip exist, 16 (gx + 1) <= ntx;
  rows:    the segment's NB = min(TR, nty - TR gy) + 3 blocks of 8 rows start at 8 (TR gy - 3) and must lie in [0, H);
  vector:  W % 4 == 0 (the plane is read with 16-byte loads; alignment of the pointer is the caller's).
The first interior strip is strip 1: px0 = 104 and 104 + 152 <= W, W >= 256.  The first interior segment is segment 1: rows
8 TR - 24 .. 16 TR - 1, H >= 16 TR."""

import pytest
import wiener_cases as wc

MI355X_CUS = 256


def restated(W, H, TR, gx, gy):
    g = wc.strip_geometry(W, H, TR)
    if gx >= g.strips or gy >= g.segments:
        return False
    px0 = 8 * (wc.STRIP_TILES * gx - 3)
    columns = px0 >= 0 and px0 + 152 <= W
    tiles = wc.STRIP_TILES * (gx + 1) <= g.ntx
    nb = wc.strip_blocks(W, H, TR)[gy]
    y0 = 8 * (TR * gy - 3)
    rows = y0 >= 0 and y0 + 8 * nb <= H
    return W % 4 == 0 and columns and tiles and rows


@pytest.fixture(scope='module')
def lib(td):
    from torch_darktable._native import lib

    return lib


def grid(lib, W, H, TR):
    g = wc.strip_geometry(W, H, TR)
    return g, [[lib.tdk_wiener_strip_interior(W, H, TR, gx, gy) for gx in range(g.strips)] for gy in range(g.segments)]


def test_first_interior_sizes():
    """The sizes the GPU test is built on, from the restatement alone."""
    assert restated(256, 128, 8, 1, 1) and not restated(255, 128, 8, 1, 1) and not restated(252, 128, 8, 1, 1) and not restated(256, 127, 8, 1, 1)
    assert not restated(248, 128, 8, 1, 1) and not restated(256, 120, 8, 1, 1)   # one tile column narrower, one tile row shorter
    assert sum(restated(256, 128, 8, gx, gy) for gx in range(3) for gy in range(3)) == 1
    assert [(gx, gy) for gy in range(4) for gx in range(4) if restated(384, 192, 8, gx, gy)] == [(1, 1), (2, 1), (1, 2), (2, 2)]


@pytest.mark.parametrize('TR', [8, 9, 13])
def test_rule_equals_the_restatement_around_the_first_interior_sizes(lib, TR):
    """Every W around 256 and 384 (strips 1 and 2 becoming interior) x every H around 16 TR and 24 TR (segments 1 and 2), every
    workgroup of the frame; W % 4 != 0 included (no interior workgroup at all)."""
    seen = 0
    for W in list(range(236, 268)) + list(range(372, 396)) + [512, 520]:
        for H in list(range(16 * TR - 10, 16 * TR + 10)) + list(range(24 * TR - 9, 24 * TR + 9)) + [32 * TR + 3]:
            g, got = grid(lib, W, H, TR)
            want = [[int(restated(W, H, TR, gx, gy)) for gx in range(g.strips)] for gy in range(g.segments)]
            assert got == want, (W, H, TR, got, want)
            seen += sum(map(sum, want))
    assert seen > 0


def test_small_and_odd_frames_have_no_interior_workgroup(lib):
    for W, H in wc.STRIP_SHAPES:
        g, got = grid(lib, W, H, 8)
        assert not any(map(any, got)) or (W >= 256 and H >= 128), (W, H)
        assert got == [[int(restated(W, H, 8, gx, gy)) for gx in range(g.strips)] for gy in range(g.segments)]


def test_query_refuses_what_is_no_plane_of_the_strip_kernel(lib):
    for bad in ((31, 64, 8, 0, 0), (64, 31, 8, 0, 0), (256, 128, 7, 1, 1), (256, 128, 8, -1, 1), (256, 128, 8, 1, -1)):
        assert lib.tdk_wiener_strip_interior(*bad) == -1, bad
    assert lib.tdk_wiener_strip_interior(256, 128, 8, 3, 1) == 0 and lib.tdk_wiener_strip_interior(256, 128, 8, 1, 3) == 0   # beyond the grid
    for bad in ((31, 64, 8, 0), (256, 128, 7, 0), (256, 128, 8, -1), (256, 128, 8, 9)):
        assert lib.tdk_wiener_strip_order(*bad) == -1, bad


def test_count_at_12_megapixels(lib):
    """4096 x 3072 on 256 CUs: TR = 26, 33 strips x 15 segments = 495 workgroups, of which strips 1 .. 31 x segments 1 .. 13 are
    interior."""
    W, H = 4096, 3072
    TR = wc.pick_segment_rows(W, H, 1, MI355X_CUS)
    g, got = grid(lib, W, H, TR)
    assert (TR, g.strips, g.segments) == (26, 33, 15)
    assert sum(map(sum, got)) == 31 * 13 == 403
    assert all(got[gy][gx] == int(1 <= gx <= 31 and 1 <= gy <= 13) for gy in range(15) for gx in range(33))
    assert got == [[int(restated(W, H, TR, gx, gy)) for gx in range(33)] for gy in range(15)]


@pytest.mark.parametrize('W,H,TR', [(4096, 3072, 26), (256, 128, 8), (384, 192, 8), (520, 333, 9), (252, 128, 8), (104, 41, 8), (1537, 809, 9)])
def test_launch_order_is_a_permutation_with_the_edge_workgroups_first(lib, W, H, TR):
    g, inner = grid(lib, W, H, TR)
    n = g.strips * g.segments
    order = [lib.tdk_wiener_strip_order(W, H, TR, b) for b in range(n)]
    assert sorted(order) == list(range(n))
    flags = [inner[k // g.strips][k % g.strips] for k in order]
    edge = n - sum(flags)
    assert flags == [0] * edge + [1] * (n - edge), (W, H, TR, flags)
    assert lib.tdk_wiener_strip_order(W, H, TR, n) == -1
    if not any(flags):
        assert order == list(range(n))   # no interior workgroup: the launch order of before
