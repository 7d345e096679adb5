"""GPU: the interior body of the constant-geometry bilateral tile kernel (csrc/tdk_bilateral_tile.h: bilateral_tile_body<..., IN>).

Bilateral.process_lab at the default sigmas runs a kernel that holds two bodies of the same phases and takes the interior one for
every tile whose table records and sample window do not touch the frame's edge.  The interior body differs from the general one in
integer addressing and control flow only, so the two must agree bit for bit: verification_paths(bilateral_general_body=True) runs
the same flavour with the general body alone ('tdk_bilateral(tiles,const,general)' in the library's event timer).  The frames are the
smallest at which the selection can go wrong; pixel tails and unaligned planes take the scalar kernel and never reach the new body."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIGMA_S, SIGMA_R, DETAIL = 2.0, 0.2, 0.4
CONST, GENERAL_BODY, RUNTIME = 'tdk_bilateral(tiles,const)', 'tdk_bilateral(tiles,const,general)', 'tdk_bilateral(tiles)'
FIELDS = ('tiles', 'constant', 'sz', 'rs', 'plane', 'usize', 'lw', 'lh', 'ncx', 'ncy', 'hx', 'hy')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def host(td):
    """(tile width, tile height) of the constant geometry, and interior(w, h) -> (interior columns, interior rows) flags."""
    from torch_darktable._native import lib

    fn = lib.tdk_bilateral_tile_geometry
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    planned, minimal, constant = (ctypes.c_int * len(FIELDS))(), (ctypes.c_int * 6)(), (ctypes.c_int * len(FIELDS))()
    assert fn(4096, 3072, SIGMA_S, SIGMA_R, planned, minimal, constant) == 0
    c = dict(zip(FIELDS, constant))
    tw, th = int((c['ncx'] - 5) * SIGMA_S), int((c['ncy'] - 5) * SIGMA_S)  # the tile slices from tile / sigma_s + 1 cells, + 2 of halo a side
    inner = lib.tdk_bilateral_tile_interior
    inner.restype = ctypes.c_int
    inner.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_ubyte), ctypes.POINTER(ctypes.c_ubyte)]

    def interior(w, h):
        counts, cols, rows = (ctypes.c_int * 5)(), (ctypes.c_ubyte * -(-w // tw))(), (ctypes.c_ubyte * -(-h // th))()
        assert inner(w, h, SIGMA_S, SIGMA_R, counts, cols, rows) == 0 and counts[0] == len(cols) and counts[1] == len(rows)
        return list(cols), list(rows)

    return tw, th, interior


# name: (width, height) in tiles and pixels to add, interior tiles expected
SHAPES = {
    '3x3': (3, 3, 0, 0, 1),
    '3x3+1': (3, 3, 1, 1, 1),     # a fourth tile column and row of one pixel; width % 4 != 0: the scalar kernel
    '3x3-1': (3, 3, -1, -1, 1),   # width % 4 != 0: the scalar kernel
    '3x3+4': (3, 3, 4, 4, 1),
    '3x3-4': (3, 3, -4, -4, 1),
    # one dimension at a time, the width a multiple of 4: the kernel with both bodies, the interior tile next to a last tile row of
    # 1 or 31 pixels, or a last tile column and row of 4 or 60 / 28 pixels
    '3x3_h+1': (3, 3, 0, 1, 1),
    '3x3_h-1': (3, 3, 0, -1, 1),
    '3x3_w+4': (3, 3, 4, 0, 1),
    '3x3_w-4': (3, 3, -4, 0, 1),
    '3x3_h+4': (3, 3, 0, 4, 1),
    '3x3_h-4': (3, 3, 0, -4, 1),
    '4x3_w+8': (3, 3, 8, 0, 2),   # 4 x 3 tiles, the last column 8 pixels wide: the window of the third column ends on the frame's last pixel
    '2x2': (2, 2, 0, 0, 0),       # no interior tile: the general body alone
    '4x1': (4, 1, 0, 0, 0),
}


def planes(w, h, dev, seed, inner_tile, offset=0):
    """fp32 lightness with smooth structure and noise; samples at exactly 0 and 1 and slightly outside (the z clamp) all over,
    and a NaN, an infinity and a huge sample inside `inner_tile` (x0, y0, tw, th) if given; (a, b) chroma.
    offset: the lightness plane is a contiguous view that starts `offset` floats into its buffer (4-byte aligned only)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    lum = 0.5 + 0.5 * np.sin(xx * 0.11) * np.cos(yy * 0.07) + rng.normal(0, 0.05, (h, w)).astype(np.float32)
    lum = np.clip(lum, -0.03, 1.04).astype(np.float32)
    n = 64
    lum[rng.integers(0, h, n), rng.integers(0, w, n)] = rng.choice(np.array([0.0, 1.0, -0.02, 1.03], np.float32), n)
    lum[0, 0], lum[h - 1, w - 1], lum[h // 2, w // 2], lum[h // 2, w // 2 + 1] = 0.0, 1.0, 0.0, 1.0
    if inner_tile:
        x0, y0, tw, th = inner_tile
        lum[y0 + th // 2, x0 + tw // 2], lum[y0 + 1, x0 + 1] = 1.0, 0.0
        lum[y0 + 3, x0 + 5], lum[y0 + th - 2, x0 + tw - 3], lum[y0 + 7, x0 + 9] = np.nan, np.inf, 3.0e38
    ab = rng.uniform(-0.25, 0.25, (h, w, 2)).astype(np.float32)
    buf = torch.empty(h * w + offset, dtype=torch.float32, device=dev)
    view = buf[offset:offset + h * w].view(h, w)
    view.copy_(torch.from_numpy(lum))
    return view, torch.from_numpy(ab).to(dev)


def timed(fn):
    """(result, {timer name: launches}) of one call under the library's event timer."""
    from torch_darktable import _native

    _native.profile_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        names = {k: v[0] for k, v in _native.profile_report().items()}
    finally:
        _native.profile_enable(False)
    return out, names


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


@pytest.mark.parametrize('out_dtype', [torch.float32, torch.float16], ids=['float', 'half'])
@pytest.mark.parametrize('offset', [0, 1], ids=['aligned', 'offset_view'])
@pytest.mark.parametrize('shape', list(SHAPES))
def test_interior_body_equals_general_body_bit_for_bit(td, dev, host, shape, offset, out_dtype):
    from torch_darktable import torch_darktable_extension as ext

    tw, th, interior = host
    nx, ny, dx, dy, want_inner = SHAPES[shape]
    w, h = nx * tw + dx, ny * th + dy
    cols, rows = interior(w, h)
    assert sum(cols) * sum(rows) == want_inner, (w, h, cols, rows)
    inner_tile = (cols.index(1) * tw, rows.index(1) * th, tw, th) if want_inner else None
    lum, ab = planes(w, h, dev, seed=w * 1000 + h, inner_tile=inner_tile, offset=offset)
    vec = w % 4 == 0 and offset == 0
    assert lum.is_contiguous() and (lum.data_ptr() % 16 == 0) == (offset == 0)
    bil = td.Bilateral(dev, (w, h), sigma_s=SIGMA_S, sigma_r=SIGMA_R)
    bil.process_lab(lum, ab, DETAIL, out_dtype=out_dtype)  # builds the workspace and its axis tables
    out, names = timed(lambda: bil.process_lab(lum, ab, DETAIL, out_dtype=out_dtype))
    with ext.verification_paths(bilateral_general_body=True):
        ref, names_g = timed(lambda: bil.process_lab(lum, ab, DETAIL, out_dtype=out_dtype))
    if vec:  # the kernel with both bodies; the switch runs the general body alone
        assert names.get(CONST) == 1 and GENERAL_BODY not in names and RUNTIME not in names, names
        assert names_g.get(GENERAL_BODY) == 1 and CONST not in names_g and RUNTIME not in names_g, names_g
    else:    # pixel tail or unaligned plane: the scalar kernel either way
        assert names.get(RUNTIME) == 1 and CONST not in names and GENERAL_BODY not in names, names
        assert names_g.get(RUNTIME) == 1 and CONST not in names_g and GENERAL_BODY not in names_g, names_g
    assert out.dtype == out_dtype and out.shape == (h, w, 3)
    differ = (bits(out) != bits(ref))
    assert not differ.any(), (int(differ.sum()), differ.nonzero()[:4].tolist())
    with ext.verification_paths(bilateral_runtime_geometry=True):  # and the kernel that reads its geometry from its arguments
        rt = bil.process_lab(lum, ab, DETAIL, out_dtype=out_dtype)
    assert torch.equal(bits(out), bits(rt))
    finite = torch.isfinite(lum)
    assert torch.isfinite(out.float()[finite]).all()
