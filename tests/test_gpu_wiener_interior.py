"""GPU: the interior body of the Wiener strip kernel (csrc/tdk_wiener_ystream.h: ystream_body<..., IN>), the idle column stage of a
short last strip, and the launch order.

The strip kernel holds two bodies of its round loop and takes the interior one for every workgroup (strip, segment) none of whose
samples lies outside the frame (the rule: tests/test_wiener_interior.py).  The two differ in integer addressing and control flow
only, so they must agree bit for bit: verification_paths(wiener_general_body=True) runs the kernel with the general body alone
('tdk_wiener(tiles,general)' in the library's event timer).  The default call is also held to the oracle with the bounds of
tests/test_gpu_wiener_geometry.py.

Sizes, from strip_geometry with TR = 8 (what pick_segment_rows gives whenever one round of workgroups suffices): strip gx covers
x in [128 gx - 24, 128 gx + 128), segment gy covers y in [64 gy - 24, 64 gy + 64).
  256 x 128   3 x 3 workgroups, exactly one interior: (1, 1), x in [104, 256), y in [40, 128) -- it ends on the last pixel both ways
  248 x 128   one tile column narrower: strip 1 reaches past the frame (ntx 34: its last tile is absent), no interior workgroup
  256 x 120   one tile row shorter: segment 1 reaches past the frame (reflected rows), no interior workgroup
  384 x 192   4 x 4 workgroups, interior (1, 1), (2, 1), (1, 2), (2, 2): the x seam at 256 and the y seam at 128 lie between interior workgroups
  105 x 81, 113 x 57   (tests/wiener_cases.py) last strip of one / two tiles: three of its four waves have no column stage to run"""

import numpy as np
import pytest
import torch
import wiener_cases as wc
from test_gpu_fallback_paths import oracle_lab
from test_gpu_lab_chain import TOL
from test_gpu_wiener_geometry import F32, gpu, held, npf
from test_wiener_interior import restated

pytestmark = pytest.mark.gpu

TILES, GENERAL = 'tdk_wiener(tiles)', 'tdk_wiener(tiles,general)'
# (W, H): interior workgroups expected
SHAPES = {(256, 128): [(1, 1)], (248, 128): [], (256, 120): [], (384, 192): [(1, 1), (2, 1), (1, 2), (2, 2)], (105, 81): [], (113, 57): []}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a visible MI355X'
    return torch.device('cuda', 0)


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


def both(fn):
    """fn() by default and with the general body forced; asserts the timer names and returns the two results."""
    from torch_darktable import torch_darktable_extension as ext

    out, names = timed(fn)
    with ext.verification_paths(wiener_general_body=True):
        ref, names_g = timed(fn)
    assert names.get(TILES) == 1 and GENERAL not in names, names
    assert names_g.get(GENERAL) == 1 and TILES not in names_g, names_g
    return out, ref


@pytest.mark.parametrize('w,h', list(SHAPES), ids=[f'{w}x{h}' for w, h in SHAPES])
def test_interior_body_equals_general_body_and_the_oracle(td, oracle, dev, scene, w, h):
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert wc.pick_segment_rows(w, h, 1, cus) == 8
    g = wc.strip_geometry(w, h)
    assert [(gx, gy) for gy in range(g.segments) for gx in range(g.strips) if restated(w, h, 8, gx, gy)] == SHAPES[(w, h)]
    if (w, h) in ((105, 81), (113, 57)):
        assert g.strips == 2 and g.last_strip_tiles <= 2   # waves 1 .. 3 of the last strip: both tile pairs beyond ntx
    tag = f'{w}x{h}'
    img = scene(h, w, 300 + w + h)
    one = img[:, :, 1:2].copy()
    ws = td.Wiener(dev, (w, h), overlap_factor=4, tile_size=32)

    x1 = gpu(one, dev)
    assert x1.data_ptr() % 16 == 0
    out, ref = both(lambda: ws.process(x1, 0.05))
    assert torch.equal(out, ref), f'{tag} C=1 f32: {int((out != ref).sum())} values differ between the bodies'
    held(out, oracle.wiener(one, 0.05, 32, 4), F32, f'interior {tag} C=1 f32')

    x16 = gpu(one, dev, torch.float16)
    out, ref = both(lambda: ws.process(x16, 0.05))
    assert out.dtype == torch.float16 and torch.equal(out, ref), f'{tag} C=1 f16'
    held(out, oracle.wiener(npf(x16), 0.05, 32, 4), F32, f'interior {tag} C=1 f16', half=True)

    x = gpu(img, dev)
    lum_ref, ab_ref, _ = oracle_lab(oracle, img)
    (lum, ab), (lum_g, ab_g) = both(lambda: ws.process_log_luminance_lab(x, 0.075))
    assert torch.equal(lum, lum_g) and torch.equal(ab, ab_g), f'{tag} lab'
    held(lum, lum_ref, TOL, f'interior {tag} lab L')
    held(ab, ab_ref, 2 * TOL, f'interior {tag} lab ab')


def test_unaligned_plane_and_interleaved_image_keep_the_general_body(td, oracle, dev, scene):
    """A plane 4 bytes into its buffer (no vector loads) and an interleaved RGB image (C = 3) have no interior workgroup whatever
    their size: the same bits as with the switch, and the oracle's values."""
    w, h = 256, 128
    img = scene(h, w, 17)
    one = img[:, :, 1:2].copy()
    ws = td.Wiener(dev, (w, h), overlap_factor=4, tile_size=32)
    buf = torch.empty(h * w + 1, dtype=torch.float32, device=dev)
    view = buf[1:].view(h, w, 1)
    view.copy_(gpu(one, dev))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    out, ref = both(lambda: ws.process(view, 0.05))
    assert torch.equal(out, ref) and torch.equal(out, ws.process(gpu(one, dev), 0.05))   # ... and the aligned plane's, which takes the interior body
    sig = gpu(np.array([0.05, 0.08, 0.03], np.float32), dev)
    out, ref = both(lambda: ws.process(gpu(img, dev), sig))
    assert torch.equal(out, ref)
    held(out, oracle.wiener(img, np.array([0.05, 0.08, 0.03], np.float32), 32, 4), F32, f'interior {w}x{h} C=3 f32')
