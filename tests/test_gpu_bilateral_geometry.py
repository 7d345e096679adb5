"""GPU: the constant-geometry flavour of the bilateral tile kernel (csrc/tdk_bilateral_tile.h: GeomConst, bt_fast MODE 3 VEC 4).

Bilateral.process_lab at the default sigmas (2, 0.2) runs a tile kernel compiled for that grid geometry; only integer addressing
and control flow differ from the kernel that reads the geometry from its arguments, so the two must agree bit for bit.  The
library's event timer names the launches: 'tdk_bilateral(tiles,const)' is the constant-geometry kernel, 'tdk_bilateral(tiles)'
the runtime-geometry one.  Any other geometry, pixel tails (width % 4) and unaligned planes run the runtime-geometry kernel."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIGMA_S, SIGMA_R, DETAIL = 2.0, 0.2, 0.4
CONST, RUNTIME = 'tdk_bilateral(tiles,const)', 'tdk_bilateral(tiles)'
TOL = 2e-5  # tests/test_gpu_lab_chain.py: the tile kernel against the general four-kernel Lab path within 2 * TOL

# (width, height): 4 x 4 full tiles (interior and all four edges); partial last tile column and row, W % 4 == 0; one tile;
# 4 tiles per axis whose last one is 4 pixels wide and high
SIZES = [(256, 128), (200, 100), (64, 32), (196, 100)]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


def planes(w, h, dev, seed, offset=0):
    """fp32 lightness over [0, 1] with smooth structure, noise and some samples slightly outside (the z clamp), and (a, b) chroma.
    offset: the lightness plane is a contiguous view that starts `offset` floats into its buffer (4-byte aligned only)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    lum = 0.5 + 0.5 * np.sin(xx * 0.11) * np.cos(yy * 0.07) + rng.normal(0, 0.05, (h, w)).astype(np.float32)
    lum = np.clip(lum, -0.03, 1.04).astype(np.float32)
    lum[rng.integers(0, h, 16), rng.integers(0, w, 16)] = rng.choice(np.array([0.0, 1.0, -0.02, 1.03], np.float32), 16)
    assert lum.min() < 0.0 and lum.max() > 1.0
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


@pytest.mark.parametrize('out_dtype', [torch.float16, torch.float32], ids=['half', 'float'])
@pytest.mark.parametrize('size', SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_constant_geometry_kernel_runs_and_matches_runtime_geometry_bit_for_bit(td, dev, size, out_dtype):
    from torch_darktable import torch_darktable_extension as ext

    w, h = size
    lum, ab = planes(w, h, dev, seed=w * 1000 + h)
    bil = td.Bilateral(dev, (w, h), sigma_s=SIGMA_S, sigma_r=SIGMA_R)
    bil.process_lab(lum, ab, DETAIL, out_dtype=out_dtype)  # builds the workspace and its axis tables
    out, names = timed(lambda: bil.process_lab(lum, ab, DETAIL, out_dtype=out_dtype))
    assert names.get(CONST) == 1 and RUNTIME not in names, names
    with ext.verification_paths(bilateral_runtime_geometry=True):
        ref, names_rt = timed(lambda: bil.process_lab(lum, ab, DETAIL, out_dtype=out_dtype))
    assert names_rt.get(RUNTIME) == 1 and CONST not in names_rt, names_rt
    assert out.dtype == out_dtype and torch.isfinite(out.float()).all()
    assert torch.equal(out, ref), ((out != ref).sum().item(), (out.float() - ref.float()).abs().max().item())
    with ext.verification_paths(bilateral_general=True):  # and both are the filter: the four-kernel path, same parameters
        general = bil.process_lab(lum, ab, DETAIL)
    d = (out.float() - general).abs().max().item()
    assert d <= (2 * TOL if out_dtype == torch.float32 else 2 * TOL + 2.0 ** -12), d  # (binary16 storage of a value in [0, 1]: half a spacing of 2^-11)


FALLBACKS = {
    'sigma_s=3': dict(w=256, h=128, sigma_s=3.0, sigma_r=SIGMA_R),
    'sigma_r=0.1': dict(w=256, h=128, sigma_s=SIGMA_S, sigma_r=0.1),  # sz = 11
    'width 250': dict(w=250, h=128, sigma_s=SIGMA_S, sigma_r=SIGMA_R),  # VEC 1
    'unaligned lum': dict(w=256, h=128, sigma_s=SIGMA_S, sigma_r=SIGMA_R, offset=1),  # VEC 1
}


@pytest.mark.parametrize('case', list(FALLBACKS), ids=lambda c: c.replace(' ', '_'))
def test_other_geometries_run_the_runtime_geometry_kernel(td, dev, case):
    from torch_darktable import torch_darktable_extension as ext

    c = FALLBACKS[case]
    w, h = c['w'], c['h']
    lum, ab = planes(w, h, dev, seed=77, offset=c.get('offset', 0))
    assert lum.is_contiguous() and (lum.data_ptr() % 16 != 0) == bool(c.get('offset', 0))
    bil = td.Bilateral(dev, (w, h), sigma_s=c['sigma_s'], sigma_r=c['sigma_r'])
    bil.process_lab(lum, ab, DETAIL)
    out, names = timed(lambda: bil.process_lab(lum, ab, DETAIL))
    assert names.get(RUNTIME) == 1 and CONST not in names, names
    with ext.verification_paths(bilateral_runtime_geometry=True):
        same, names_rt = timed(lambda: bil.process_lab(lum, ab, DETAIL))
    assert names_rt.get(RUNTIME) == 1 and CONST not in names_rt, names_rt
    assert torch.equal(out, same)
    with ext.verification_paths(bilateral_general=True):
        general = bil.process_lab(lum, ab, DETAIL)
    d = (out - general).abs().max().item()
    assert d <= 2 * TOL, d
