"""GPU: the local Laplacian (csrc/laplacian.hip) over its whole input and parameter domain.

The other Laplacian tests all run the Lab lightness of the synthetic scene -- values in [0, 1], sigma 0.2 to 0.35.  Here the kernel
runs the classes of tests/laplacian_cases.py (values far outside [0, 1], the binary16 neighbours of every gamma centre, samples
exactly on the curve's |c| == 2 sigma select, flat frames, frames built around the curve's wave-uniform shortcut, the binary16
subnormal range and values near its top, single NaN / +-inf / overflowing samples, sigma from 2^-21 to 2^21, slopes from -0.5 to 2.5,
clarity from -1 to 5) on the smallest frames that take each branch of the launch schedule, in both storage types, and is held to
the C oracle on the same float32 input -- the oracle evaluates in the kernel's operation order, and tests/test_laplacian_spec.py
holds the oracle to the float64 specification on the same classes:

  clarity == 0   the oracle's values, every pixel;
  clarity != 0   at most one binary16 ulp of max(|result|, s) on at most 1e-4 of the pixels (hardware exp2 against libm's expf; s is
                 the scale of the level-0 sum, tests/laplacian_spec.py);
  masks          NaN, +inf and -inf positions are the oracle's, exactly.

The workspace tests poison what the kernel leaves unwritten: the assemble side writes only the rectangles the finer level reads, into
a cached buffer that is reused from call to call."""

import numpy as np
import pytest
import torch

import laplacian_cases as C
from laplacian_spec import half_ulp_of, laplacian_spec

pytestmark = pytest.mark.gpu

CLASS_FRAMES = [(33, 70), (301, 515)]
PARAMETER_FRAME = (120, 161)
DTYPES = {'f32': torch.float32, 'f16': torch.float16}
MAKERS = {name: make for name, make, _ in C.CLASSES}
FLIP_SHARE = 1e-4   # the project's figure for hardware exp2 against libm (test_gpu_parity.py::test_laplacian)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a visible MI355X'
    return torch.device('cuda', 0)


def gpu(a, dev, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dtype)


def npf(t):
    return t.detach().float().cpu().numpy()


def laplacian(td, dev, shape, prm):
    return td.Laplacian(dev, (shape[1], shape[0]), td.LaplacianParams(6, *prm))


_references = {}


def reference(oracle, name, shape, prm, dtype='f32'):
    """(frame as the kernel sees it, the oracle's result) of a value class -- computed once, shared by the tests, never modified."""
    key = (name, shape, prm, dtype)
    if key not in _references:
        frame = MAKERS[name](*shape)
        if dtype == 'f16':
            frame = frame.astype(np.float16).astype(np.float32)
        ref = oracle.laplacian(frame, *prm)
        frame.setflags(write=False)
        ref.setflags(write=False)
        _references[key] = (frame, ref)
    return _references[key]


def same_masks(got, ref, what):
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f'{what}: NaN positions differ on {(np.isnan(got) != np.isnan(ref)).mean():.3f} of the pixels'
    assert np.array_equal(np.isposinf(got), np.isposinf(ref)) and np.array_equal(np.isneginf(got), np.isneginf(ref)), f'{what}: inf positions differ'


def hold(got, ref, frame, prm, what):
    """The bound of the module docstring for one result."""
    same_masks(got, ref, what)
    fin = np.isfinite(ref)
    d = np.abs(got[fin].astype(np.float64) - ref[fin])
    share = float((d > 0).sum() / ref.size)
    print(f'{what}: largest |d| {d.max() if d.size else 0.0:.3e}, differing share {share:.2e}, finite share {fin.mean():.2f}')
    if prm[3] == 0.0 or not d.any():
        assert not d.any(), f'{what}: {share:.2e} of the pixels differ, largest {d.max():.3e}'
        return
    s = laplacian_spec(frame, *prm)[1]
    ulps = d / half_ulp_of(np.maximum(np.maximum(np.abs(got[fin]), np.abs(ref[fin])), s[fin]))
    print(f'{what}: {ulps.max():.2f} binary16 ulps of max(|result|, s)')
    assert ulps.max() <= 1.0 and share <= FLIP_SHARE, f'{what}: {ulps.max():.2f} ulps, share {share:.2e}'


# ------------------------------------------------------------------ the value classes
@pytest.mark.parametrize('shape', CLASS_FRAMES, ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('name,prm', [(n, p) for n, _, p in C.VALUE_CASES], ids=[C.case_id(n, p) for n, _, p in C.VALUE_CASES])
def test_value_classes(td, oracle, dev, name, prm, shape):
    frame, ref = reference(oracle, name, shape, prm)
    if name == 'huge':
        assert np.isfinite(ref).all()   # every curve stays below 65504: the class is about magnitude, not overflow
    got = npf(laplacian(td, dev, shape, prm).process(gpu(frame, dev)))
    hold(got, ref, frame, prm, f'{C.case_id(name, prm)} {shape}')


@pytest.mark.parametrize('shape', C.FRAMES, ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('value', [0.0, 1.0, 0.37, -3.0, 1000.0])
def test_flat_frame_closed_form(td, dev, value, shape):
    """shadows = highlights = 1, clarity = 0: the curve is the identity, every Laplacian of a flat frame is 0 and every level of the
    output pyramid is the constant -- the result is the binary16-rounded constant.  No oracle needed."""
    got = npf(laplacian(td, dev, shape, C.IDENTITY).process(gpu(np.full(shape, value, np.float32), dev)))
    assert np.array_equal(got, np.full(shape, np.float32(np.float16(value))))


# ------------------------------------------------------------------ the parameter domain
@pytest.mark.parametrize('prm', C.PARAMETER_CASES, ids=[C.case_id('p', p) for p in C.PARAMETER_CASES])
def test_parameter_domain(td, oracle, dev, prm):
    frame, ref = reference(oracle, 'uniform_mid', PARAMETER_FRAME, prm)
    got = npf(laplacian(td, dev, PARAMETER_FRAME, prm).process(gpu(frame, dev)))
    hold(got, ref, frame, prm, f'{C.case_id("uniform_mid", prm)} {PARAMETER_FRAME}')


# ------------------------------------------------------------------ one non-finite sample
@pytest.mark.parametrize('shape', C.NONFINITE_FRAMES, ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('where', ['corner00', 'top_mid', 'corner11', 'interior'])
@pytest.mark.parametrize('special', list(C.SPECIALS))
def test_one_non_finite_sample(td, oracle, dev, special, where, shape):
    """The sample is data, not an address: every index in the kernel comes from pixel coordinates and clamps.  What the test holds is
    the footprint -- the reference's expand never reads the cells an odd coordinate skips, so a corner sample leaves a quarter to
    a half of the frame finite, and the kernel must leave exactly the same part finite, with the oracle's values in it."""
    frame = C.nonfinite_frame(*shape, special, where)
    for prm in (C.PLAIN, C.CLARITY):
        ref = oracle.laplacian(frame, *prm)
        finite = np.isfinite(ref).mean()
        if where == 'interior':
            assert np.isnan(ref).all()     # one interior sample wipes the frame, in the reference too
        elif where.startswith('corner'):
            assert finite >= 0.2, finite   # what makes the mask comparison discriminating (measured: 0.26 to 0.60)
        lap = laplacian(td, dev, shape, prm)
        got = npf(lap.process(gpu(frame, dev)))
        hold(got, ref, frame, prm, f'{special} at {where} {shape} clarity {prm[3]}')
        if shape == (33, 70):   # both storage types; 7e4 is an infinity in binary16 already
            x16 = gpu(frame, dev, torch.float16)
            got16 = lap.process(x16)
            assert got16.dtype == torch.float16
            same_masks(npf(got16), oracle.laplacian(npf(x16), *prm), f'{special} at {where} float16')
            assert np.array_equal(npf(got16), npf(lap.process(x16.float())), equal_nan=True)


@pytest.mark.parametrize('shape', C.NONFINITE_SLOPE_FRAMES, ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('prm', C.NONFINITE_SLOPES, ids=[C.case_id('slopes', p) for p in C.NONFINITE_SLOPES])
def test_one_non_finite_sample_with_negative_and_zero_slopes(td, oracle, dev, prm, shape):
    """Clarity 0 with a negative or zero slope: the curve's linear branch sends an infinite sample to an infinity of the other sign than
    the input pyramid's, and the assemble would return +-inf -- on a third to a half of the frame -- where the reference returns NaN.
    The reference adds clarity * c * exp(..) for every clarity, 0 * inf = NaN at clarity 0; the clarity-free instantiation must too."""
    lap = laplacian(td, dev, shape, prm)
    for special in C.SPECIALS:
        for where in C.positions(*shape):
            frame = C.nonfinite_frame(*shape, special, where)
            ref = oracle.laplacian(frame, *prm)
            assert not np.isinf(ref).any()
            hold(npf(lap.process(gpu(frame, dev))), ref, frame, prm, f'{special} at {where} {shape} slopes {prm[1]} {prm[2]}')
            if shape == (33, 70):
                x16 = gpu(frame, dev, torch.float16)
                same_masks(npf(lap.process(x16)), oracle.laplacian(npf(x16), *prm), f'{special} at {where} float16')


# ------------------------------------------------------------------ float16 storage, an offset view
CASES_F16 = [(n, p, CLASS_FRAMES[0]) for n, _, p in C.VALUE_CASES] + [('uniform_mid', p, PARAMETER_FRAME) for p in C.PARAMETER_CASES]


@pytest.mark.parametrize('name,prm,shape', CASES_F16, ids=[C.case_id(n, p) + f'-{s[0]}x{s[1]}' for n, p, s in CASES_F16])
def test_float16_storage_same_values(td, oracle, dev, name, prm, shape):
    """binary16 in and out carries the same values as the float32 call on the same (binary16-valued) input
    (test_gpu_fp16_storage.py::test_laplacian_fp16_storage_same_values), and those are the oracle's."""
    frame, ref = reference(oracle, name, shape, prm, 'f16')
    lap = laplacian(td, dev, shape, prm)
    x16 = gpu(frame, dev, torch.float16)
    got16, got32 = lap.process(x16), lap.process(x16.float())
    assert got16.dtype == torch.float16 and torch.equal(got16.float(), got32)
    hold(npf(got16), ref, frame, prm, f'{C.case_id(name, prm)} {shape} float16')


def test_offset_view(td, oracle, dev):
    """The gamma-centre class on a plane that starts 4 bytes into its allocation: the scalar fallback of the level-1 loads."""
    shape = CLASS_FRAMES[0]
    for prm in (C.PLAIN, (0.1, 0.5, 1.5, 0.3)):
        frame, ref = reference(oracle, 'gamma_centres', shape, prm)
        t = gpu(frame, dev)
        pool = torch.zeros(t.numel() + 4, dtype=torch.float32, device=dev)
        view = pool[1:1 + t.numel()].view(t.shape)
        view.copy_(t)
        assert view.is_contiguous() and pool.data_ptr() % 256 == 0 and view.data_ptr() % 16 == 4
        lap = laplacian(td, dev, shape, prm)
        got = lap.process(view)
        hold(npf(got), ref, frame, prm, f'gamma_centres +4 B clarity {prm[3]}')
        assert torch.equal(got, lap.process(t))


# ------------------------------------------------------------------ the workspace the kernel leaves partly unwritten
@pytest.mark.parametrize('dtype', list(DTYPES))
@pytest.mark.parametrize('shape', C.FRAMES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_poisoned_workspace(td, dev, shape, dtype):
    """The assemble side writes only the rectangles the finer level reads, into a cached torch.empty buffer.  Fill that buffer with
    NaNs between two calls: a tap that reads a cell this call did not write shows as a NaN or as a changed value."""
    from torch_darktable.torch_darktable_extension import lib

    h, w = shape
    x = gpu(MAKERS['uniform_mid'](h, w), dev, DTYPES[dtype])
    lap = laplacian(td, dev, shape, C.CLARITY)
    first = lap.process(x)
    nbytes = max(int(lib.tdk_laplacian_workspace_bytes(w, h, 6)), 256)
    ws = lap._laplacian._scratch.get(nbytes, dev)   # the buffer the next call on this stream gets
    assert ws.numel() >= nbytes and lap._laplacian._scratch.get(nbytes, dev) is ws and len(lap._laplacian._scratch) == 1
    ws.fill_(0xFF)   # every half a NaN
    second = lap.process(x)
    assert lap._laplacian._scratch.get(nbytes, dev) is ws
    assert torch.isfinite(first).all() and torch.equal(first, second), f'{(first != second).float().mean().item():.3f} of the pixels changed'


@pytest.mark.parametrize('shape', [(33, 70), (301, 515)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_stale_frame(td, dev, shape):
    """A frame full of +-inf, NaN and 6e4 samples, then an ordinary one on the same object: nothing of the first survives."""
    h, w = shape
    rng = np.random.default_rng(5)
    bad = MAKERS['uniform_mid'](h, w).copy()
    bad.flat[rng.choice(bad.size, bad.size // 7, replace=False)] = rng.choice(np.array([np.inf, -np.inf, np.nan, 6e4], np.float32), bad.size // 7)
    x = gpu(MAKERS['uniform_wide'](h, w), dev)
    lap = laplacian(td, dev, shape, C.CLARITY)
    assert not torch.isfinite(lap.process(gpu(bad, dev))).all()
    got = lap.process(x)
    assert torch.isfinite(got).all() and torch.equal(got, laplacian(td, dev, shape, C.CLARITY).process(x))


# ------------------------------------------------------------------ Laplacian.process_rgb
@pytest.mark.parametrize('dtype', list(DTYPES))
def test_process_rgb(td, oracle, dev, scene, dtype):
    """compute_luminance -> process -> modify_luminance on a frame with a patch above 1 and a negative patch, against the oracle's chain
    step by step (compute_luminance clips the pixel into [0, 1] before the Lab conversion, color_conversions.cu:168-172, so the filter
    sees L in [0, 1] with both patches on the clip -- values beyond that reach Laplacian.process only directly): the luminance and the replacement within the tolerances of test_gpu_parity.py::test_luminance_extract_replace (2e-5,
    5e-5), the filter -- without the clarity term -- exact on the luminance the device produced.  float16 storage sees the rounded
    frame and rounds each result once more: half a binary16 ulp on top."""
    h, w = 72, 100
    img = scene(h, w, 21).copy()
    img[10:30, 20:50] *= 2.5
    img[40:60, 60:90] = -0.25 * img[40:60, 60:90] - 0.05
    x = gpu(img, dev, DTYPES[dtype])
    img = npf(x)
    assert img.max() > 1.5 and img.min() < -0.05
    half = (lambda v: 0.5 * half_ulp_of(v)) if dtype == 'f16' else (lambda v: 0.0)
    lum = td.compute_luminance(x)
    ref_lum = oracle.compute_luminance(img)
    assert np.isfinite(ref_lum).all() and ref_lum.min() == 0.0 and ref_lum.max() == 1.0   # both patches reach the clip
    assert (np.abs(npf(lum) - ref_lum) <= 2e-5 + half(ref_lum)).all()
    ref_lap = oracle.laplacian(npf(lum), *C.PLAIN)
    ref = oracle.modify_luminance(img, ref_lap)
    assert np.isfinite(ref).all()
    got = laplacian(td, dev, (h, w), C.PLAIN).process_rgb(x)
    assert got.dtype == DTYPES[dtype] and got.shape == x.shape
    assert (np.abs(npf(got) - ref) <= 5e-5 + half(ref)).all(), np.abs(npf(got) - ref).max()
