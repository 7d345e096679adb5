"""GPU: the Wiener denoiser across strip, segment and tile-group geometry (tables and inputs: tests/wiener_cases.py, whose claims
tests/test_wiener_cases.py checks without a GPU).

Every comparison is the whole frame against oracle.wiener on the same float32 values.  Bounds: float32 results within
2e-5 * max(1, max |input|) (test_gpu_parity.py::test_wiener's figure for [0, 1] data, scaled for the log-lightness range); binary16
results that plus half a binary16 ulp of the value (test_gpu_fallback_paths.py::assert_close); the Lab entry point TOL for the
lightness and 2 * TOL for (a, b) (test_gpu_lab_chain.py).  The oracle itself is within 2e-6 of a float64 restatement on these
inputs, relative to the same scale (test_wiener_cases.py).  Measured maxima per test: profiles/r14/wiener_geometry.txt."""

import numpy as np
import pytest
import torch
import wiener_cases as wc
from test_gpu_fallback_paths import f16_ulp, oracle_lab
from test_gpu_lab_chain import TOL

pytestmark = pytest.mark.gpu

F32 = 2e-5
RGB_SIGMAS = np.array([0.05, 0.08, 0.03], np.float32)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a visible MI355X'
    return torch.device('cuda', 0)


def gpu(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t if dtype is None else t.to(dtype)


def npf(t):
    return t.detach().float().cpu().numpy()


def strip_tag(w, h):
    g = wc.strip_geometry(w, h)
    return f'{w}x{h} (ntx {g.ntx}, nty {g.nty}, last strip {g.last_strip_tiles} tiles, last segment {g.last_segment_rows} rows)'


def group_tag(w, h, K, ov):
    g = wc.group_geometry(w, h, K, ov)
    return f'K={K} ov={ov} {w}x{h} (ntx {g.ntx}, nty {g.nty}, last group {g.last_group_tiles} tiles, last band {g.last_group_rows} rows)'


def held(got, ref, tol, what, half=False):
    """|got - ref| <= tol (+ half a binary16 ulp of the value for a binary16 result) everywhere; the message names the worst
    pixel.  Prints the maximum (collected into profiles/r14/wiener_geometry.txt)."""
    g = npf(got)
    assert g.shape == ref.shape, (what, g.shape, ref.shape)
    bound = tol + (0.5 * f16_ulp(np.maximum(np.abs(g), np.abs(ref))) if half else 0.0)
    d = np.abs(g - ref)
    d = np.where(np.isfinite(d), d, np.inf)
    at = np.unravel_index(np.argmax(d - bound), d.shape)
    print(f'MEASURED {what}: max |d| {d.max():.3e}')
    assert (d <= bound).all(), f'{what}: {(d > bound).sum()} values beyond the bound, worst {d[at]:.3e} at (y, x[, c]) = {tuple(int(i) for i in at)}'
    return float(d.max())


# ------------------------------------------------------------------ strip kernel (K = 32, ov = 4)
@pytest.mark.parametrize('w,h', wc.STRIP_SHAPES, ids=[f'{w}x{h}' for w, h in wc.STRIP_SHAPES])
def test_strip_sweep(td, oracle, dev, scene, w, h):
    """wiener_ystream on every STRIP_SHAPES entry (what each reaches: the comments of the table): planar and interleaved float32,
    planar binary16, and the two log-lightness entry points (the planar kernel on the extracted plane + the fused finishes)."""
    tag = strip_tag(w, h)
    img = scene(h, w, 100 + w + h)
    ws = td.Wiener(dev, (w, h), overlap_factor=4, tile_size=32)
    x = gpu(img, dev)
    one = img[:, :, 1:2].copy()
    held(ws.process(gpu(one, dev), 0.05), oracle.wiener(one, 0.05, 32, 4), F32, f'strip {tag} C=1 f32')
    held(ws.process(x, gpu(RGB_SIGMAS, dev)), oracle.wiener(img, RGB_SIGMAS, 32, 4), F32, f'strip {tag} C=3 f32')
    x16 = gpu(one, dev, torch.float16)
    got16 = ws.process(x16, 0.05)
    assert got16.dtype == torch.float16
    held(got16, oracle.wiener(npf(x16), 0.05, 32, 4), F32, f'strip {tag} C=1 f16', half=True)
    lum_ref, ab_ref, den_ref = oracle_lab(oracle, img)
    held(ws.process_log_luminance(x, 0.075), den_ref, F32, f'strip {tag} log-L')
    lum, ab = ws.process_log_luminance_lab(x, 0.075)
    held(lum, lum_ref, TOL, f'strip {tag} lab L')
    held(ab, ab_ref, 2 * TOL, f'strip {tag} lab ab')


def test_strip_longer_segments(td, oracle, dev, scene):
    """pick_segment_rows returns TR = 8 whenever one round of workgroups suffices, so only large frames run another segment
    length: at W = 1537, C = 3, the smallest H <= 1200 for which this device takes TR != 8 with a partial last segment
    (MI355X, 256 CUs: H = 809, TR = 9, last segment 6 rows).  The only test above a megapixel."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    w, pick = 1537, None
    for h in range(32, 1201):
        tr = wc.pick_segment_rows(w, h, 3, cus)
        if tr != 8 and wc.strip_geometry(w, h, tr).nty % tr != 0:
            pick = (h, tr)
            break
    assert pick is not None, f'no H <= 1200 with TR != 8 and a partial last segment on {cus} CUs'
    h, tr = pick
    g = wc.strip_geometry(w, h, tr)
    img = scene(h, w, 77)
    got = td.Wiener(dev, (w, h), overlap_factor=4, tile_size=32).process(gpu(img, dev), gpu(RGB_SIGMAS, dev))
    held(got, oracle.wiener(img, RGB_SIGMAS, 32, 4), F32,
         f'strip {w}x{h} TR={tr} ({cus} CUs; ntx {g.ntx}, nty {g.nty}, last strip {g.last_strip_tiles} tiles, last segment {g.last_segment_rows} rows) C=3 f32')


# ------------------------------------------------------------------ general kernel (the five other (K, ov))
GROUP_CASES = [(K, ov, w, h) for (K, ov) in wc.GROUP_PAIRS for (w, h) in wc.GROUP_SHAPES[(K, ov)]]


@pytest.mark.parametrize('K,ov,w,h', GROUP_CASES, ids=[f'K{K}ov{ov}-{w}x{h}' for K, ov, w, h in GROUP_CASES])
def test_group_sweep(td, oracle, dev, scene, K, ov, w, h):
    """wiener_stream<T, K, OV> on every GROUP_SHAPES entry: planar and interleaved float32; on one shape per (K, ov) also planar
    binary16 and process_log_luminance."""
    tag = group_tag(w, h, K, ov)
    img = scene(h, w, 200 + w + h)
    ws = td.Wiener(dev, (w, h), overlap_factor=ov, tile_size=K)
    x = gpu(img, dev)
    one = img[:, :, 1:2].copy()
    held(ws.process(gpu(one, dev), 0.05), oracle.wiener(one, 0.05, K, ov), F32, f'group {tag} C=1 f32')
    held(ws.process(x, gpu(RGB_SIGMAS, dev)), oracle.wiener(img, RGB_SIGMAS, K, ov), F32, f'group {tag} C=3 f32')
    if (w, h) == wc.GROUP_EXTRA_SHAPE[(K, ov)]:
        x16 = gpu(one, dev, torch.float16)
        held(ws.process(x16, 0.05), oracle.wiener(npf(x16), 0.05, K, ov), F32, f'group {tag} C=1 f16', half=True)
        ll = oracle.compute_luminance(img, True, 1e-4)
        ref = oracle.modify_luminance(img, oracle.wiener(ll[:, :, None], 0.075, K, ov)[:, :, 0], True)
        held(ws.process_log_luminance(x, 0.075), ref, F32, f'group {tag} log-L')


# ------------------------------------------------------------------ spectrum
@pytest.mark.parametrize('h,w', wc.SPECTRUM_SHAPES, ids=[f'{w}x{h}' for h, w in wc.SPECTRUM_SHAPES])
@pytest.mark.parametrize('K,ov', wc.SPECTRUM_PAIRS)
def test_spectrum_patterns(td, oracle, dev, scene, K, ov, h, w):
    """Inputs on which single bins decide the result (the self-conjugate bins 0 and K / 2 of each axis, conjugate pairs at bins
    1, 5, K / 2 - 1, partially attenuated at sigma = 0.1: test_wiener_cases.py), single samples, white noise and the
    log-lightness range, for every sigma from 'nothing removed' to 'everything removed'."""
    ws = td.Wiener(dev, (w, h), overlap_factor=ov, tile_size=K)
    for name, p in {**wc.patterns(h, w, K, scene, oracle), **wc.extra_patterns(h, w, scene, oracle)}.items():
        scale = wc.scale_of(p)
        x = gpu(p[:, :, None], dev)
        worst = 0.0
        for sigma in wc.SIGMAS:
            got = ws.process(x, sigma)
            what = f'spectrum K={K} ov={ov} {w}x{h} {name} sigma={sigma}'
            d = np.abs(npf(got) - oracle.wiener(p[:, :, None], sigma, K, ov))
            at = np.unravel_index(np.argmax(d), d.shape)
            assert d.max() <= F32 * scale, f'{what}: {d.max():.3e} at (y, x) = {tuple(int(i) for i in at[:2])}'
            worst = max(worst, float(d.max()))
            if sigma == 0.0:
                assert np.abs(npf(got)[:, :, 0] - p).max() <= 2e-6 * scale, what
            if name == 'const':
                assert np.abs(npf(got) - 0.3).max() <= 2e-6, what
        print(f'MEASURED spectrum K={K} ov={ov} {w}x{h} {name}: max |d| over sigmas {worst:.3e} (scale {scale:.2f})')


# ------------------------------------------------------------------ sigma forms
@pytest.mark.parametrize('K,ov', [(32, 4), (16, 4)])
def test_sigma_forms(td, oracle, dev, scene, K, ov):
    """A float and a tensor of the same value(s) give identical bits (C = 1: one element; C = 3: three equal elements); sigmas
    that differ per channel from 'identity' to 'everything removed' are held to the oracle."""
    h, w = 57, 113
    img = scene(h, w, 31)
    ws = td.Wiener(dev, (w, h), overlap_factor=ov, tile_size=K)
    x, x1 = gpu(img, dev), gpu(img[:, :, :1].copy(), dev)
    assert torch.equal(ws.process(x1, 0.1), ws.process(x1, torch.tensor([0.1], device=dev)))
    assert torch.equal(ws.process(x, 0.1), ws.process(x, torch.tensor([0.1, 0.1, 0.1])))
    with pytest.raises(ValueError):
        ws.process(x, torch.tensor([0.1], device=dev))
    sig = np.array([0.0, 0.1, 5.0], np.float32)
    held(ws.process(x, gpu(sig, dev)), oracle.wiener(img, sig, K, ov), F32, f'sigma forms K={K} ov={ov} {w}x{h} per-channel (0, 0.1, 5)')


# ------------------------------------------------------------------ state
@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('K,ov', [(32, 4), (16, 4)])
def test_result_is_independent_of_the_workspace_contents(td, dev, scene, K, ov, C):
    """The slabs live in a workspace that calls reuse: a call's result must not depend on what the previous call left there
    (slab regions of absent tiles, carried seam rows), nor on the run (no atomics): bit-identical after an intervening
    sigma = 5 call on another image, on a fresh object, and repeated."""
    w, h = (233, 89) if K == 32 else (53, 53)  # last strip / group of one tile, a partial last segment / band
    a = gpu(scene(h, w, 41)[:, :, :C].copy(), dev)
    other = gpu(1.0 - scene(h, w, 42)[:, :, :C], dev)
    sig = gpu(RGB_SIGMAS[:C], dev)
    ws = td.Wiener(dev, (w, h), overlap_factor=ov, tile_size=K)
    first = ws.process(a, sig).clone()
    assert torch.equal(ws.process(a, sig), first), 'repeated call differs'
    ws.process(other, 5.0)
    assert torch.equal(ws.process(a, sig), first), 'differs after an intervening call on the same workspace'
    assert torch.equal(td.Wiener(dev, (w, h), overlap_factor=ov, tile_size=K).process(a, sig), first), 'a fresh object differs'
    assert not torch.equal(first, a)
