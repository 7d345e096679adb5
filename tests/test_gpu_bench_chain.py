"""GPU: the chain bench.py times, at full size, against the strict-fp32 oracle chain.

bench.build_pipeline's Lab hand-over (RCD -> Wiener.process_log_luminance_lab -> Bilateral.process_lab(out_dtype, metrics) ->
reinhard_tonemap(acc.finish())) is imported, not restated, so this test follows whatever the bench measures.  Three frames run
on three streams through sharding.FrameStreams inside concurrent_frames(), as the timed region issues them (RCD takes the
register-blocked strips).  Each frame is checked on windows -- interior ones, one on each edge of the frame, the four corners --
by crop consistency (tests/test_gpu_fullsize.py): Wiener (tile grid period 8, 32-px tiles) and the bilateral grid (cells of
exactly 2 px) have bounded footprints, so the oracle's Wiener -> bilateral on a crop with a 64-px margin on its inner sides
(none on the sides that are the frame's own edges; origins on multiples of 8, even widths) reproduces the window.
RCD is the exception: the reference's shared p/q scratch slots make its last computed row and columns at the bottom / right
edges depend on samples far away (oracle/src/rcd.c), so the oracle's RCD runs on the whole frame (a fraction of a second)."""

import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 2e-5   # the colour operators' tolerance (tests/test_gpu_lab_chain.py)
N, M = 192, 64  # window size; crop margin on the inner sides


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


def npy(t):
    return t.detach().float().cpu().numpy() if t.dtype == torch.float16 else t.detach().cpu().numpy()


class _Tapped:
    """torch_darktable as build_pipeline sees it, except that what each RCD.process and Bilateral.process_lab return and the
    metrics handed to reinhard_tonemap are recorded (in issue order: one of each per frame)."""

    def __init__(self, td):
        self._td, self.demosaiced, self.rgb, self.metrics = td, [], [], []

    def __getattr__(self, name):
        return getattr(self._td, name)

    def RCD(self, *args, **kwargs):
        rcd = self._td.RCD(*args, **kwargs)
        process = rcd.process

        def tapped(*a, **k):
            out = process(*a, **k)
            self.demosaiced.append(out)
            return out

        rcd.process = tapped
        return rcd

    def Bilateral(self, *args, **kwargs):
        bil = self._td.Bilateral(*args, **kwargs)
        process_lab = bil.process_lab

        def tapped(*a, **k):
            out = process_lab(*a, **k)
            self.rgb.append(out)
            return out

        bil.process_lab = tapped
        return bil

    def reinhard_tonemap(self, image, metrics, params):
        self.metrics.append(metrics)
        return self._td.reinhard_tonemap(image, metrics, params)


def windows(w, h):
    """(y0, y1, x0, x1) output windows: 3 interior, one on each edge, the 4 corners.  Windows on the right / bottom edge start on
    the last multiple of 8 that leaves at least N pixels and run to the edge."""
    yb, xr = 8 * ((h - N) // 8), 8 * ((w - N) // 8)
    interior = [(1024, 2048), (2000, 304), (1504, 3304)]
    edges = [(0, 1600), (yb, 2400), (1400, 0), (800, xr)]
    corners = [(0, 0), (0, xr), (yb, 0), (yb, xr)]
    return [(y0, h if y0 == yb else y0 + N, x0, w if x0 == xr else x0 + N) for y0, x0 in interior + edges + corners]


def oracle_lab_chain(oracle, rgb):
    """cpu_baseline.run's isp sequence (bench.py) after the demosaic, on one crop."""
    ll = oracle.compute_luminance(rgb, True, 1e-4)
    den = oracle.modify_luminance(rgb, oracle.wiener(ll[:, :, None], 0.075, 32, 4)[:, :, 0], True)
    return oracle.modify_luminance(den, oracle.bilateral(oracle.compute_luminance(den), 2.0, 0.2, 0.4))


def run_bench_chain(td, dev, w, h, storage, seeds):
    import bench
    from torch_darktable.sharding import FrameStreams
    from torch_darktable.synthetic import synthetic_bayer
    from torch_darktable.torch_darktable_extension import concurrent_frames

    tap = _Tapped(td)
    dtype = bench.build_pipeline(tap, dev, w, h, storage, 'isp')[0]
    runner = FrameStreams(dev, lambda: bench.build_pipeline(tap, dev, w, h, storage, 'isp')[1], streams=3)
    inputs = [synthetic_bayer(h, w, seed=s, device=dev).to(dtype) for s in seeds]
    with concurrent_frames():
        outs = runner.run(inputs)
    torch.cuda.synchronize()
    assert len(tap.demosaiced) == len(tap.rgb) == len(tap.metrics) == len(inputs)
    for o, rgb in zip(outs, tap.rgb):
        assert o.dtype == torch.uint8 and o.shape == (h, w, 3) and rgb.dtype == dtype and rgb.shape == (h, w, 3)
    return inputs, outs, tap.rgb, tap.metrics, tap.demosaiced


@pytest.mark.parametrize('storage,shape', [('f16', (4096, 3072)), ('f32', (4096, 3072)), ('f32', (4098, 3041))])
def test_bench_chain_against_the_oracle_chain(td, oracle, dev, storage, shape):
    """f16 (what is benchmarked): the bounds of test_full_pipeline_12mp_fp16_vs_fp32_oracle -- |d| <= 2e-3 * max(R, G, B) per pixel and
    uint8 within 2 LSB with at most 1e-5 of the values above 1 LSB against the oracle chain; <= 2e-3 * max(|ref|, 0.05) per value
    against the oracle chain from the GPU's binary16 demosaic.  (The lightness replacement moves every channel of a pixel together, so
    a dark channel of a bright pixel carries the bright channels' binary16 rounding of the demosaic: per value against the oracle's
    fp32 demosaic that is up to 1.1e-2, 1.2e-3 even from the oracle's demosaic rounded to nearest; from the GPU's own demosaic every
    later stage stays within half a binary16 ulp, 4.9e-4.  The demosaic's binary16 result is checked by
    test_gpu_fullsize.py::test_rcd_12mp_fp16_fast_arithmetic.)  f32 (the sharp check: binary16 rounding hides differences of ~1e-4):
    the float result within 2 * TOL, uint8 within 1 LSB.  4098 x 3041: y-stream strips that end partway, scalar loads (W % 4 != 0),
    the bilateral tile kernel with VEC = 1.  Metrics: the accumulator's against oracle.image_metrics of the GPU's own float result."""
    w, h = shape
    assert oracle.bilateral_grid_size(w, h, 2.0, 0.2)[:2] == (math.ceil(w / 2) + 1, math.ceil(h / 2) + 1)  # cells of exactly 2 px
    inputs, outs, rgbs, metrics, gpu_demosaiced = run_bench_chain(td, dev, w, h, storage, [1234, 1235, 1236])
    wins = windows(w, h)
    worst = {'rel_px': 0.0, 'rel_val': 0.0, 'abs': 0.0, 'u8': 0, 'u8_gt1': 0, 'u8_n': 0}
    for i, (bayer, out, rgb, m, gdem) in enumerate(zip(inputs, outs, rgbs, metrics, gpu_demosaiced)):
        got_rgb = npy(rgb)
        ref_m = oracle.image_metrics([got_rgb], 8)
        assert np.allclose(npy(m), ref_m, rtol=2e-5, atol=1e-7), (i, npy(m), ref_m)
        demosaiced = oracle.rcd(npy(bayer), oracle.RGGB)
        gdem = npy(gdem) if storage == 'f16' else None
        got_u8 = out.cpu().numpy()
        for y0, y1, x0, x1 in wins:
            cy0, cy1, cx0, cx1 = max(y0 - M, 0), min(y1 + M, h), max(x0 - M, 0), min(x1 + M, w)
            assert cy0 % 8 == 0 and cx0 % 8 == 0 and (cx1 - cx0) % 2 == 0
            assert oracle.bilateral_grid_size(cx1 - cx0, cy1 - cy0, 2.0, 0.2)[:2] == (math.ceil((cx1 - cx0) / 2) + 1, math.ceil((cy1 - cy0) / 2) + 1)
            r = oracle_lab_chain(oracle, np.ascontiguousarray(demosaiced[cy0:cy1, cx0:cx1]))
            ref_u8 = oracle.tonemap('reinhard', r, npy(m), 0.75, 2.0, 1.0, 0.0)[y0 - cy0:y1 - cy0, x0 - cx0:x1 - cx0]
            ref = r[y0 - cy0:y1 - cy0, x0 - cx0:x1 - cx0]
            got = got_rgb[y0:y1, x0:x1]
            d = np.abs(got - ref)
            du8 = np.abs(got_u8[y0:y1, x0:x1].astype(np.int32) - ref_u8.astype(np.int32))
            where = f'frame {i} window {(y0, y1, x0, x1)}'
            worst['abs'] = max(worst['abs'], float(d.max()))
            worst['rel_px'] = max(worst['rel_px'], float((d / np.maximum(ref.max(-1, keepdims=True), 1e-3)).max()))
            if gdem is not None:  # per value: every stage after the demosaic, from the GPU's binary16 demosaic
                r2 = oracle_lab_chain(oracle, np.ascontiguousarray(gdem[cy0:cy1, cx0:cx1]))[y0 - cy0:y1 - cy0, x0 - cx0:x1 - cx0]
                worst['rel_val'] = max(worst['rel_val'], float((np.abs(got - r2) / np.maximum(np.abs(r2), 0.05)).max()))
            else:
                worst['rel_val'] = max(worst['rel_val'], float((d / np.maximum(np.abs(ref), 0.05)).max()))
            worst['u8'] = max(worst['u8'], int(du8.max()))
            worst['u8_gt1'] += int((du8 > 1).sum())
            worst['u8_n'] += du8.size
            if storage == 'f32':
                assert d.max() <= 2 * TOL, (where, d.max(), np.unravel_index(d.argmax(), d.shape))
                assert du8.max() <= 1, (where, du8.max())
            else:
                assert worst['rel_px'] < 2e-3 and worst['rel_val'] < 2e-3, (where, worst)
                assert du8.max() <= 2, (where, du8.max())
    if storage == 'f16':
        assert worst['u8_gt1'] <= 1e-5 * worst['u8_n'], worst
    print(f'\nbench chain {storage} {w}x{h}: measured {worst}')
