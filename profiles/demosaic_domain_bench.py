"""The kernels that tests/test_gpu_demosaic_domain.py changed, alone, at 12 MP on the finite synthetic scene (their fast paths):
bilinear5x5_demosaic, PostProcess colour smoothing (3 passes: one launch) and PPG with the pre-median, float32 and float16 storage.

  python profiles/demosaic_domain_bench.py [--batches 5] [--iters 40]

Device microseconds per call between two events around `iters` calls after a warm-up, one figure per batch and the median; run
once per library (`TDK_LIB_PATH`) for an A/B."""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / 'torch-darktable_amd'))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, default=5)
    ap.add_argument('--iters', type=int, default=40)
    a = ap.parse_args()
    import torch_darktable as td
    from torch_darktable.synthetic import synthetic_bayer, synthetic_rgb

    dev = torch.device('cuda', 0)
    w, h = 4096, 3072
    bayer = synthetic_bayer(h, w, seed=1234, device=dev)
    rgb = synthetic_rgb(h, w, 1234, dev, 0.02)
    assert torch.isfinite(bayer).all() and torch.isfinite(rgb).all()
    smooth = td.PostProcess(dev, (w, h), td.BayerPattern.RGGB, color_smoothing_passes=3)
    ppg = td.PPG(dev, (w, h), td.BayerPattern.RGGB, median_threshold=1.5)
    ops = [('bilinear5x5', lambda x: td.bilinear5x5_demosaic(x, td.BayerPattern.RGGB), bayer),
           ('smoothing x3', smooth.process, rgb),
           ('ppg median 1.5', ppg.process, bayer)]
    for name, fn, x32 in ops:
        for storage, x in (('f32', x32), ('f16', x32.half())):
            for _ in range(5):
                fn(x)
            torch.cuda.synchronize()
            us = []
            for _ in range(a.batches):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.iters):
                    fn(x)
                t1.record()
                torch.cuda.synchronize()
                us.append(t0.elapsed_time(t1) * 1000.0 / a.iters)
            print(json.dumps({'op': name, 'storage': storage, 'us_per_call': [round(u, 1) for u in us], 'median_us': round(statistics.median(us), 1)}), flush=True)


if __name__ == '__main__':
    main()
