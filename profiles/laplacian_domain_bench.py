"""Laplacian.process at 12 MP with and without the clarity term (the two instantiations of the curve), float32 and float16 storage.

  python profiles/laplacian_domain_bench.py [--batches 5] [--iters 40]

Device microseconds per call between two events around `iters` calls, one line per batch and the median; run once per library
(`TDK_LIB_PATH`, or the in-tree library swapped) for an A/B.  profiles/op_bench.py times the clarity form only."""
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
    from torch_darktable.synthetic import synthetic_rgb

    dev = torch.device('cuda', 0)
    w, h = 4096, 3072
    lum32 = td.compute_luminance(synthetic_rgb(h, w, 1234, dev, 0.02))
    for clarity in (0.0, 0.2):
        lap = td.Laplacian(dev, (w, h), td.LaplacianParams(6, 0.2, 0.8, 1.2, clarity))
        for name, x in (('f32', lum32), ('f16', lum32.half())):
            for _ in range(5):
                lap.process(x)
            torch.cuda.synchronize()
            us = []
            for _ in range(a.batches):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.iters):
                    lap.process(x)
                t1.record()
                torch.cuda.synchronize()
                us.append(t0.elapsed_time(t1) * 1000.0 / a.iters)
            print(json.dumps({'clarity': clarity, 'storage': name, 'us_per_call': [round(u, 1) for u in us], 'median_us': round(statistics.median(us), 1)}), flush=True)


if __name__ == '__main__':
    main()
