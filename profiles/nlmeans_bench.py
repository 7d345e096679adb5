"""NLMeans.process (csrc/nlmeans.hip) at 12 MP: device time per call between two HIP events around a batch of back-to-back calls,
for C = 1 and C = 3, float32 and float16 storage, (S, P) in {(7, 2), (5, 2), (3, 1)}.  Beside each time: the offsets per pixel and
the time per pixel and offset, the figure the issue floor in DESIGN.md is compared with.

  python3 profiles/nlmeans_bench.py [--size 4096x3072] [--iters 10] [--radii 7,2 5,2 3,1]
"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / 'torch-darktable_amd'))
import torch_darktable as td  # noqa: E402
from torch_darktable._native import lib  # noqa: E402
from torch_darktable.synthetic import synthetic_rgb  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', default='4096x3072')
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--radii', nargs='+', default=['7,2', '5,2', '3,1'])
    a = ap.parse_args()
    w, h = map(int, a.size.split('x'))
    dev = torch.device('cuda', 0)
    rgb = synthetic_rgb(h, w, 5, dev, 0.03)
    out = {'size': [w, h], 'iters': a.iters, 'rows': []}
    for radii in a.radii:
        s, p = map(int, radii.split(','))
        nlm = td.NLMeans(dev, (w, h), s, p)
        for c in (3, 1):
            for dtype in (torch.float32, torch.float16):
                x = (rgb if c == 3 else rgb[:, :, 1:2]).to(dtype).contiguous()
                for _ in range(2):
                    nlm.process(x, 0.1)
                torch.cuda.synchronize()
                times = []
                for _ in range(3):   # three batches: the spread says how far to trust the figure
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    for _ in range(a.iters):
                        nlm.process(x, 0.1)
                    t1.record()
                    t1.synchronize()
                    times.append(t0.elapsed_time(t1) * 1e3 / a.iters)
                us = min(times)
                offsets = (2 * s + 1) ** 2
                row = {'S': s, 'P': p, 'C': c, 'dtype': str(dtype).split('.')[1], 'us_per_call': round(us, 1), 'us_batches': [round(t, 1) for t in times],
                       'offsets': offsets, 'ps_per_pixel_offset': round(us * 1e6 / (w * h * offsets), 3), 'MP_per_s': round(w * h / us, 1),
                       'lds_bytes': int(lib.tdk_nlmeans_lds_bytes(s, p, c))}
                out['rows'].append(row)
                print(json.dumps(row), flush=True)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
