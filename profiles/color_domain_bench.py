"""Device time of the kernels that the whole-domain colour fixes touch: the four tone mappers (LEAN and full instantiation) and
modify_hsl on a 4096 x 3072 frame, median of 40 calls between events.  Run once per library (TDK_LIB_PATH selects a variant build)
and compare:  python profiles/color_domain_bench.py;  TDK_LIB_PATH=parent.so python profiles/color_domain_bench.py"""
import json
import os
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / 'torch-darktable_amd'))
import torch_darktable as td  # noqa: E402


def timed(fn, n=40):
    for _ in range(5):
        fn()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return sorted(ts)[n // 2]


def main():
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    m = torch.tensor([-2.3, 0.18, 0.21, 0.19, 0.15], device=dev)
    rows = {}
    for dt in (torch.float16, torch.float32):
        rgb = torch.rand(3072, 4096, 3, device=dev).to(dt)
        tag = 'f16' if dt == torch.float16 else 'f32'
        for vib in (0.0, 0.4):
            p = td.TonemapParameters(0.75, 2.0, 1.0, vib)
            form = 'lean' if vib == 0.0 else 'full'
            rows[f'reinhard_{form}_{tag}'] = timed(lambda: td.reinhard_tonemap(rgb, m, p))
            rows[f'linear_{form}_{tag}'] = timed(lambda: td.linear_tonemap(rgb, m, p))
            rows[f'aces_{form}_{tag}'] = timed(lambda: td.aces_tonemap(rgb, p))
            rows[f'adaptive_aces_{form}_{tag}'] = timed(lambda: td.aces_tonemap(rgb, p, m))
        rows[f'modify_hsl_{tag}'] = timed(lambda: td.modify_hsl(rgb, 0.1, 0.3, -0.2))
    print(json.dumps({'library': os.environ.get('TDK_LIB_PATH', 'in-tree'), 'unit': 'us per 12.6 MP call', **{k: round(v, 1) for k, v in rows.items()}}))


if __name__ == '__main__':
    main()
