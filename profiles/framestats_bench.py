"""FrameStats.measure (csrc/framestats.hip) at 12 MP next to what a user would write today.

Two frames: a 4096 x 3072 x 3 float16 RGB frame and a 4096 x 3072 float32 mosaic (RGGB), each with natural-like contents (a gamma
distribution over the range, every lane on another bin) and flat (every lane on ONE bin: the worst case of an LDS histogram).
Settings: strides 1 and 8, 256 and 1024 bins.  Beside them, on the same frame in the same process:
  torch.histc per channel plus torch.quantile (three fractions) on the strided view, as a user would write the same measurement
    (float16 is converted first: neither takes it; the mosaic's four planes are sliced first);
  compute_image_bounds at the same stride (the minimum and maximum the processor normalises by today; RGB frames only);
  a device copy of the bytes the gather launch reads, as the floor (clone of the frame at stride 1, of every stride-th row at stride 8).
Device time per call between two HIP events on one stream around a batch of back-to-back calls, after warm-up calls of the same
shape; five batches per figure, the MEDIAN is reported and all are listed.  The three launches of a call are timed one by one through
the library's event timer in a pass of their own.  One process; run it under a time limit:

  timeout -k 10 600 python3 profiles/framestats_bench.py [--warmup 5] [--iters 20] [--out profiles/r15/framestats_bench.txt]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / 'torch-darktable_amd'))
import torch_darktable as td  # noqa: E402
from torch_darktable import _native  # noqa: E402

QUANTILES = (0.001, 0.5, 0.999)


def device_us(fn, warmup, iters, batches=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(batches):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1) * 1e3 / iters)
    return statistics.median(times), [round(t, 1) for t in times]


def torch_way(planes, bins, q):
    """histc per plane and quantile of each plane: the same measurement without the kernel (no pooled row, no counters)."""
    out = []
    for p in planes:
        p = p.float().reshape(-1)
        out.append(torch.histc(p, bins=bins, min=0.0, max=1.0))
        out.append(torch.quantile(p, q))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'r15' / 'framestats_bench.txt'))
    a = ap.parse_args()
    assert a.warmup >= 5 and a.iters >= 20
    dev = torch.device('cuda', 0)
    w, h = 4096, 3072
    lines = []

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    g = torch.Generator(device='cpu').manual_seed(15)
    q = torch.tensor(QUANTILES, device=dev)
    for kind in ('rgb float16', 'mosaic float32'):
        mosaic = kind.startswith('mosaic')
        shape = (h, w) if mosaic else (h, w, 3)
        natural = (torch.empty(shape).exponential_(1 / 0.12, generator=g) + torch.empty(shape).exponential_(1 / 0.12, generator=g)).clamp_(0, 1.5)   # gamma(2, 0.12)
        for content in ('natural', 'flat'):
            x = (natural if content == 'natural' else torch.full(shape, 0.6)).to(torch.float32 if mosaic else torch.float16).to(dev)
            for stride in (1, 8):
                rows = x.view(h // 2, 2, w)[::stride] if mosaic else x[::stride]   # what the gather launch reads: the sampled rows (row pairs)
                read_bytes = rows.numel() * x.element_size()
                head = {'frame': kind, 'content': content, 'size': [w, h], 'stride': stride, 'read_bytes': read_bytes}
                us, batches = device_us(lambda: rows.clone(), a.warmup, a.iters)
                copy_us = us
                emit({**head, 'op': 'copy of the bytes read (read + write)', 'us': round(us, 1), 'us_batches': batches, 'GB_per_s_read': round(read_bytes / us * 1e-3, 1)})
                for bins in (256, 1024):
                    fs = td.FrameStats(dev, (w, h), bayer_pattern=td.BayerPattern.RGGB if mosaic else None, bins=bins, stride=stride, quantiles=QUANTILES)
                    us, batches = device_us(lambda: fs.measure(x), a.warmup, a.iters)
                    _native.profile_enable(True, 'tdk_framestats')
                    for _ in range(a.iters):
                        fs.measure(x)
                    torch.cuda.synchronize()
                    launches = {k: round(ms * 1e3 / n, 1) for k, (n, ms) in _native.profile_report().items()}
                    _native.profile_enable(False)
                    emit({**head, 'op': f'FrameStats.measure bins={bins}', 'us': round(us, 1), 'us_batches': batches, 'GB_per_s_read': round(read_bytes / us * 1e-3, 1),
                          'copy_us': round(copy_us, 1), 'launch_us': launches, 'lds_bytes': fs.lds_bytes(), 'workspace_bytes': fs.workspace_bytes()})
                    if mosaic:
                        planes = [x[0::2, 0::2], x[0::2, 1::2], x[1::2, 0::2], x[1::2, 1::2]]
                        planes = [p[::stride, ::stride] for p in planes]
                    else:
                        planes = [x[::stride, ::stride, k] for k in range(3)]
                    try:
                        us, batches = device_us(lambda: torch_way(planes, bins, q), a.warmup, a.iters)
                        emit({**head, 'op': f'torch.histc + torch.quantile per plane bins={bins}', 'us': round(us, 1), 'us_batches': batches})
                    except RuntimeError as e:
                        emit({**head, 'op': f'torch.histc + torch.quantile per plane bins={bins}', 'error': str(e).splitlines()[0][:160]})
                if not mosaic:
                    us, batches = device_us(lambda: td.compute_image_bounds([x], stride=stride), a.warmup, a.iters)
                    emit({**head, 'op': 'compute_image_bounds', 'us': round(us, 1), 'us_batches': batches})
            del x
            torch.cuda.empty_cache()
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text('\n'.join([f'# profiles/framestats_bench.py --warmup {a.warmup} --iters {a.iters} on {torch.cuda.get_device_name(0)}', *lines]) + '\n')


if __name__ == '__main__':
    main()
