"""Highlights.process (csrc/highlights.hip) at 12 MP next to apply_white_balance, the kernel whose place it takes.

4096 x 3072 RGGB mosaics, float32 and float16 (the same type in and out), daylight gains (1.9, 1.0, 1.6), default parameters.  Three
frames: no clipped site, about 1 % and about 30 % of the sites clipped (round blobs that run into the saturation, as a sky or a
specular surface does).  On each: apply_white_balance, Highlights 'clip', Highlights 'opposed', and 'opposed' with a supplied
chrominance (no statistics launch).  Device time per call between two HIP events on one stream around a batch of back-to-back calls,
after warm-up calls of the same shape; three batches per figure, the fastest is reported and all are listed.  The time of each launch
comes from the library's own event timer in a pass of its own.  spec_bytes: the frame read once per launch and written once.

  python3 profiles/highlights_bench.py [--warmup 5] [--iters 20] [--out profiles/r13/highlights_bench.txt]
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / 'torch-darktable_amd'))
import torch_darktable as td  # noqa: E402
from torch_darktable import _native  # noqa: E402

GAINS = (1.9, 1.0, 1.6)


def device_us(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(3):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1) * 1e3 / iters)
    return min(times), [round(t, 1) for t in times]


def frame(h, w, fraction, dev):
    """A mosaic below 0.85 with round blobs that saturate at 1.0 over about `fraction` of the sites."""
    g = torch.Generator(device='cpu').manual_seed(11)
    base = 0.35 + 0.5 * torch.rand((h, w), generator=g)
    if fraction > 0:
        radius, n = 40.0, max(1, round(fraction * h * w / (3.14159 * 40.0 * 40.0)))
        ys, xs = torch.rand(n, generator=g) * h, torch.rand(n, generator=g) * w
        i, j = torch.arange(h, dtype=torch.float32)[:, None], torch.arange(w, dtype=torch.float32)[None, :]
        for y, x in zip(ys.tolist(), xs.tolist()):
            y0, y1, x0, x1 = max(int(y - 3 * radius), 0), min(int(y + 3 * radius), h), max(int(x - 3 * radius), 0), min(int(x + 3 * radius), w)
            d2 = (i[y0:y1] - y) ** 2 + (j[:, x0:x1] - x) ** 2
            base[y0:y1, x0:x1] += 1.2 * torch.exp(-d2 / (2 * (radius / 1.2) ** 2))
    return base.clamp_(max=1.0).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'r13' / 'highlights_bench.txt'))
    a = ap.parse_args()
    assert a.warmup >= 5 and a.iters >= 20
    dev = torch.device('cuda', 0)
    w, h = 4096, 3072
    gains = torch.tensor(GAINS, dtype=torch.float32, device=dev)
    lines = []

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    for fraction in (0.0, 0.01, 0.30):
        base = frame(h, w, fraction, dev)
        for dtype in (torch.float32, torch.float16):
            x = base.to(dtype)
            esz = x.element_size()
            clipped = float((x >= 0.98).float().mean())
            head = {'size': [w, h], 'dtype': str(dtype).split('.')[-1], 'clipped_fraction': round(clipped, 4)}
            wb_us, wb_batches = device_us(lambda: td.apply_white_balance(x, gains, td.BayerPattern.RGGB), a.warmup, a.iters)
            emit({**head, 'op': 'apply_white_balance', 'us': round(wb_us, 1), 'us_batches': wb_batches, 'GB_per_s': round(2 * esz * w * h / wb_us * 1e-3, 1)})
            clip = td.Highlights(dev, (w, h), td.BayerPattern.RGGB, mode='clip')
            us, batches = device_us(lambda: clip.process(x, gains, out_dtype=dtype), a.warmup, a.iters)
            emit({**head, 'op': 'Highlights clip', 'us': round(us, 1), 'us_batches': batches, 'over_white_balance': round(us / wb_us, 2)})
            hl = td.Highlights(dev, (w, h), td.BayerPattern.RGGB)
            chroma = hl.chrominance(x, gains)
            total, cnt = hl.statistics(x, gains)
            for label, kw, launches in (('Highlights opposed', {}, 2), ('Highlights opposed, chrominance supplied', {'chrominance': chroma}, 1)):
                us, batches = device_us(lambda: hl.process(x, gains, out_dtype=dtype, **kw), a.warmup, a.iters)
                _native.profile_enable(True, 'tdk_highlights(')
                for _ in range(a.iters):
                    hl.process(x, gains, out_dtype=dtype, **kw)
                torch.cuda.synchronize()
                report = _native.profile_report()
                _native.profile_enable(False)
                per_launch = {name: round(ms * 1e3 / n, 1) for name, (n, ms) in sorted(report.items())}
                nbytes = (launches * esz + esz) * w * h
                emit({**head, 'op': label, 'us': round(us, 1), 'us_batches': batches, 'spec_bytes': nbytes, 'GB_per_s': round(nbytes / us * 1e-3, 1),
                      'us_per_launch': per_launch, 'over_white_balance': round(us / wb_us, 2), 'chrominance': [round(v, 5) for v in chroma.tolist()],
                      'cnt': cnt.tolist(), 'lds_bytes': hl.lds_bytes(), 'workspace_bytes': hl.workspace_bytes()})
            del x, clip, hl
        del base
        torch.cuda.empty_cache()
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text('\n'.join([f'# profiles/highlights_bench.py --warmup {a.warmup} --iters {a.iters} on {torch.cuda.get_device_name(0)}', *lines]) + '\n')


if __name__ == '__main__':
    main()
