"""Dehaze.process (csrc/dehaze.hip) at 12 MP against a device copy of the same bytes and against the same arithmetic composed from
torch operations.

4096 x 3072 frames of float32 and float16, cell 8, dark_radius 1, radius 4, quantile 0.01 (K = 1966 of 196 608 cells), with the
estimate of the ambient light (five launches) and with the ambient light given (three).  On the same frames, in the same process:
  * copy: out.copy_(x), the frame in and the frame out once -- the stage reads the frame twice and writes it once, so 1.5 x the
    copy's bytes is what it has to move;
  * torch: clamp, max_pool2d of the negated frame and avg_pool2d to the cells, the windowed minimum as max_pool2d over a
    replicate-padded grid, topk for the threshold, the box passes as avg_pool2d, F.interpolate back to the pixels, the division --
    float32 throughout, close to the stage's result but not its bits.
Device time per call between two HIP events on one stream around a batch of back-to-back calls, after warm-up calls of the same
shape; three batches per figure, the fastest is reported and all are listed.  The time of each launch comes from the library's own
event timer in a pass of its own (profile_enable).

  python3 profiles/dehaze_bench.py [--warmup 5] [--iters 20] [--out profiles/r23/dehaze_bench.txt]

On a shared machine run it with a time limit of its own, e.g.  timeout -k 10 300 python3 profiles/dehaze_bench.py && next step.
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / 'torch-darktable_amd'))
import torch_darktable as td  # noqa: E402
from torch_darktable import _native  # noqa: E402


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


def torch_composition(dh, given):
    """The stage from torch operations, float32 arithmetic: a callable frame -> frame.  given: the ambient light, or None to estimate."""
    dev = dh.ambient.device
    s, rd, rg, eps = dh.cell, dh.dark_radius, dh.radius, dh.eps
    weights = torch.tensor(dh.weights, device=dev)

    def minwin(p, r):
        return -F.max_pool2d(F.pad(-p, (r, r, r, r), mode='replicate'), 2 * r + 1, stride=1)

    def box(p):
        return F.avg_pool2d(F.pad(p, (rg, rg, rg, rg), mode='replicate'), 2 * rg + 1, stride=1)

    def run(x):
        h, wd, _ = x.shape
        xf = x.float()
        grow = (0, -wd % s, 0, -h % s)
        planes = F.pad(xf.clamp_min(0).permute(2, 0, 1)[None], grow, mode='replicate')
        low, mean = -F.max_pool2d(-planes, s), F.avg_pool2d(planes, s)
        lum = (xf * weights).sum(-1).clamp_min(0)
        cells = F.avg_pool2d(F.pad(lum[None, None], grow, mode='replicate'), s)
        if given is None:
            dark = minwin(low.min(1, keepdim=True).values, rd).flatten()
            chosen = dark >= torch.topk(dark, dh.count).values[-1]
            ambient = (mean.flatten(2)[0] * chosen).sum(1) / chosen.sum()
        else:
            ambient = given[:3]
        ambient = ambient.clamp_min(2.0 ** -10)
        q = (low / ambient[None, :, None, None]).min(1, keepdim=True).values
        t = 1.0 - dh.strength * minwin(q, rd).clamp_max(1.0)
        ml, mt = box(cells), box(t)
        cov = box(cells * t) - ml * mt
        var = (box(cells * cells) - ml * ml).clamp_min(0)
        a = cov / (var + eps)
        b = mt - a * ml
        up = F.interpolate(torch.cat((box(a), box(b)), 1), scale_factor=s, mode='bilinear', align_corners=False)[0, :, :h, :wd]
        tp = (up[0] * lum + up[1]).clamp(dh.floor, 1.0)
        return ((xf - ambient) / tp[..., None] + ambient).clamp_min(0).to(x.dtype)

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--size', type=int, nargs=2, default=(4096, 3072), metavar=('W', 'H'))
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'r23' / 'dehaze_bench.txt'))
    a = ap.parse_args()
    assert a.warmup >= 5 and a.iters >= 20
    assert torch.cuda.is_available(), 'the measurement needs the GPU: there is no fallback'
    dev = torch.device('cuda', 0)
    w, h = a.size
    lines = []

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    # a textured scene with black pixels behind a veil that thins from the top to the bottom
    rng = np.random.default_rng(7)
    clear = rng.uniform(0.1, 0.8, (h // 48 + 1, w // 48 + 1, 3)).repeat(48, 0).repeat(48, 1)[:h, :w] * rng.uniform(0.5, 1.0, (h, w, 1))
    clear[rng.random((h, w)) < 0.05] = 0.0
    t = np.linspace(0.15, 0.95, h)[:, None, None]
    frame = torch.from_numpy((clear * t + np.array([0.8, 0.85, 0.9]) * (1 - t)).astype(np.float32)).to(dev)
    del clear
    for dtype in (torch.float32, torch.float16):
        x = frame.to(dtype)
        esz = x.element_size()
        out = torch.empty_like(x)
        copy_bytes = 2 * x.numel() * esz
        copy_us, copy_batches = device_us(lambda: out.copy_(x), a.warmup, a.iters)
        emit({'size': [w, h], 'dtype': str(dtype), 'op': 'copy (frame in, frame out)', 'us': round(copy_us, 1), 'us_batches': copy_batches, 'bytes': copy_bytes,
              'GB_per_s': round(copy_bytes / copy_us * 1e-3, 1)})
        dh = td.Dehaze(dev, (w, h))
        light = dh.estimate_ambient(x)
        for given, label in ((None, 'estimate'), (light, 'ambient given')):
            us, batches = device_us(lambda: dh.process(x, ambient=given), a.warmup, a.iters)
            _native.profile_enable(True, 'tdk_dehaze(')
            for _ in range(a.iters):
                dh.process(x, ambient=given)
            torch.cuda.synchronize()
            report = _native.profile_report()
            _native.profile_enable(False)
            per_launch = {name: round(ms * 1e3 / n, 1) for name, (n, ms) in sorted(report.items())}
            # the frame read twice and written once; the planes of step 1 written and read, a and b written and read, the dark channel too
            nbytes = 3 * x.numel() * esz + 4 * dh.cells * ((7 + 4 + 2 + 2) + (0 if given is not None else 3 + 1 + 5 * 1 + 3))
            compose = torch_composition(dh, given)
            torch_us, torch_batches = device_us(lambda: compose(x), a.warmup, a.iters)
            got, ref = dh.process(x, ambient=given).float(), compose(x).float()
            diff = (got - ref).abs().max().item()
            emit({'size': [w, h], 'dtype': str(dtype), 'op': f'Dehaze.process cell={dh.cell} dark_radius={dh.dark_radius} radius={dh.radius} count={dh.count}, {label}',
                  'us': round(us, 1), 'us_batches': batches, 'spec_bytes': nbytes, 'GB_per_s': round(nbytes / us * 1e-3, 1), 'us_per_launch': per_launch,
                  'sum_of_launches_us': round(sum(per_launch.values()), 1), 'over_copy': round(us / copy_us, 2), 'torch_us': round(torch_us, 1),
                  'torch_us_batches': torch_batches, 'torch_over_stage': round(torch_us / us, 1), 'max_abs_difference_to_torch': float(f'{diff:.3g}'),
                  'ambient': [round(v, 6) for v in dh.ambient.tolist()], 'workspace_bytes': dh.workspace_bytes(), 'lds_bytes': dh.lds_bytes(dtype)})
            del compose, got, ref
        del x, out, dh
        torch.cuda.empty_cache()
    path = Path(a.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text('\n'.join([f'# profiles/dehaze_bench.py --warmup {a.warmup} --iters {a.iters} on {torch.cuda.get_device_name(0)}', *lines]) + '\n')


if __name__ == '__main__':
    main()
