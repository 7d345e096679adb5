"""LMMSE.process (csrc/lmmse.hip) at 12 MP beside the other demosaics of the same frame, a device copy of the same bytes and the
same arithmetic composed from torch operations.

A 4096 x 3072 RGGB mosaic (blocks, a slanted edge, fine stripes, a colour cast per CFA site, Poisson-Gaussian noise), float32 and
float16, both domains.  On the same frame, in the same process:
  * RCD.process and PPG.process;
  * copy: one plane in, three planes out (out.copy_ of the mosaic expanded to three channels);
  * torch: the frame reflect-padded by the apron, every tap a torch.roll, float32 throughout -- close to the stage's result but not
    its bits (the largest difference is printed).
Device time per call between two HIP events on one stream around a batch of back-to-back calls, after warm-up calls of the same
shape; three batches per figure, the fastest is reported and all are listed.  The time of the one launch comes from the library's
own event timer in a pass of its own (profile_enable).

  python3 profiles/lmmse_bench.py [--warmup 5] [--iters 20] [--out profiles/r27/lmmse_bench.txt]

On a shared machine run it with a time limit of its own, e.g.  timeout -k 10 300 python3 profiles/lmmse_bench.py && next step.
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

APRON = 11


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


def torch_composition(green00: bool, red_row0: bool, linear: bool):
    """The stage from torch operations, float32 arithmetic: a callable (H, W) mosaic -> (H, W, 3).  green00: the site (0, 0) is green;
    red_row0: row 0 holds the red sites.  Sizes of at least 12 per axis (one reflection)."""
    w_ = np.exp(-np.arange(5, dtype=np.float64) ** 2 / 8.0)
    g = [float(v) for v in (w_ / (w_[0] + 2.0 * w_[1:].sum())).astype(np.float32)]

    def pair(a, k, axis):
        return torch.roll(a, k, axis) + torch.roll(a, -k, axis)

    def window(a, axis):
        s = a
        for k in range(1, 5):
            s = s + pair(a, k, axis)
        return s

    def direction(t, green, axis):
        e = (0.5 * pair(t, 1, axis) - 0.25 * pair(t, 2, axis)) + 0.5 * t
        d = torch.where(green, t - e, e - t)
        p = g[0] * d
        for k in range(1, 5):
            p = p + g[k] * pair(d, k, axis)
        mu = window(p, axis) * (1.0 / 9.0)
        s = (p - mu) ** 2
        for k in range(1, 5):
            s = s + ((torch.roll(p, k, axis) - mu) ** 2 + (torch.roll(p, -k, axis) - mu) ** 2)
        vx, vn = 1e-7 + s, 1e-7 + window((d - p) ** 2, axis)
        return (p * vn + d * vx) / (vx + vn), (vx * vn) / (vx + vn)

    def run(mosaic):
        m = mosaic.float()
        h, w = m.shape
        t = m if linear else m.clamp_min(0.0).sqrt()
        t = F.pad(t[None, None], (APRON, APRON, APRON, APRON), mode='reflect')[0, 0]
        ys = torch.arange(-APRON, h + APRON, device=m.device)[:, None]
        xs = torch.arange(-APRON, w + APRON, device=m.device)[None, :]
        green = ((ys + xs) % 2 == 0) == green00
        red_row = (ys % 2 == 0) == red_row0
        xh, vh = direction(t, green, 1)
        xv, vv = direction(t, green, 0)
        D = (xh * vv + xv * vh) / (vh + vv)
        G = torch.where(green, t, t + D)
        along, across = t - 0.5 * pair(D, 1, 1), t - 0.5 * pair(D, 1, 0)
        other = G - 0.25 * (pair(torch.roll(D, 1, 0), 1, 1) + pair(torch.roll(D, -1, 0), 1, 1))
        red = torch.where(green, torch.where(red_row, along, across), torch.where(red_row, t, other))
        blue = torch.where(green, torch.where(red_row, across, along), torch.where(red_row, other, t))
        est = torch.stack([red, G, blue], dim=-1)[APRON:APRON + h, APRON:APRON + w]
        if not linear:
            est = est.clamp_min(0.0) ** 2
        # the own colour is the sample itself
        colour = torch.where(green, 1, torch.where(red_row, 0, 2))[APRON:APRON + h, APRON:APRON + w]
        own = F.one_hot(colour, 3).bool()
        return torch.where(own, m[..., None], est).to(mosaic.dtype)

    return run


def main():
    import torch_darktable as td
    from torch_darktable import _native

    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--size', type=int, nargs=2, default=(4096, 3072), metavar=('W', 'H'))
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'r27' / 'lmmse_bench.txt'))
    a = ap.parse_args()
    assert a.warmup >= 5 and a.iters >= 20
    assert torch.cuda.is_available(), 'the measurement needs the GPU: there is no fallback'
    dev = torch.device('cuda', 0)
    w, h = a.size
    lines = []

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:h, 0:w]
    clean = rng.uniform(0.05, 0.8, (h // 24 + 1, w // 24 + 1)).repeat(24, 0).repeat(24, 1)[:h, :w] * np.where((xx + 2 * yy) % 23 < 11, 1.0, 0.5) + 0.1 * ((xx // 2) % 2)
    clean = clean * np.array([[0.7, 1.0], [1.0, 0.55]])[yy % 2, xx % 2]
    frame = torch.from_numpy((clean + rng.normal(size=(h, w)) * np.sqrt(4e-4 * clean + 1e-5)).astype(np.float32)).to(dev)
    del clean, yy, xx
    pattern = td.BayerPattern.RGGB
    rcd, ppg = td.RCD(dev, (w, h), pattern), td.PPG(dev, (w, h), pattern)
    for dtype in (torch.float32, torch.float16):
        x = frame.to(dtype)
        esz = x.element_size()
        out = torch.empty((h, w, 3), dtype=dtype, device=dev)
        nbytes = 4 * w * h * esz   # one plane in, three out
        copy_us, copy_batches = device_us(lambda: out.copy_(x[..., None].expand(h, w, 3)), a.warmup, a.iters)
        emit({'size': [w, h], 'dtype': str(dtype), 'op': 'copy (one plane in, three out)', 'us': round(copy_us, 1), 'us_batches': copy_batches, 'bytes': nbytes,
              'GB_per_s': round(nbytes / copy_us * 1e-3, 1)})
        x1 = x.unsqueeze(-1)
        rcd_us, rcd_batches = device_us(lambda: rcd.process(x1), a.warmup, a.iters)
        emit({'size': [w, h], 'dtype': str(dtype), 'op': 'RCD.process', 'us': round(rcd_us, 1), 'us_batches': rcd_batches, 'over_copy': round(rcd_us / copy_us, 2)})
        ppg_us, ppg_batches = device_us(lambda: ppg.process(x1), a.warmup, a.iters)
        emit({'size': [w, h], 'dtype': str(dtype), 'op': 'PPG.process', 'us': round(ppg_us, 1), 'us_batches': ppg_batches, 'over_copy': round(ppg_us / copy_us, 2)})
        for domain in ('sqrt', 'linear'):
            stage = td.LMMSE(dev, (w, h), pattern, domain=domain)
            compose = torch_composition(False, True, domain == 'linear')
            torch_us, torch_batches = device_us(lambda: compose(x), a.warmup, a.iters)
            ref = compose(x).float()
            us, batches = device_us(lambda: stage.process(x), a.warmup, a.iters)
            _native.profile_enable(True, 'tdk_lmmse')
            for _ in range(a.iters):
                stage.process(x)
            torch.cuda.synchronize()
            report = _native.profile_report()
            _native.profile_enable(False)
            per_launch = {name: round(ms * 1e3 / n, 1) for name, (n, ms) in sorted(report.items())}
            got = stage.process(x).float()
            diff = (got - ref).abs().max().item()
            emit({'size': [w, h], 'dtype': str(dtype), 'op': f'LMMSE.process domain={domain}', 'us': round(us, 1), 'us_batches': batches, 'launches': 1,
                  'us_per_launch': per_launch, 'spec_bytes': nbytes, 'GB_per_s': round(nbytes / us * 1e-3, 1), 'over_copy': round(us / copy_us, 2),
                  'over_rcd': round(us / rcd_us, 2), 'over_ppg': round(us / ppg_us, 2), 'torch_us': round(torch_us, 1), 'torch_us_batches': torch_batches,
                  'torch_over_stage': round(torch_us / us, 1), 'max_abs_difference_to_torch': float(f'{diff:.3g}'), 'lds_bytes': stage.lds_bytes(dtype)})
            del compose, ref, got, stage
        del x, x1, out
        torch.cuda.empty_cache()
    path = Path(a.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text('\n'.join([f'# profiles/lmmse_bench.py --warmup {a.warmup} --iters {a.iters} on {torch.cuda.get_device_name(0)}', *lines]) + '\n')


if __name__ == '__main__':
    main()
