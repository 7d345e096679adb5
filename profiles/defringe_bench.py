"""Defringe.process (csrc/defringe.hip) at 12 MP beside a device copy of the same bytes, the same arithmetic composed from torch
operations, and Wavelet in chroma mode at two scales (the stage it would otherwise be confused with).

A 4096 x 3072 frame (coloured blocks under stripes, a clipped band with dark bars whose red and blue are blurred more than green,
Poisson-Gaussian noise), float32 and float16, at (R, S_r) = (6, 6) and (12, 8).  The share of fringed pixels is set through the
static mode: the threshold is the quantile of E that leaves about 1 %, 10 % and 50 % of the pixels above it; the global mode with
the default strength is measured as well and its share is reported.  On the same frame, in the same process:
  * copy: the frame in and out (out.copy_);
  * torch: replicate padding, every tap and every sample of the disc a slice of the padded plane, float32 throughout -- close to
    the stage's result but not its bits (the largest difference is printed);
  * Wavelet(scales=2, ycc=True).process.
Device time per call between two HIP events on one stream around a batch of back-to-back calls, after warm-up calls of the same
shape; three batches per figure, the fastest is reported and all are listed.  The time of each of the two launches comes from the
library's own event timer in a pass of its own (profile_enable).

  python3 profiles/defringe_bench.py [--warmup 5] [--iters 20] [--out profiles/r28/defringe_bench.txt]

On a shared machine run it with a time limit of its own, e.g.  timeout -k 10 400 python3 profiles/defringe_bench.py && next step.
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


def torch_composition(taps, sample_radius, strength, floor, static):
    """The stage from torch operations in the square-root domain, float32 arithmetic: a callable (H, W, 3) -> (H, W, 3)."""
    radius = len(taps) - 1
    disc = [(dy, dx) for dy in range(-sample_radius, sample_radius + 1) for dx in range(-sample_radius, sample_radius + 1) if dx * dx + dy * dy <= sample_radius ** 2]

    def padded(planes, r):
        return F.pad(planes[None], (r, r, r, r), mode='replicate')[0]

    def blur(planes):
        c, h, w = planes.shape
        p = F.pad(planes[None], (radius, radius, 0, 0), mode='replicate')[0]
        hor = taps[0] * planes
        for k in range(1, radius + 1):
            hor = hor + taps[k] * (p[:, :, radius - k:radius - k + w] + p[:, :, radius + k:radius + k + w])
        p = F.pad(hor[None], (0, 0, radius, radius), mode='replicate')[0]
        ver = taps[0] * hor
        for k in range(1, radius + 1):
            ver = ver + taps[k] * (p[:, radius - k:radius - k + h] + p[:, radius + k:radius + k + h])
        return ver

    def run(frame):
        h, w, _ = frame.shape
        t = frame.float().clamp_min(0.0).sqrt()
        y = (0.25 * t[..., 0] + 0.5 * t[..., 1]) + 0.25 * t[..., 2]
        c = torch.stack([t[..., 2] - t[..., 1], t[..., 0] - t[..., 1]])
        d = c - blur(c)
        e = d[0] * d[0] + d[1] * d[1]
        th = max(floor, strength) if static else torch.clamp_min(strength * e.clamp_max(1024.0).mean(), floor)
        wt = 1.0 / (e + th)
        s = sample_radius
        p = padded(torch.cat([wt[None] * c, wt[None]]), s)
        acc = torch.zeros_like(p[:, s:s + h, s:s + w])
        for dy, dx in disc:
            acc = acc + p[:, s + dy:s + dy + h, s + dx:s + dx + w]
        cb, cr = acc[0] / acc[2], acc[1] / acc[2]
        g = y - 0.25 * (cb + cr)
        new = torch.stack([g + cr, g, g + cb], dim=-1).clamp_min(0.0) ** 2
        return torch.where((e > th)[..., None], new, frame.float()).to(frame.dtype)

    return run


def scene(w, h, rng):
    yy, xx = np.mgrid[0:h, 0:w]
    x = rng.uniform(0.05, 0.8, (h // 24 + 1, w // 24 + 1, 3)).repeat(24, 0).repeat(24, 1)[:h, :w].astype(np.float32)
    x *= np.where((xx + 2 * yy) % 23 < 11, 1.0, 0.5)[..., None].astype(np.float32)
    # a backlit band: a sky that clips with dark slanted bars, red and blue wider than green
    top = slice(0, h // 3)
    for c, half in enumerate((4.5, 3.0, 6.0)):
        dist = np.abs((xx[top] + 0.3 * yy[top]) % 40 - 20)
        x[top, :, c] = np.clip(1.8 * np.clip((dist - half) / 3.0, 0.0, 1.0) + 0.05, 0.0, 1.0)
    x += (rng.normal(size=x.shape) * np.sqrt(4e-4 * np.abs(x) + 1e-5)).astype(np.float32)
    return x


def main():
    import torch_darktable as td
    from torch_darktable import _native

    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--size', type=int, nargs=2, default=(4096, 3072), metavar=('W', 'H'))
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'r28' / 'defringe_bench.txt'))
    a = ap.parse_args()
    assert a.warmup >= 5 and a.iters >= 20
    assert torch.cuda.is_available(), 'the measurement needs the GPU: there is no fallback'
    dev = torch.device('cuda', 0)
    w, h = a.size
    lines = []

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    frame = torch.from_numpy(scene(w, h, np.random.default_rng(7))).to(dev)
    for dtype in (torch.float32, torch.float16):
        x = frame.to(dtype)
        out = torch.empty_like(x)
        nbytes = 2 * x.numel() * x.element_size()   # the frame in and out
        copy_us, copy_batches = device_us(lambda: out.copy_(x), a.warmup, a.iters)
        emit({'size': [w, h], 'dtype': str(dtype), 'op': 'copy (the frame in and out)', 'us': round(copy_us, 1), 'us_batches': copy_batches, 'bytes': nbytes,
              'GB_per_s': round(nbytes / copy_us * 1e-3, 1)})
        wavelet = td.Wavelet.from_sigma(dev, (w, h), (0.01, 0.01, 0.01), scales=2, ycc=True)
        wav_us, wav_batches = device_us(lambda: wavelet.process(x), a.warmup, a.iters)
        emit({'size': [w, h], 'dtype': str(dtype), 'op': 'Wavelet(scales=2, ycc=True).process', 'us': round(wav_us, 1), 'us_batches': wav_batches,
              'over_copy': round(wav_us / copy_us, 2)})
        del wavelet
        for sigma, sample_radius in ((2.0, 6), (4.0, 8)):
            probe = td.Defringe(dev, (w, h), sigma=sigma, radius=sample_radius)
            e = probe.edge(x).flatten()
            sample = e[torch.randint(0, e.numel(), (1 << 22,), device=dev)]
            cases = [('global', 2.5, None)] + [('static', float(torch.quantile(sample, 1.0 - share)), share) for share in (0.01, 0.10, 0.50)]
            del e, sample, probe
            for mode, strength, aimed in cases:
                stage = td.Defringe(dev, (w, h), sigma=sigma, radius=sample_radius, strength=strength, mode=mode)
                us, batches = device_us(lambda: stage.process(x), a.warmup, a.iters)
                _native.profile_enable(True, 'tdk_defringe')
                for _ in range(a.iters):
                    stage.process(x)
                torch.cuda.synchronize()
                report = _native.profile_report()
                _native.profile_enable(False)
                per_launch = {name: round(ms * 1e3 / n, 1) for name, (n, ms) in sorted(report.items())}
                got, mask = stage.process(x, return_mask=True)
                s, th = (float(v) for v in stage.threshold())
                row = {'size': [w, h], 'dtype': str(dtype), 'op': f'Defringe.process mode={mode}', 'blur_radius': stage.blur_radius, 'sample_radius': sample_radius,
                       'fringed_share': round(float(mask.float().mean()), 4), 'aimed_share': aimed, 'threshold': float(f'{th:.4g}'), 'us': round(us, 1),
                       'us_batches': batches, 'launches': stage.launches, 'us_per_launch': per_launch, 'spec_bytes': nbytes, 'GB_per_s': round(nbytes / us * 1e-3, 1),
                       'over_copy': round(us / copy_us, 2), 'over_wavelet': round(us / wav_us, 2), 'lds_bytes': stage.lds_bytes(dtype)}
                if mode == 'global' or aimed == 0.10:   # the composition's time does not depend on the share: two of the four cases
                    compose = torch_composition(stage.taps, sample_radius, stage.strength, stage.floor, mode == 'static')
                    torch_us, torch_batches = device_us(lambda: compose(x), 5, 20)
                    diff = (got.float() - compose(x).float()).abs().max().item()
                    row.update({'torch_us': round(torch_us, 1), 'torch_us_batches': torch_batches, 'torch_over_stage': round(torch_us / us, 1),
                                'max_abs_difference_to_torch': float(f'{diff:.3g}')})
                    del compose
                emit(row)
                del stage, got, mask
                torch.cuda.empty_cache()
        del x, out
        torch.cuda.empty_cache()
    path = Path(a.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text('\n'.join([f'# profiles/defringe_bench.py --warmup {a.warmup} --iters {a.iters} on {torch.cuda.get_device_name(0)}', *lines]) + '\n')


if __name__ == '__main__':
    main()
