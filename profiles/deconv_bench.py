"""Deconvolve.process (csrc/deconv.hip) at 12 MP against a device copy of the same bytes and against the same arithmetic composed
from torch operations, at every number F of fused iterations that was built for the radius.

4096 x 3072 frames of three channels, float32 and float16, N = 8 iterations, threshold 0.02, max_gain 4; sigma 0.7 (radius 3: F = 1
and 2), and with --all-radii also sigma 0.3 (radius 1: F = 1, 2, 4), sigma 1.2 (radius 4: F = 1, 2) and sigma 2 (radius 6: F = 1).
On the same frames, in the same process:
  * copy: out.copy_(x), the frame in and the frame out once;
  * torch: the luminance as a weighted sum, every blur as two conv2d over a replicate-padded plane, the division, the mask from
    max_pool2d, the gain -- float32 throughout, close to the stage's result but not its bits.
Device time per call between two HIP events on one stream around a batch of back-to-back calls, after warm-up calls of the same
shape; three batches per figure, the fastest is reported and all are listed.  The time of each launch comes from the library's own
event timer in a pass of its own (profile_enable).  F is forced through the flags (Deconvolve.fused_iterations); the row of the
library's own choice is marked "default".

  python3 profiles/deconv_bench.py [--warmup 5] [--iters 20] [--all-radii] [--out profiles/r25/deconv_bench.txt]

On a shared machine run it with a time limit of its own, e.g.  timeout -k 10 300 python3 profiles/deconv_bench.py && next step.
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
from torch_darktable.deconvolve import BUILT_FUSED  # noqa: E402


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


def torch_composition(d, dev):
    """The stage from torch operations, float32 arithmetic: a callable frame -> frame."""
    taps = torch.tensor(d.taps[:0:-1] + d.taps, device=dev)
    kx, ky = taps.view(1, 1, 1, -1), taps.view(1, 1, -1, 1)
    r = d.radius
    weights = torch.tensor(d.weights, device=dev)
    tiny = 2.0 ** -20

    def blur(p):
        return F.conv2d(F.pad(F.conv2d(F.pad(p, (r, r, 0, 0), mode='replicate'), kx), (0, 0, r, r), mode='replicate'), ky)

    def run(x):
        xf = x.float()
        o = (xf * weights).sum(-1).clamp_min(tiny)[None, None]
        u = o
        for _ in range(d.iterations):
            u = u * blur(o / blur(u).clamp_min(tiny))
        if d.threshold is not None:
            padded = F.pad(o, (1, 1, 1, 1), mode='replicate')
            e = ((F.max_pool2d(padded, 3, stride=1).sqrt() - (-F.max_pool2d(-padded, 3, stride=1)).sqrt() - d.threshold) / d.threshold).clamp(0.0, 1.0)
            u = o + e * e * (3.0 - 2.0 * e) * (u - o)
        g = (u / o).clamp(1.0 / d.max_gain, d.max_gain)[0, 0]
        return (xf * g[..., None]).to(x.dtype)

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--size', type=int, nargs=2, default=(4096, 3072), metavar=('W', 'H'))
    ap.add_argument('--all-radii', action='store_true')
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'r25' / 'deconv_bench.txt'))
    a = ap.parse_args()
    assert a.warmup >= 5 and a.iters >= 20
    assert torch.cuda.is_available(), 'the measurement needs the GPU: there is no fallback'
    dev = torch.device('cuda', 0)
    w, h = a.size
    lines = []

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    # blocks and fine stripes, blurred a little by averaging neighbours, with noise
    rng = np.random.default_rng(7)
    sharp = rng.uniform(0.05, 0.9, (h // 24 + 1, w // 24 + 1, 3)).repeat(24, 0).repeat(24, 1)[:h, :w] + 0.1 * ((np.arange(w) // 2) % 2)[None, :, None]
    sharp = 0.5 * sharp + 0.25 * (np.roll(sharp, 1, 1) + np.roll(sharp, -1, 1))
    frame = torch.from_numpy((sharp + rng.normal(0.0, 0.004, (h, w, 3))).astype(np.float32)).to(dev)
    del sharp
    sigmas = (0.7, 0.3, 1.2, 2.0) if a.all_radii else (0.7,)
    for dtype in (torch.float32, torch.float16):
        x = frame.to(dtype)
        esz = x.element_size()
        out = torch.empty_like(x)
        copy_bytes = 2 * x.numel() * esz
        copy_us, copy_batches = device_us(lambda: out.copy_(x), a.warmup, a.iters)
        emit({'size': [w, h], 'dtype': str(dtype), 'op': 'copy (frame in, frame out)', 'us': round(copy_us, 1), 'us_batches': copy_batches, 'bytes': copy_bytes,
              'GB_per_s': round(copy_bytes / copy_us * 1e-3, 1)})
        for sigma in sigmas:
            d = td.Deconvolve(dev, (w, h), sigma=sigma, iterations=8)
            default = d.fused_iterations
            compose = torch_composition(d, dev)
            torch_us, torch_batches = device_us(lambda: compose(x), a.warmup, a.iters)
            ref = compose(x).float()
            for fused in (f for f, rmax in BUILT_FUSED.items() if d.radius <= rmax):
                d.fused_iterations = fused
                us, batches = device_us(lambda: d.process(x), a.warmup, a.iters)
                _native.profile_enable(True, 'tdk_deconv(')
                for _ in range(a.iters):
                    d.process(x)
                torch.cuda.synchronize()
                report = _native.profile_report()
                _native.profile_enable(False)
                per_launch = {name: round(ms * 1e3 / n, 1) for name, (n, ms) in sorted(report.items())}
                # every launch reads the frame; all but the first read a plane, all but the last write one; the last writes the frame
                nbytes = x.numel() * esz * (d.launches + 1) + 4 * w * h * 2 * (d.launches - 1)
                diff = (d.process(x).float() - ref).abs().max().item()
                emit({'size': [w, h], 'dtype': str(dtype), 'op': f'Deconvolve.process sigma={sigma} radius={d.radius} iterations={d.iterations} F={fused}' + (' (default)' if fused == default else ''),
                      'us': round(us, 1), 'us_batches': batches, 'launches': d.launches, 'us_per_iteration': round(us / d.iterations, 1), 'spec_bytes': nbytes,
                      'GB_per_s': round(nbytes / us * 1e-3, 1), 'us_per_launch': per_launch, 'over_copy': round(us / copy_us, 2), 'torch_us': round(torch_us, 1),
                      'torch_us_batches': torch_batches, 'torch_over_stage': round(torch_us / us, 1), 'max_abs_difference_to_torch': float(f'{diff:.3g}'),
                      'workspace_bytes': d.workspace_bytes(), 'lds_bytes': d.lds_bytes(dtype, 3)})
            del compose, ref, d
        del x, out
        torch.cuda.empty_cache()
    path = Path(a.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text('\n'.join([f'# profiles/deconv_bench.py --warmup {a.warmup} --iters {a.iters}{" --all-radii" if a.all_radii else ""} on {torch.cuda.get_device_name(0)}', *lines]) + '\n')


if __name__ == '__main__':
    main()
