"""Sharpen.process (csrc/sharpen.hip) at 12 MP against the torch composition a user would write without it.

A 4096 x 3072 x 3 frame; uint8 in luminance mode (the pipeline's call) and float16 per channel; sigma 1 (radius 3) and sigma 4
(radius 12); threshold and halo limit on.  The yardstick is the composition in torch on the same frame: conversion to float32 (and
the luminance), replicate pad, two conv2d, the elementwise part (threshold, amount, 3x3 extrema by max_pool2d, clamp), conversion
back.  Device time per call between two HIP events on one stream around a batch of back-to-back calls, after warm-up calls of the
same shape; three batches per figure, the fastest is reported and all are listed.  The share of the copy rate is on the
algorithmic bytes, 2 C sizeof per pixel (every element read once and written once), against a device-to-device copy_ of a 256 MB
buffer timed the same way in the same process (read + write bytes per second).

  python3 profiles/sharpen_bench.py [--size 4096x3072] [--warmup 5] [--iters 20]
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as nnf

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / 'torch-darktable_amd'))
import torch_darktable as td  # noqa: E402


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


def torch_sharpen(image, s):
    """The same operator from torch ops (float32 arithmetic, its own summation order: close to Sharpen, not its bits)."""
    scale = 255.0 if image.dtype == torch.uint8 else 1.0
    x = image.permute(2, 0, 1).float()                                            # (C, H, W)
    sig = (0.2126729 * x[0] + 0.7151522 * x[1] + 0.0721750 * x[2])[None] if s.luma else x
    taps = torch.tensor(s.weights, device=image.device)
    kernel = torch.cat([taps.flip(0)[:-1], taps])
    r = s.radius
    blur = nnf.conv2d(nnf.conv2d(nnf.pad(sig[:, None], (r, r, r, r), mode='replicate'), kernel.view(1, 1, 1, -1)), kernel.view(1, 1, -1, 1))[:, 0]
    d = sig - blur
    t = s.threshold * scale
    y = x + s.amount * torch.sign(d) * (d.abs() - t).clamp_min(0.0)
    if s.overshoot is not None:
        padded = nnf.pad(x[None], (1, 1, 1, 1), mode='replicate')
        hi, lo = nnf.max_pool2d(padded, 3, 1)[0], -nnf.max_pool2d(-padded, 3, 1)[0]
        y = torch.minimum(torch.maximum(y, lo - s.overshoot * scale), hi + s.overshoot * scale)
    y = y.permute(1, 2, 0)
    return y.clamp(0, 255).round().to(torch.uint8) if image.dtype == torch.uint8 else y.to(image.dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', default='4096x3072')
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    a = ap.parse_args()
    assert a.warmup >= 5 and a.iters >= 20
    w, h = map(int, a.size.split('x'))
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(7)

    src = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    copy_us, copy_batches = device_us(lambda: dst.copy_(src), a.warmup, a.iters)
    copy_rate = 2 * src.numel() / copy_us * 1e-3   # GB/s, read + write
    base = {'size': [w, h], 'copy_256MB_us': round(copy_us, 1), 'copy_us_batches': copy_batches, 'copy_GB_per_s_read_plus_write': round(copy_rate, 1)}
    print(json.dumps(base), flush=True)
    del src, dst

    frames = {'uint8': torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).to(dev),
              'float16': torch.from_numpy(rng.random((h, w, 3), dtype=np.float32)).to(dev).half()}
    rows = []
    for name, luma in (('uint8', True), ('float16', False)):
        x = frames[name]
        for sigma in (1.0, 4.0):
            s = td.Sharpen(dev, sigma=sigma, amount=1.0, threshold=0.004, luma=luma, overshoot=0.02)
            close = (s.process(x).float() - torch_sharpen(x, s).float()).abs().max().item()
            us, batches = device_us(lambda: s.process(x), a.warmup, a.iters)
            torch_us, torch_batches = device_us(lambda: torch_sharpen(x, s), a.warmup, a.iters)
            nbytes = 2 * x.numel() * x.element_size()
            row = {'dtype': name, 'luma': luma, 'sigma': sigma, 'radius': s.radius, 'us': round(us, 1), 'us_batches': batches,
                   'GB_per_s': round(nbytes / us * 1e-3, 1), 'share_of_copy_rate': round(nbytes / us * 1e-3 / copy_rate, 3), 'algorithmic_bytes': nbytes,
                   'lds_bytes': s.lds_bytes(3, x.dtype), 'torch_composition_us': round(torch_us, 1), 'torch_us_batches': torch_batches,
                   'torch_over_sharpen': round(torch_us / us, 2), 'max_abs_difference_to_torch': close}
            rows.append(row)
            print(json.dumps(row), flush=True)
    print(json.dumps({'warmup': a.warmup, 'iters': a.iters, **base, 'rows': rows}))


if __name__ == '__main__':
    main()
