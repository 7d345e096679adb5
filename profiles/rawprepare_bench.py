"""RawPrepare.process_packed (csrc/rawprepare.hip) at 12 MP against what the head of the chain runs without it.

A 4096 x 3072 Packed12 frame, float32 and float16 output, three configurations:
  identity    black = 0, white = 4095, no clip: the bits of decode12_float (the plain streaming form, no LDS)
  no_defects  black and white level, a 33 x 25 gain grid, white balance and clip (streaming form with the grid records in LDS)
  full        the same plus hot and dead pixel correction (the tile form: 128 x 16 pixels with a two-pixel apron in LDS)
Yardsticks on the same frame, from the same build (this change touches neither kernel): decode12_float followed by
apply_white_balance (two launches, float32), and the fused decode + gain kernel of RCD.process_packed, taken from the library's
per-kernel event timer while the RCD call runs.  Device time per call between two HIP events on one stream around a batch of
back-to-back calls, after warm-up calls of the same shape; three batches per figure, the fastest is reported and all are listed.
GB/s is on the algorithmic bytes: 1.5 B per pixel in, 4 or 2 out.

  python3 profiles/rawprepare_bench.py [--size 4096x3072] [--warmup 5] [--iters 50]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', default='4096x3072')
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=50)
    a = ap.parse_args()
    assert a.warmup >= 5 and a.iters >= 50
    w, h = map(int, a.size.split('x'))
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(7)
    codes = torch.from_numpy(rng.integers(256, 4096, (h, w)).astype(np.uint16)).to(dev)
    data = td.encode12_u16(codes.view(-1))
    pattern, fmt = td.BayerPattern.RGGB, td.PackedFormat.Packed12
    gains = torch.tensor([1.9, 1.0, 1.6], device=dev)
    y, x = np.meshgrid(np.linspace(-1, 1, 25), np.linspace(-1, 1, 33), indexing='ij')
    grid = torch.from_numpy((1.0 + 0.6 * (x * x + y * y))[:, :, None].repeat(4, axis=2).astype(np.float32))
    configs = {
        'identity': (td.RawPrepare(dev, (w, h), pattern, clip=False), None),
        'no_defects': (td.RawPrepare(dev, (w, h), pattern, black=256.0, shading=grid), gains),
        'full': (td.RawPrepare(dev, (w, h), pattern, black=256.0, shading=grid, hot=True, dead=True), gains),
    }
    assert torch.equal(configs['identity'][0].process_packed(data, fmt), td.decode12_float(data).view(h, w))

    chain_us, chain_batches = device_us(lambda: td.apply_white_balance(td.decode12_float(data).view(h, w), gains, pattern), a.warmup, a.iters)
    decode_us, decode_batches = device_us(lambda: td.decode12_float(data), a.warmup, a.iters)
    rcd = td.RCD(dev, (w, h), pattern)
    for _ in range(a.warmup):
        rcd.process_packed(data, gains, fmt)
    torch.cuda.synchronize()
    _native.profile_enable(True, 'tdk_decode12_wb')
    for _ in range(a.iters):
        rcd.process_packed(data, gains, fmt)
    torch.cuda.synchronize()
    launches, ms = _native.profile_report()['tdk_decode12_wb']
    _native.profile_enable(False)
    fused_us = ms * 1e3 / launches
    base = {'size': [w, h], 'decode12_float_plus_apply_white_balance_us': round(chain_us, 1), 'chain_us_batches': chain_batches,
            'decode12_float_us': round(decode_us, 1), 'decode12_float_us_batches': decode_batches,
            'fused_decode_gain_kernel_us': round(fused_us, 1), 'fused_launches': launches}
    print(json.dumps(base), flush=True)

    rows = []
    for out_dtype in (torch.float32, torch.float16):
        for name, (rp, wb) in configs.items():
            us, batches = device_us(lambda: rp.process_packed(data, fmt, white_balance=wb, out_dtype=out_dtype), a.warmup, a.iters)
            nbytes = w * h * 3 // 2 + w * h * (4 if out_dtype == torch.float32 else 2)
            row = {'config': name, 'out_dtype': str(out_dtype).split('.')[1], 'us': round(us, 1), 'us_batches': batches,
                   'GB_per_s': round(nbytes / us * 1e-3, 1), 'algorithmic_bytes': nbytes, 'lds_bytes': rp.lds_bytes(),
                   'over_two_kernel_chain': round(us / chain_us, 2), 'over_fused_decode_gain_kernel': round(us / fused_us, 2)}
            rows.append(row)
            print(json.dumps(row), flush=True)
    print(json.dumps({'warmup': a.warmup, 'iters': a.iters, **base, 'rows': rows}))


if __name__ == '__main__':
    main()
