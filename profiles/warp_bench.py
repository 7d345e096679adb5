"""Warp.process (csrc/warp.hip) at 12 MP, staged against direct sampling, against what a user has to do today on the same device:
torch.nn.functional.grid_sample with a precomputed (H, W, 2) float32 grid.

4096 x 3072 x 3 undistortion (f = 2950, k1 = -0.12, k2 = 0.09, p1 = 8e-4, p2 = -5e-4, k3 = -0.02) to the same size; float16 and
uint8, bilinear and bicubic, flags 0 and TDK_WARP_DIRECT.  grid_sample is timed twice: on an NCHW tensor of its compute type that
already exists ("bare"; float32 for uint8 frames), and with the NHWC <-> NCHW permutes and, for uint8, the float round trip a
caller with interleaved frames pays ("with layout").  Device time per call between two HIP events around a batch of back-to-back
calls, after warm-up calls of the same shape; three batches per figure, the fastest is reported and all three are listed.  GB/s
is on the algorithmic bytes: the source read once plus the destination written once (grid_sample: plus its grid).

  python3 profiles/warp_bench.py [--size 4096x3072] [--warmup 5] [--iters 50]
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


def with_layout(x, grid, mode):
    """(H, W, C) in x's dtype -> the same, through grid_sample."""
    chw = x.permute(2, 0, 1).unsqueeze(0)
    if x.dtype == torch.uint8:
        chw = chw.float()
    y = torch.nn.functional.grid_sample(chw, grid.to(chw.dtype) if grid.dtype != chw.dtype else grid, mode=mode, padding_mode='zeros', align_corners=True)
    if x.dtype == torch.uint8:
        y = y.clamp_(0, 255).round_().to(torch.uint8)
    return y.squeeze(0).permute(1, 2, 0).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', default='4096x3072')
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=50)
    a = ap.parse_args()
    assert a.warmup >= 5 and a.iters >= 50
    w, h = map(int, a.size.split('x'))
    dev = torch.device('cuda', 0)
    torch.manual_seed(7)
    base = torch.rand(h, w, 3, device=dev)
    s = w / 4096.0
    K = np.array([[2950.0 * s, 0, 2040.3 * s], [0, 2946.0 * s, 1507.7 * s], [0, 0, 1]])
    dist = [-0.12, 0.09, 8e-4, -5e-4, -0.02]
    rows = []
    for dtype in (torch.float16, torch.uint8):
        x = (base * 255).to(torch.uint8) if dtype == torch.uint8 else base.to(dtype)
        for mode in ('bilinear', 'bicubic'):
            wp = td.Warp.undistort(dev, (w, h), K, dist, interpolation=mode)
            xy = wp.coordinates()
            compute = torch.float32 if dtype == torch.uint8 else dtype
            grid = torch.stack([2.0 * xy[..., 0] / (w - 1) - 1.0, 2.0 * xy[..., 1] / (h - 1) - 1.0], dim=-1).unsqueeze(0).to(compute).contiguous()
            chw = x.permute(2, 0, 1).unsqueeze(0).to(compute).contiguous()
            staged, direct = wp.process(x), wp.process(x, direct=True)
            same_bits = bool(torch.equal(staged, direct))
            diff = (staged.float() - with_layout(x, grid, mode).float()).abs().max().item()
            us, batches = device_us(lambda: wp.process(x), a.warmup, a.iters)
            direct_us, direct_batches = device_us(lambda: wp.process(x, direct=True), a.warmup, a.iters)
            bare_us, bare_batches = device_us(lambda: torch.nn.functional.grid_sample(chw, grid, mode=mode, padding_mode='zeros', align_corners=True),
                                              a.warmup, a.iters)
            layout_us, layout_batches = device_us(lambda: with_layout(x, grid, mode), a.warmup, a.iters)
            nbytes = 2 * w * h * 3 * x.element_size()
            grid_bytes = 2 * w * h * 3 * chw.element_size() + grid.numel() * grid.element_size()
            row = {'size': [w, h], 'dtype': str(dtype).split('.')[1], 'interpolation': mode,
                   'warp_us': round(us, 1), 'warp_us_batches': batches, 'warp_GB_per_s': round(nbytes / us * 1e-3, 1),
                   'warp_direct_us': round(direct_us, 1), 'warp_direct_us_batches': direct_batches, 'warp_direct_GB_per_s': round(nbytes / direct_us * 1e-3, 1),
                   'direct_over_staged': round(direct_us / us, 2), 'staged_equals_direct_bits': same_bits,
                   'grid_sample_bare_us': round(bare_us, 1), 'grid_sample_bare_us_batches': bare_batches,
                   'grid_sample_bare_GB_per_s': round(grid_bytes / bare_us * 1e-3, 1),
                   'grid_sample_with_layout_us': round(layout_us, 1), 'grid_sample_with_layout_us_batches': layout_batches,
                   'grid_sample_with_layout_over_warp': round(layout_us / us, 2), 'algorithmic_bytes': nbytes, 'grid_sample_bytes': grid_bytes,
                   'lds_bytes': wp.lds_bytes(3, dtype), 'max_abs_diff_to_grid_sample': diff}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del grid, chw
    print(json.dumps({'warmup': a.warmup, 'iters': a.iters, 'rows': rows}))


if __name__ == '__main__':
    main()
