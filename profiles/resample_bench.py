"""Resize.process (csrc/resample.hip) against what a user would otherwise call on the same device: torch's antialiased bilinear
interpolate, with the HWC <-> CHW permutes it needs and, for uint8, the float round trip (to float32, clamp, round, back).

4096 x 3072 x 3 -> 1024 x 768 and -> 256 x 192, uint8 and float16.  Device time per call between two HIP events around a batch of
back-to-back calls, after warm-up calls of the same shape; three batches per figure, the fastest is reported and all three are
listed.  GB/s is on the algorithmic bytes: the source read once plus the destination written once.

  python3 profiles/resample_bench.py [--size 4096x3072] [--warmup 5] [--iters 50]
"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / 'torch-darktable_amd'))
import torch_darktable as td  # noqa: E402


def torch_antialiased(x, out_h, out_w):
    """(H, W, C) -> (out_h, out_w, C) in x's dtype through torch.nn.functional.interpolate(antialias=True)."""
    chw = x.permute(2, 0, 1).unsqueeze(0)
    if x.dtype == torch.uint8:
        chw = chw.float()
    y = torch.nn.functional.interpolate(chw, size=(out_h, out_w), mode='bilinear', antialias=True, align_corners=False)
    if x.dtype == torch.uint8:
        y = y.clamp_(0, 255).round_().to(torch.uint8)
    return y.squeeze(0).permute(1, 2, 0).contiguous()


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
    torch.manual_seed(7)
    base = torch.rand(h, w, 3, device=dev)
    rows = []
    for dtype in (torch.uint8, torch.float16):
        x = (base * 255).to(torch.uint8) if dtype == torch.uint8 else base.to(dtype)
        for ow, oh in ((w // 4, h // 4), (w // 16, h // 16)):
            rs = td.Resize(dev, (w, h), (ow, oh))
            mine, theirs = rs.process(x), torch_antialiased(x, oh, ow)
            diff = (mine.float() - theirs.float()).abs().max().item()
            us, batches = device_us(lambda: rs.process(x), a.warmup, a.iters)
            ref_us, ref_batches = device_us(lambda: torch_antialiased(x, oh, ow), a.warmup, a.iters)
            nbytes = (w * h + ow * oh) * 3 * x.element_size()
            row = {'src': [w, h], 'dst': [ow, oh], 'dtype': str(dtype).split('.')[1], 'resize_us': round(us, 1), 'resize_us_batches': batches,
                   'torch_us': round(ref_us, 1), 'torch_us_batches': ref_batches, 'torch_over_resize': round(ref_us / us, 2),
                   'algorithmic_bytes': nbytes, 'resize_GB_per_s': round(nbytes / us * 1e-3, 1), 'lds_bytes': rs.lds_bytes(3, dtype),
                   'max_abs_diff_to_torch': diff, 'slower_than_torch': bool(us > ref_us)}
            rows.append(row)
            print(json.dumps(row), flush=True)
    print(json.dumps({'warmup': a.warmup, 'iters': a.iters, 'rows': rows}))


if __name__ == '__main__':
    main()
