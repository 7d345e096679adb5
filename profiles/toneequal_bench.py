"""ToneEqualizer.process (csrc/toneequal.hip) at 12 MP against a device copy of the same bytes and against the same arithmetic
composed from torch operations.

4096 x 3072 frames of float32 and float16, cell 8 and 16, radius 4, a 3 EV shadow lift.  On the same frames, in the same process:
  * copy: out.copy_(x), the frame in and the frame out once -- the stage reads the frame twice and writes it once, so 1.5 x the
    copy's bytes is what it has to move;
  * torch: luminance, avg_pool2d to the cells, the two box passes as avg_pool2d over a replicate-padded grid, F.interpolate back to
    the pixels, the gain as exp2 of the curve's Gaussians at log2 of the mask (no table), the product -- float32 throughout, close
    to the stage's result but not its bits.
Device time per call between two HIP events on one stream around a batch of back-to-back calls, after warm-up calls of the same
shape; three batches per figure, the fastest is reported and all are listed.  The time of each launch comes from the library's own
event timer in a pass of its own (profile_enable).

  python3 profiles/toneequal_bench.py [--warmup 5] [--iters 20] [--out profiles/r22/toneequal_bench.txt]

On a shared machine run it with a time limit of its own, e.g.  timeout -k 10 300 python3 profiles/toneequal_bench.py && next step.
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

GAINS = (3, 3, 3, 2.5, 2, 1.5, 1, 0.5, 0)


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


def torch_composition(te):
    """The stage from torch operations, float32 arithmetic: a callable frame -> frame."""
    dev = te.table.device
    s, r, eps = te.cell, te.radius, te.eps
    weights = torch.tensor(te.weights, device=dev)
    w = torch.from_numpy(td.ToneEqualizer.curve(te.gains_ev, te.sigma)).to(dev, torch.float32)
    centres = torch.arange(-8.0, 1.0, device=dev)

    def box(p):   # (1, 1, CH, CW) -> the window mean with the grid's edge replicated
        return F.avg_pool2d(F.pad(p, (r, r, r, r), mode='replicate'), 2 * r + 1, stride=1)

    def run(x):
        h, wd, _ = x.shape
        xf = x.float()
        lum = (xf * weights).sum(-1).clamp_min(0)
        pad = F.pad(lum[None, None], (0, -wd % s, 0, -h % s), mode='replicate')
        cells = F.avg_pool2d(pad, s)
        mean, corr = box(cells), box(cells * cells)
        var = (corr - mean * mean).clamp_min(0)
        a = var / (var + eps)
        b = mean - a * mean
        up = F.interpolate(torch.cat((box(a), box(b)), 1), scale_factor=s, mode='bilinear', align_corners=False)[0, :, :h, :wd]
        m = (up[0] * lum + up[1]).clamp(2.0 ** -16, 16.0)
        ev = (torch.log2(m) + te.mask_exposure).clamp(-8.0, 0.0)
        gain = torch.exp2((w * torch.exp(-(ev[..., None] - centres) ** 2 / (2.0 * te.sigma ** 2))).sum(-1))
        return (xf * gain[..., None]).to(x.dtype)

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--size', type=int, nargs=2, default=(4096, 3072), metavar=('W', 'H'))
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'r22' / 'toneequal_bench.txt'))
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
    base = np.exp2(rng.uniform(-9.0, 0.0, (h // 64 + 1, w // 64 + 1, 1))).repeat(64, 0).repeat(64, 1)[:h, :w]
    frame = torch.from_numpy((base * rng.uniform(0.7, 1.3, (h, w, 3))).astype(np.float32)).to(dev)
    for dtype in (torch.float32, torch.float16):
        x = frame.to(dtype)
        esz = x.element_size()
        out = torch.empty_like(x)
        copy_bytes = 2 * x.numel() * esz
        copy_us, copy_batches = device_us(lambda: out.copy_(x), a.warmup, a.iters)
        emit({'size': [w, h], 'dtype': str(dtype), 'op': 'copy (frame in, frame out)', 'us': round(copy_us, 1), 'us_batches': copy_batches, 'bytes': copy_bytes,
              'GB_per_s': round(copy_bytes / copy_us * 1e-3, 1)})
        for cell in (8, 16):
            te = td.ToneEqualizer(dev, (w, h), gains_ev=GAINS, cell=cell, radius=4)
            us, batches = device_us(lambda: te.process(x), a.warmup, a.iters)
            _native.profile_enable(True, 'tdk_toneeq(')
            for _ in range(a.iters):
                te.process(x)
            torch.cuda.synchronize()
            report = _native.profile_report()
            _native.profile_enable(False)
            per_launch = {name: round(ms * 1e3 / n, 1) for name, (n, ms) in sorted(report.items())}
            cells = -(-w // cell) * -(-h // cell)
            nbytes = 3 * x.numel() * esz + 4 * cells * (1 + 1 + 2 + 2)   # the frame read twice and written once; L written and read, a and b written and read
            compose = torch_composition(te)
            torch_us, torch_batches = device_us(lambda: compose(x), a.warmup, a.iters)
            got, ref = te.process(x).float(), compose(x).float()
            rel = ((got - ref).abs() / ref.abs().clamp_min(1e-6)).max().item()
            emit({'size': [w, h], 'dtype': str(dtype), 'op': f'ToneEqualizer.process cell={cell} radius=4', 'us': round(us, 1), 'us_batches': batches,
                  'spec_bytes': nbytes, 'GB_per_s': round(nbytes / us * 1e-3, 1), 'us_per_launch': per_launch, 'sum_of_launches_us': round(sum(per_launch.values()), 1),
                  'over_copy': round(us / copy_us, 2), 'torch_us': round(torch_us, 1), 'torch_us_batches': torch_batches, 'torch_over_stage': round(torch_us / us, 1),
                  'max_rel_difference_to_torch': float(f'{rel:.3g}'), 'workspace_bytes': te.workspace_bytes(), 'lds_bytes': te.lds_bytes(dtype)})
            del te, compose, got, ref
        del x, out
        torch.cuda.empty_cache()
    path = Path(a.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text('\n'.join([f'# profiles/toneequal_bench.py --warmup {a.warmup} --iters {a.iters} on {torch.cuda.get_device_name(0)}', *lines]) + '\n')


if __name__ == '__main__':
    main()
