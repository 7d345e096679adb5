"""HdrMerge.process (csrc/hdrmerge.hip) at 12 MP next to two yardsticks that are not the code under test.

Frames: a bracket of F = 3 (1, 1/4, 1/16) and F = 5 (1 .. 1/16 in stops) 4096 x 3072 mosaics (RGGB) of one scene, a ramp of 0.01 .. 4
in units where the longest frame saturates at 1 with Poisson-Gaussian noise, so that the longer frames clip in part of the frame and
every path of the kernel runs.  Configurations: float32 in and out, binary16 in and out, radius 2.  Beside them, in the same process:
  a device-to-device copy of the bytes the merge must move, F planes in and one out -- timed as a copy of half that many bytes, which
    reads and writes each once;
  the same arithmetic composed from torch operations: per frame a 3 x 3 max pool for the saturation, two zero-padded box sums
    (avg_pool2d with divisor 1) and the elementwise rest, float32, one colour-blind model row.
Device time per call between two HIP events on one stream around a batch of back-to-back calls, after warm-up calls of the same shape;
five batches per figure, the MEDIAN is reported and all are listed.  One process; run it under a time limit:

  timeout -k 10 600 python3 profiles/hdrmerge_bench.py [--warmup 5] [--iters 20] [--out profiles/r19/hdrmerge_bench.txt]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / 'torch-darktable_amd'))
import torch_darktable as td  # noqa: E402

A_NOISE, B_NOISE, CLIP = 3e-4, 2e-6, 0.95


def device_us(fn, warmup, iters, batches=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(batches):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1) * 1e3 / iters)
    return statistics.median(times), [round(t, 1) for t in times]


class TorchMerge:
    """The header's arithmetic in torch operations on one colour-blind model row (a, b): what a user would write today."""

    def __init__(self, exposures, radius=2, t_lo=1.5, t_hi=3.0, pixel=4.0, v_min=1e-12):
        e_min = min(exposures)
        self.k = [e / e_min for e in exposures]
        self.ref = max(range(len(exposures)), key=lambda f: exposures[f])
        self.size, self.r = 2 * radius + 1, radius
        self.t_hi, self.inv, self.c2, self.v_min = t_hi, 1.0 / (t_hi - t_lo), pixel * pixel, v_min

    def box(self, p):
        return torch.nn.functional.avg_pool2d(p[None, None], self.size, stride=1, padding=self.r, divisor_override=1)[0, 0]

    def u(self, Rp, k):
        return torch.clamp(A_NOISE * (Rp * k) + B_NOISE, min=self.v_min) / (k * k)

    def process(self, frames):
        nf = len(frames)
        sat = [torch.nn.functional.max_pool2d((~(x < CLIP)).float()[None, None], 3, stride=1, padding=1)[0, 0] > 0 for x in frames]
        best = torch.full_like(frames[0], -1.0)
        bk = torch.zeros_like(frames[0])
        for f in range(nf):
            take = ~sat[f] & ((best < 0) | (self.k[f] > bk))
            best = torch.where(take, float(f), best)
            bk = torch.where(take, self.k[f], bk)
        g = torch.where(~sat[self.ref], float(self.ref), best)
        blown = g < 0
        lo = min(range(nf), key=lambda f: self.k[f])
        g = torch.where(blown, float(lo), g).long()
        stack = torch.stack(frames)
        kg = torch.tensor(self.k, device=stack.device)[g]
        R = torch.gather(stack, 0, g[None])[0] / kg
        Rp = torch.clamp(R, min=0.0)
        ug = self.u(Rp, kg)
        num, den = torch.zeros_like(R), torch.zeros_like(R)
        for f in range(nf):
            r = frames[f] / self.k[f]
            u = self.u(Rp, self.k[f])
            d = r - R
            out_of_it = sat[f] | blown | (g == f)
            eps = torch.where(out_of_it, 0.0, d * d)
            v = torch.where(out_of_it, 0.0, u + ug)
            t = self.box(eps) / self.box(v)
            s = torch.nan_to_num(torch.clamp((self.t_hi - t) * self.inv, 0.0, 1.0), nan=0.0)
            s = torch.where(eps > self.c2 * v, 0.0, s)
            s = torch.where(g == f, 1.0, s)
            w = torch.where(sat[f], 0.0, s / u)
            num, den = num + w * torch.where(w > 0, r, 0.0), den + w
        return torch.where(den > 0, num / den, R)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'r19' / 'hdrmerge_bench.txt'))
    a = ap.parse_args()
    assert a.warmup >= 5 and a.iters >= 20
    dev = torch.device('cuda', 0)
    w, h = 4096, 3072
    lines = []

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    g = torch.Generator(device=dev).manual_seed(19)
    scene = torch.exp(torch.linspace(-4.6, 1.39, w, device=dev))[None, :] * torch.linspace(0.5, 1, h, device=dev)[:, None]
    model = td.NoiseModel.from_values(A_NOISE, B_NOISE, dev)
    merge = td.HdrMerge(dev, (w, h), td.BayerPattern.RGGB, model, radius=2, clip=CLIP)
    for exposures in ((1.0, 0.25, 1 / 16), (1.0, 0.5, 0.25, 0.125, 1 / 16)):
        nf = len(exposures)
        frames32 = []
        for e in exposures:
            clean = scene * e
            frames32.append(torch.clamp(clean + torch.randn((h, w), device=dev, generator=g) * torch.sqrt(A_NOISE * clean + B_NOISE), max=1.0))
        for name, dtype, size in (('float32', torch.float32, 4), ('float16', torch.float16, 2)):
            frames = [x.to(dtype) for x in frames32]
            moved = w * h * size * (nf + 1)
            head = {'frames': nf, 'storage': f'{name} in and out', 'size': [w, h], 'bytes_moved': moved}
            half = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
            copy_us, batches = device_us(lambda: half.clone(), a.warmup, a.iters)
            emit({**head, 'op': 'device copy of the same number of bytes (read half, write half)', 'us': round(copy_us, 1), 'us_batches': batches,
                  'GB_per_s': round(moved / copy_us * 1e-3, 1)})
            del half
            us, batches = device_us(lambda: merge.process(frames, exposures), a.warmup, a.iters)
            out, mask = merge.process(frames, exposures, return_mask=True)
            emit({**head, 'op': 'HdrMerge.process radius=2', 'us': round(us, 1), 'us_batches': batches, 'GB_per_s': round(moved / us * 1e-3, 1),
                  'times_the_copy': round(us / copy_us, 2), 'lds_bytes': merge.lds_bytes(),
                  'sites_anchored_on_the_longest': round(float(((mask & 7) == 0).float().mean()), 4),
                  'mean_frames_with_weight': round(float((mask >> 4).float().mean()), 3)})
            if name == 'float32':
                ref = TorchMerge(exposures)
                us_t, batches = device_us(lambda: ref.process(frames), a.warmup, a.iters)
                err = float((ref.process(frames) - out).abs().max())
                emit({**head, 'op': 'torch operations: the same arithmetic, radius=2', 'us': round(us_t, 1), 'us_batches': batches,
                      'times_the_kernel': round(us_t / us, 1), 'max_abs_difference_to_the_kernel': err})
            del frames
            torch.cuda.empty_cache()
    out_path = Path(a.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text('\n'.join([f'# profiles/hdrmerge_bench.py --warmup {a.warmup} --iters {a.iters} on {torch.cuda.get_device_name(0)}', *lines]) + '\n')


if __name__ == '__main__':
    main()
