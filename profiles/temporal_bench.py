"""TemporalDenoise.process (csrc/temporal.hip) at 12 MP next to two yardsticks that are not the code under test.

Frames: a 4096 x 3072 mosaic (RGGB), a ramp with Poisson-Gaussian noise, a new noise realisation per call out of a ring of four, so the
filter runs in its steady state (history kept at most sites).  Configurations: float32 throughout (source, state, output) and
binary16 throughout, radius 2 and 3.  Beside them, in the same process:
  a device-to-device copy of the bytes the filter must move: per site 10 in and 10 out at float32 (sample, average, count; average,
    count, output), 6 and 6 at binary16 -- timed as a copy of half that many bytes, which reads and writes each once;
  the same arithmetic composed from torch operations: two zero-padded box sums (avg_pool2d with divisor 1) and the elementwise rest,
    float32, out of place, the state held as two tensors.
Device time per call between two HIP events on one stream around a batch of back-to-back calls, after warm-up calls of the same shape;
five batches per figure, the MEDIAN is reported and all are listed.  The two launches of a call are timed one by one through the
library's event timer in a pass of their own.  One process; run it under a time limit:

  timeout -k 10 600 python3 profiles/temporal_bench.py [--warmup 5] [--iters 20] [--out profiles/r17/temporal_bench.txt]
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
from torch_darktable import _native  # noqa: E402

A_NOISE, B_NOISE = 3e-4, 2e-6


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


class TorchTemporal:
    """The header's arithmetic in torch operations on one colour-blind model row (a, b): what a user would write today."""

    def __init__(self, radius, t_lo=1.5, t_hi=3.0, pixel=4.0, n_max=8.0, v_min=1e-12):
        self.k, self.r = 2 * radius + 1, radius
        self.t_hi, self.inv, self.c2, self.n_max, self.v_min = t_hi, 1.0 / (t_hi - t_lo), pixel * pixel, n_max, v_min
        self.acc = self.cnt = None

    def box(self, p):
        return torch.nn.functional.avg_pool2d(p[None, None], self.k, stride=1, padding=self.r, divisor_override=1)[0, 0]

    def process(self, x):
        if self.acc is None:
            self.acc, self.cnt = x.clone(), torch.ones_like(x)
            return self.acc
        A, N = self.acc, self.cnt
        d = x - A
        var = torch.clamp(A_NOISE * torch.clamp(A, min=0.0) + B_NOISE, min=self.v_min)
        v = var + var / torch.clamp(N, min=1.0)
        e = d * d
        t = self.box(e) / self.box(v)
        s = torch.clamp((self.t_hi - t) * self.inv, 0.0, 1.0)
        s = torch.where(e > self.c2 * v, torch.zeros_like(s), s)
        n1 = torch.clamp(s * N + 1.0, max=self.n_max)
        self.acc, self.cnt = A + d / n1, n1
        return self.acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'r17' / 'temporal_bench.txt'))
    a = ap.parse_args()
    assert a.warmup >= 5 and a.iters >= 20
    dev = torch.device('cuda', 0)
    w, h = 4096, 3072
    lines = []

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    g = torch.Generator(device=dev).manual_seed(17)
    ramp = 0.03 + 0.9 * torch.linspace(0, 1, w, device=dev)[None, :] * torch.linspace(0.3, 1, h, device=dev)[:, None]
    ring32 = [ramp + torch.randn((h, w), device=dev, generator=g) * torch.sqrt(A_NOISE * ramp + B_NOISE) for _ in range(4)]
    model = td.NoiseModel.from_values(A_NOISE, B_NOISE, dev)
    for name, dtype, per_site in (('float32', torch.float32, 20), ('float16', torch.float16, 12)):
        ring = [x.to(dtype) for x in ring32]
        moved = w * h * per_site
        head = {'frame': f'mosaic {name} throughout', 'size': [w, h], 'bytes_moved': moved}
        half = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
        copy_us, batches = device_us(lambda: half.clone(), a.warmup, a.iters)
        emit({**head, 'op': 'device copy of the same number of bytes (read half, write half)', 'us': round(copy_us, 1), 'us_batches': batches,
              'GB_per_s': round(moved / copy_us * 1e-3, 1)})
        del half
        for radius in (2, 3):
            t = td.TemporalDenoise(dev, (w, h), td.BayerPattern.RGGB, model, radius=radius, state_dtype=dtype)
            step = [0]

            def call():
                step[0] += 1
                return t.process(ring[step[0] & 3])

            us, batches = device_us(call, a.warmup, a.iters)
            _native.profile_enable(True, 'tdk_temporal_denoise')
            for _ in range(a.iters):
                call()
            torch.cuda.synchronize()
            launches = {k: round(ms * 1e3 / n, 1) for k, (n, ms) in _native.profile_report().items()}
            _native.profile_enable(False)
            kept = float((t.state()[1] > 1).float().mean())
            emit({**head, 'op': f'TemporalDenoise.process radius={radius}', 'us': round(us, 1), 'us_batches': batches, 'GB_per_s': round(moved / us * 1e-3, 1),
                  'times_the_copy': round(us / copy_us, 2), 'launch_us': launches, 'lds_bytes': t.lds_bytes(), 'state_bytes': t.state_bytes(),
                  'sites_with_history': round(kept, 4)})
            del t
            if name == 'float32':
                ref = TorchTemporal(radius)
                step[0] = 0

                def torch_call():
                    step[0] += 1
                    return ref.process(ring[step[0] & 3])

                us, batches = device_us(torch_call, a.warmup, a.iters)
                emit({**head, 'op': f'torch operations: the same arithmetic, radius={radius}', 'us': round(us, 1), 'us_batches': batches})
                del ref
            torch.cuda.empty_cache()
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text('\n'.join([f'# profiles/temporal_bench.py --warmup {a.warmup} --iters {a.iters} on {torch.cuda.get_device_name(0)}', *lines]) + '\n')


if __name__ == '__main__':
    main()
