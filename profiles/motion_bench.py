"""MotionTemporalDenoise.process (csrc/motion.hip) at 12 MP, launch by launch, next to the plain TemporalDenoise.process and a device copy
timed in the same sitting.

Frames: a 4096 x 3072 mosaic (RGGB), a textured scene (smoothed noise, structure in both directions) panned by (2, -4) sites per frame,
with Poisson-Gaussian noise, a ring of four frames.  Radius 2; float32 throughout (source, state, output) and binary16 throughout.
Figures per configuration:
  the device time of the pyramid launch and of the match launch, each in a batch of back-to-back calls of that entry point alone;
  the compensated filter (tdk_motion_temporal_denoise: filter and advance) under a zero field and under a uniform field of (2, -4);
  the whole MotionTemporalDenoise.process (four launches), and what displacement the estimator found;
  TemporalDenoise.process on the same frames, and a device-to-device copy of the bytes the pyramid launch reads (the mosaic).
Device time per call between two HIP events on one stream around a batch of back-to-back calls, after warm-up calls of the same shape;
five batches per figure, the MEDIAN is reported and all are listed.  One process; run it under a time limit:

  timeout -k 10 600 python3 profiles/motion_bench.py [--warmup 5] [--iters 20] [--out profiles/r18/motion_bench.txt]
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
from torch_darktable._native import TDK_F16, TDK_F32, check, lib  # noqa: E402
from torch_darktable.torch_darktable_extension import _pattern, _ptr, _stream  # noqa: E402

A_NOISE, B_NOISE = 3e-4, 2e-6
STEP = (2, -4)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'r18' / 'motion_bench.txt'))
    a = ap.parse_args()
    assert a.warmup >= 5 and a.iters >= 20
    dev = torch.device('cuda', 0)
    w, h, pad, radius = 4096, 3072, 16, 2
    lines = []

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    g = torch.Generator(device=dev).manual_seed(17)
    base = torch.rand((1, 1, h + 2 * pad + 8, w + 2 * pad + 8), device=dev, generator=g)
    scene = torch.nn.functional.avg_pool2d(base, 9, stride=1)[0, 0]
    scene = 0.05 + 0.85 * (scene - scene.min()) / (scene.max() - scene.min())
    ring32 = []
    for f in range(4):   # frame f + 1 sees the scene STEP further: the ring pans forward three times and jumps back once
        clean = scene[pad + f * STEP[0]:pad + f * STEP[0] + h, pad + f * STEP[1] + 16:pad + f * STEP[1] + 16 + w]
        ring32.append((clean + torch.randn((h, w), device=dev, generator=g) * torch.sqrt(A_NOISE * clean + B_NOISE)).contiguous())
    del base, scene
    model = td.NoiseModel.from_values(A_NOISE, B_NOISE, dev)
    for name, dtype, tag in (('float32', torch.float32, TDK_F32), ('float16', torch.float16, TDK_F16)):
        ring = [x.to(dtype) for x in ring32]
        head = {'frame': f'mosaic {name} throughout', 'size': [w, h], 'radius': radius}
        me = td.MotionEstimate(dev, (w, h))
        mt = td.MotionTemporalDenoise(dev, (w, h), td.BayerPattern.RGGB, model, motion=me, radius=radius, state_dtype=dtype)
        plain = td.TemporalDenoise(dev, (w, h), td.BayerPattern.RGGB, model, radius=radius, state_dtype=dtype)
        step = [0]

        def frame():
            step[0] += 1
            return ring[step[0] & 3]

        src_bytes = ring[0].numel() * ring[0].element_size()
        copy_us, batches = device_us(lambda: ring[0].clone(), a.warmup, a.iters)
        emit({**head, 'op': 'device copy of the mosaic (the bytes the pyramid launch reads)', 'us': round(copy_us, 1), 'us_batches': batches,
              'GB_per_s': round(2 * src_bytes / copy_us * 1e-3, 1)})
        pyramid = me.new_pyramid(dev)
        field, costs = me.new_field(dev)
        us, batches = device_us(lambda: me.build_pyramid(frame(), pyramid, step[0] & 1), a.warmup, a.iters)
        emit({**head, 'op': 'tdk_motion_pyramid', 'us': round(us, 1), 'us_batches': batches, 'times_the_copy': round(us / copy_us, 2), 'pyramid_bytes': me.pyramid_bytes()})
        me.build_pyramid(ring[1], pyramid, 0)
        me.build_pyramid(ring[0], pyramid, 1)
        us, batches = device_us(lambda: me.match(pyramid, 0, pyramid, 1, field, costs), a.warmup, a.iters)
        torch.cuda.synchronize()
        found = float((field.cpu() == torch.tensor(STEP, dtype=torch.int16)).all(-1).float().mean())
        emit({**head, 'op': 'tdk_motion_match (levels 3, search 4)', 'us': round(us, 1), 'us_batches': batches, 'tiles': list(me.tiles), 'tiles_with_the_pan': round(found, 4)})

        state = mt._states[None]
        for what, value in (('zero field', (0, 0)), (f'uniform field {STEP}', STEP)):
            given = torch.tensor(value, dtype=torch.int16, device=dev).repeat(*me.tiles, 1).contiguous()
            out = torch.empty((h, w), dtype=dtype, device=dev)

            def filter_call():
                check(lib.tdk_motion_temporal_denoise(_ptr(frame()), tag, _ptr(out), tag, _ptr(state), tag, w, h, _pattern(td.BayerPattern.RGGB), _ptr(model.model), None,
                                                      radius, 1.5, 3.0, 16.0, 8.0, 1e-12, _ptr(given), _stream()))

            us, batches = device_us(filter_call, a.warmup, a.iters)
            emit({**head, 'op': f'tdk_motion_temporal_denoise, {what}', 'us': round(us, 1), 'us_batches': batches})
        mt.reset()
        us_plain, batches = device_us(lambda: plain.process(frame()), a.warmup, a.iters)
        emit({**head, 'op': 'TemporalDenoise.process', 'us': round(us_plain, 1), 'us_batches': batches, 'sites_with_history': round(float((plain.state()[1] > 1).float().mean()), 4)})
        us, batches = device_us(lambda: mt.process(frame()), a.warmup, a.iters)
        torch.cuda.synchronize()
        found = float((mt.field().cpu() == torch.tensor(STEP, dtype=torch.int16)).all(-1).float().mean())
        emit({**head, 'op': 'MotionTemporalDenoise.process (pyramid, match, filter, advance)', 'us': round(us, 1), 'us_batches': batches,
              'times_the_plain_filter': round(us / us_plain, 2), 'tiles_with_the_pan': round(found, 4),
              'sites_with_history': round(float((mt.state()[1] > 1).float().mean()), 4)})
        del mt, plain, pyramid, ring
        torch.cuda.empty_cache()
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text('\n'.join([f'# profiles/motion_bench.py --warmup {a.warmup} --iters {a.iters} on {torch.cuda.get_device_name(0)}', *lines]) + '\n')


if __name__ == '__main__':
    main()
