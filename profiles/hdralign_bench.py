"""MotionHdrMerge (csrc/hdralign.hip, and tdk_motion_match of csrc/motion.hip) at 12 MP, launch by launch, next to HdrMerge.process.

Frames: the brackets of profiles/hdrmerge_bench.py -- F = 3 (1, 1/4, 1/16) and F = 5 (1 .. 1/16 in stops) 4096 x 3072 mosaics (RGGB) of
a ramp of 0.01 .. 4 in units where the longest frame saturates at 1, with Poisson-Gaussian noise -- float32 in and out and binary16 in
and out, radius 2.  Per configuration, in one process:
  tdk_hdralign_pyramid of one frame, and tdk_motion_pyramid of the same frame beside it;
  tdk_motion_match of one frame against the anchor frame;
  tdk_hdr_merge (HdrMerge.process), tdk_hdralign_merge with a zero field and with a panned field (frame f displaced by (-4 f, 6 f - 2 f % 4));
  the whole MotionHdrMerge.process: F pyramids, F - 1 matches, one merge.
Device time per call between two HIP events on one stream around a batch of back-to-back calls, after warm-up calls of the same shape;
five batches per figure, the MEDIAN is reported and all are listed.  One process; run it under a time limit:

  timeout -k 10 600 python3 profiles/hdralign_bench.py [--warmup 5] [--iters 20] [--out profiles/r26/hdralign_bench.txt]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'r26' / 'hdralign_bench.txt'))
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
    plain = td.HdrMerge(dev, (w, h), td.BayerPattern.RGGB, model, radius=2, clip=CLIP)
    merge = td.MotionHdrMerge(dev, (w, h), td.BayerPattern.RGGB, model, radius=2, clip=CLIP)
    me = merge.motion
    ty, tx = me.tiles
    for exposures in ((1.0, 0.25, 1 / 16), (1.0, 0.5, 0.25, 0.125, 1 / 16)):
        nf = len(exposures)
        frames32 = []
        for e in exposures:
            clean = scene * e
            frames32.append(torch.clamp(clean + torch.randn((h, w), device=dev, generator=g) * torch.sqrt(A_NOISE * clean + B_NOISE), max=1.0))
        zero = torch.zeros((nf, ty, tx, 2), dtype=torch.int16, device=dev)
        panned = zero.clone()
        for f in range(nf):
            panned[f, :, :, 0], panned[f, :, :, 1] = -4 * f, 6 * f - 2 * (f % 4)
        exp = torch.tensor(exposures, dtype=torch.float32, device=dev)
        for name, dtype, size in (('float32', torch.float32, 4), ('float16', torch.float16, 2)):
            frames = [x.to(dtype) for x in frames32]
            head = {'frames': nf, 'storage': f'{name} in and out', 'size': [w, h]}
            merge.prepare(nf)
            merge.align(frames, exp, ref=0)
            pyramids, fields, costs = merge._workspace(nf, dev)
            rows = {}

            def time(op, fn, **more):
                us, batches = device_us(fn, a.warmup, a.iters)
                rows[op] = us
                emit({**head, 'op': op, 'us': round(us, 1), 'us_batches': batches, **more})

            time('tdk_hdralign_pyramid, one frame', lambda: td._native.check(td._native.lib.tdk_hdralign_pyramid(
                frames[1].data_ptr(), td._native.TDK_F32 if dtype == torch.float32 else td._native.TDK_F16, w, h, me.scale, me.levels, pyramids[0].data_ptr(), 1,
                exp.data_ptr(), nf, 1, torch.cuda.current_stream().cuda_stream)))
            time('tdk_motion_pyramid, one frame', lambda: me.build_pyramid(frames[1], pyramids[0], 1))
            time('tdk_motion_match, one frame against the anchor', lambda: me.match(pyramids[0], 0, pyramids[0], 1, fields[1], costs[1]))
            time('tdk_hdr_merge (HdrMerge.process) radius=2', lambda: plain.process(frames, exp, ref=0), lds_bytes=plain.lds_bytes())
            base = rows['tdk_hdr_merge (HdrMerge.process) radius=2']
            for label, field in (('a zero field', zero), ('a panned field', panned)):
                op = f'tdk_hdralign_merge with {label} radius=2'
                us, batches = device_us(lambda: merge.process(frames, exp, ref=0, fields=field), a.warmup, a.iters)
                rows[op] = us
                emit({**head, 'op': op, 'us': round(us, 1), 'us_batches': batches, 'times_the_plain_merge': round(us / base, 3), 'lds_bytes': merge.lds_bytes()})
            us, batches = device_us(lambda: merge.process(frames, exp, ref=0), a.warmup, a.iters)
            parts = nf * rows['tdk_hdralign_pyramid, one frame'] + (nf - 1) * rows['tdk_motion_match, one frame against the anchor']
            emit({**head, 'op': f'MotionHdrMerge.process: {nf} pyramids, {nf - 1} matches, one merge', 'us': round(us, 1), 'us_batches': batches,
                  'times_the_plain_merge': round(us / base, 2), 'us_pyramids_and_matches_by_the_rows_above': round(parts, 1),
                  'share_of_the_matches': round((nf - 1) * rows['tdk_motion_match, one frame against the anchor'] / us, 3)})
            del frames
            torch.cuda.empty_cache()
    out_path = Path(a.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text('\n'.join([f'# profiles/hdralign_bench.py --warmup {a.warmup} --iters {a.iters} on {torch.cuda.get_device_name(0)}', *lines]) + '\n')


if __name__ == '__main__':
    main()
