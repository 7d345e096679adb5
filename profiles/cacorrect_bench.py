"""ChromaticAberration.correct and .estimate (csrc/cacorrect.hip) at 12 MP next to yardsticks that are not the code under test.

Frame: a 4096 x 3072 mosaic (RGGB), smooth texture with noise, red and blue magnified by 1.0008 and 0.9994 (2.0 and 1.5 sites at the
corner).  `correct`: float32 in and out and binary16 in and out, bilinear and bicubic, with a model of that size.  Beside it, in the same
process:
  a device-to-device copy of the bytes the stage must move, one plane in and one out -- timed as a copy of one plane, which reads and
    writes each byte once;
  the torch composition a user would write today: the red and the blue plane taken out of the mosaic, grid_sample on each with a
    sampling grid that was computed beforehand (not timed), and written back into a copy of the mosaic; float32.
`estimate`: one frame and three frames, float32, with a noise model, fit='poly3', blocks of 64; the device time of the gather launches
and of the finishing launch come from the library's per-kernel event timer (tdk_profile_*), in a pass of its own; beside it the copy of
one frame.
Device time per call between two HIP events on one stream around a batch of back-to-back calls, after warm-up calls of the same shape;
five batches per figure, the MEDIAN is reported and all are listed.  One process; run it under a time limit:

  timeout -k 10 600 python3 profiles/cacorrect_bench.py [--warmup 5] [--iters 20] [--out profiles/r20/cacorrect_bench.txt]
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


class TorchCorrect:
    """Four planes and grid_sample: the model's coordinates per plane, normalised for align_corners=True, computed once."""

    def __init__(self, w, h, red, blue, mode, dev):
        self.mode = mode
        self.grids = []
        x0, y0 = (w - 1) / 2, (h - 1) / 2
        for s, (oy, ox) in ((red, (0, 0)), (blue, (1, 1))):
            j, i = torch.arange(ox, w, 2, device=dev, dtype=torch.float32), torch.arange(oy, h, 2, device=dev, dtype=torch.float32)
            qx, qy = x0 + (j - x0) * s, y0 + (i - y0) * s                 # site coordinates in the captured plane
            u, v = (qx - ox) / 2, (qy - oy) / 2                           # plane samples
            gx, gy = u / (w // 2 - 1) * 2 - 1, v / (h // 2 - 1) * 2 - 1
            self.grids.append(((oy, ox), torch.stack(torch.broadcast_tensors(gx[None, :], gy[:, None]), dim=-1)[None].contiguous()))

    def process(self, x):
        out = x.clone()
        for (oy, ox), grid in self.grids:
            plane = x[oy::2, ox::2][None, None]
            out[oy::2, ox::2] = torch.nn.functional.grid_sample(plane, grid, mode=self.mode, padding_mode='border', align_corners=True)[0, 0]
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'r20' / 'cacorrect_bench.txt'))
    a = ap.parse_args()
    assert a.warmup >= 5 and a.iters >= 20
    dev = torch.device('cuda', 0)
    w, h = 4096, 3072
    red, blue = 1.0008, 0.9994
    lines = []

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    g = torch.Generator(device=dev).manual_seed(20)
    yy, xx = torch.arange(h, device=dev, dtype=torch.float32)[:, None], torch.arange(w, device=dev, dtype=torch.float32)[None, :]
    x0, y0 = (w - 1) / 2, (h - 1) / 2
    scene = lambda x, y: 0.4 + 0.15 * torch.sin(0.19 * x + 0.07 * y) + 0.12 * torch.sin(0.05 * x - 0.23 * y) + 0.08 * torch.sin(0.31 * x + 0.29 * y)
    mosaic = scene(xx, yy).clone()
    mosaic[0::2, 0::2] = 0.5 * scene(x0 + (xx[:, 0::2] - x0) / red, y0 + (yy[0::2] - y0) / red)
    mosaic[1::2, 1::2] = 0.7 * scene(x0 + (xx[:, 1::2] - x0) / blue, y0 + (yy[1::2] - y0) / blue)
    noise_a, noise_b = 2e-5, 2e-6
    mosaic = mosaic + torch.randn((h, w), device=dev, generator=g) * torch.sqrt(noise_a * mosaic + noise_b)
    noise = td.NoiseModel.from_values(noise_a, noise_b, dev)

    # ---- correct
    for name, dtype, size in (('float32', torch.float32, 4), ('float16', torch.float16, 2)):
        x = mosaic.to(dtype)
        moved = 2 * w * h * size
        head = {'storage': f'{name} in and out', 'size': [w, h], 'bytes_moved': moved}
        plane = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
        copy_us, batches = device_us(lambda: plane.clone(), a.warmup, a.iters)
        emit({**head, 'op': 'device copy of the same number of bytes (read one plane, write one)', 'us': round(copy_us, 1), 'us_batches': batches,
              'GB_per_s': round(moved / copy_us * 1e-3, 1)})
        del plane
        for interp in ('bilinear', 'bicubic'):
            ca = td.ChromaticAberration.from_coefficients(dev, (w, h), td.BayerPattern.RGGB, red=(red, 0, 0), blue=(blue, 0, 0), interp=interp)
            us, batches = device_us(lambda: ca.correct(x), a.warmup, a.iters)
            out = ca.correct(x)
            row = {**head, 'op': f'ChromaticAberration.correct {interp}', 'us': round(us, 1), 'us_batches': batches, 'GB_per_s': round(moved / us * 1e-3, 1),
                   'times_the_copy': round(us / copy_us, 2), 'lds_bytes': ca.lds_bytes(dtype)}
            emit(row)
            if name == 'float32':
                ref = TorchCorrect(w, h, red, blue, interp, dev)
                us_t, batches = device_us(lambda: ref.process(x), a.warmup, a.iters)
                err = float((ref.process(x) - out).abs().max())
                emit({**head, 'op': f'torch operations: four planes and grid_sample {interp}', 'us': round(us_t, 1), 'us_batches': batches,
                      'times_the_kernel': round(us_t / us, 1), 'max_abs_difference_to_the_kernel': err})
        del x
        torch.cuda.empty_cache()

    # ---- estimate
    ca = td.ChromaticAberration(dev, (w, h), td.BayerPattern.RGGB)
    frame_copy_us, batches = device_us(lambda: mosaic.clone(), a.warmup, a.iters)
    emit({'op': 'device copy of one float32 frame', 'size': [w, h], 'us': round(frame_copy_us, 1), 'us_batches': batches})
    for nf in (1, 3):
        frames = [mosaic] + [mosaic + 0.001 * torch.randn((h, w), device=dev, generator=g) for _ in range(nf - 1)]
        run = lambda: ca.estimate(frames, noise_model=noise, fit='poly3')
        us, batches = device_us(run, a.warmup, a.iters)
        fitted = run()
        rows = fitted.model.cpu().tolist()
        corner = [ca.rn * ((r[0] - 1) + r[1] + r[2]) for r in rows]
        _native.profile_enable(True, 'tdk_ca')
        for _ in range(a.iters):
            run()
        torch.cuda.synchronize()
        report = _native.profile_report()
        _native.profile_enable(False)
        gather_us = report['tdk_ca_gather'][1] * 1e3 / report['tdk_ca_gather'][0]
        finish_us = report['tdk_ca_finish'][1] * 1e3 / report['tdk_ca_finish'][0]
        emit({'op': "ChromaticAberration.estimate fit='poly3' block=64 with a noise model", 'frames': nf, 'size': [w, h], 'us': round(us, 1), 'us_batches': batches,
              'gather_launch_us_each': round(gather_us, 1), 'finishing_launch_us': round(finish_us, 1), 'gather_times_the_frame_copy': round(gather_us / frame_copy_us, 2),
              'blocks': (w // 64) * (h // 64), 'corner_shift_true': [round(ca.rn * (red - 1), 3), round(ca.rn * (blue - 1), 3)],
              'corner_shift_estimated': [round(c, 3) for c in corner], 'valid': [r[3] for r in rows]})
    out_path = Path(a.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text('\n'.join([f'# profiles/cacorrect_bench.py --warmup {a.warmup} --iters {a.iters} on {torch.cuda.get_device_name(0)}', *lines]) + '\n')


if __name__ == '__main__':
    main()
