"""NoiseProfile.estimate, NoiseModel.stabilize and NoiseModel.unstabilize (csrc/noiseprofile.hip) at 12 MP next to what a user would
write today.

Frames: a 4096 x 3072 mosaic (RGGB) as float32, float16 and uint16 for the estimate -- a ramp with Poisson-Gaussian noise -- and a
4096 x 3072 x 3 RGB frame as float32 and float16 for the transform.  Beside them, on the same frames in the same process:
  estimate_channel_noise on the RGB frame (the one number per channel the denoisers are given today);
  a torch composition of the same block statistics on the mosaic: the four CFA planes sliced, quantised, cut into 8 x 8 blocks with
    reshape (what unfold would give, without its copy), second differences, sum / min / max / energy per block -- no binning, no
    median, no fit: those would only add to it;
  the transform written with torch operations (mul, add, clamp, sqrt and their inverse), out of place;
  a device copy of the bytes each kernel reads, as the floor.
Device time per call between two HIP events on one stream around a batch of back-to-back calls, after warm-up calls of the same
shape; five batches per figure, the MEDIAN is reported and all are listed.  The three launches of an estimate are timed one by one
through the library's event timer in a pass of their own.  One process; run it under a time limit:

  timeout -k 10 600 python3 profiles/noiseprofile_bench.py [--warmup 5] [--iters 20] [--out profiles/r16/noiseprofile_bench.txt]
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


def torch_blocks(mosaic, scale):
    """S, qmin, qmax and E of every 8 x 8 block of the four CFA planes, with torch operations."""
    out = []
    for p in range(4):
        plane = mosaic[p >> 1::2, p & 1::2].float()
        q = torch.round(torch.clamp(plane * scale, 0.0, 65535.0)).to(torch.int64)
        nby, nbx = q.shape[0] // 8, q.shape[1] // 8
        b = q[:nby * 8, :nbx * 8].reshape(nby, 8, nbx, 8).permute(0, 2, 1, 3)
        h = 2 * b[..., 1:7] - b[..., 0:6] - b[..., 2:8]
        v = 2 * b[..., 1:7, :] - b[..., 0:6, :] - b[..., 2:8, :]
        out.append((b.sum((2, 3)), b.amin((2, 3)), b.amax((2, 3)), (h * h).sum((2, 3)) + (v * v).sum((2, 3))))
    return out


def torch_stabilize(x, a, c, k):
    return k * torch.sqrt(torch.clamp(a * x.float() + c, min=0.0))


def torch_unstabilize(y, a, coa):
    return (a * (y * y)) * 0.25 - coa


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'r16' / 'noiseprofile_bench.txt'))
    a = ap.parse_args()
    assert a.warmup >= 5 and a.iters >= 20
    dev = torch.device('cuda', 0)
    w, h = 4096, 3072
    lines = []

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    g = torch.Generator(device=dev).manual_seed(16)
    ramp = (0.03 + 0.9 * torch.linspace(0, 1, w, device=dev)[None, :] * torch.linspace(0.3, 1, h, device=dev)[:, None])
    clean = ramp + torch.randn((h, w), device=dev, generator=g) * torch.sqrt(2e-4 * ramp + 2e-6)
    for name, x, white in (('float32', clean, 1.0), ('float16', clean.half(), 1.0),
                           ('uint16', (clean * 65535).round().clamp(0, 65535).to(torch.int32).to(torch.int16).view(torch.uint16), 65535.0)):
        head = {'frame': f'mosaic {name}', 'size': [w, h], 'read_bytes': x.numel() * x.element_size()}
        us, batches = device_us(lambda: x.view(torch.int16 if name == 'uint16' else x.dtype).clone(), a.warmup, a.iters)
        copy_us = us
        emit({**head, 'op': 'copy of the bytes read (read + write)', 'us': round(us, 1), 'us_batches': batches})
        profile = td.NoiseProfile(dev, (w, h), td.BayerPattern.RGGB, white=white)
        us, batches = device_us(lambda: profile.estimate(x), a.warmup, a.iters)
        _native.profile_enable(True, 'tdk_noise_profile')
        for _ in range(a.iters):
            profile.estimate(x)
        torch.cuda.synchronize()
        launches = {k: round(ms * 1e3 / n, 1) for k, (n, ms) in _native.profile_report().items()}
        _native.profile_enable(False)
        model = profile.estimate(x)
        emit({**head, 'op': 'NoiseProfile.estimate bins=32', 'us': round(us, 1), 'us_batches': batches, 'GB_per_s_read': round(head['read_bytes'] / us * 1e-3, 1),
              'copy_us': round(copy_us, 1), 'launch_us': launches, 'lds_bytes': profile.lds_bytes(), 'workspace_bytes': profile.workspace_bytes(),
              'model': model.to_dict()})
        if name == 'float32':
            scale = 65535.0 / white
            us, batches = device_us(lambda: torch_blocks(x, scale), a.warmup, a.iters)
            emit({**head, 'op': 'torch composition of the block statistics (no binning, median or fit)', 'us': round(us, 1), 'us_batches': batches})
    del clean, ramp
    torch.cuda.empty_cache()

    model = td.NoiseModel.from_values((2e-4, 1.5e-4, 3e-4), 2e-6, dev)
    gains = torch.tensor([1.9, 1.0, 1.4], device=dev)
    av = (gains * model.a).view(1, 1, 3)
    cv = 0.375 * av * av + (gains * gains * model.b).view(1, 1, 3)
    kv = 2.0 / av
    rgb32 = torch.rand((h, w, 3), device=dev, generator=g)
    for name, x in (('float32', rgb32), ('float16', rgb32.half())):
        head = {'frame': f'rgb {name}', 'size': [w, h], 'read_bytes': x.numel() * x.element_size()}
        us, batches = device_us(lambda: x.clone(), a.warmup, a.iters)
        emit({**head, 'op': 'copy of the frame (read + write)', 'us': round(us, 1), 'us_batches': batches})
        us, batches = device_us(lambda: model.stabilize(x, gains=gains), a.warmup, a.iters)
        emit({**head, 'op': f'NoiseModel.stabilize {name} -> float32', 'us': round(us, 1), 'us_batches': batches})
        y = model.stabilize(x, gains=gains)
        for inverse in ('unbiased', 'algebraic'):
            us, batches = device_us(lambda: model.unstabilize(y, gains=gains, inverse=inverse, out_dtype=x.dtype), a.warmup, a.iters)
            emit({**head, 'op': f'NoiseModel.unstabilize ({inverse}) float32 -> {name}', 'us': round(us, 1), 'us_batches': batches})
        us, batches = device_us(lambda: torch_stabilize(x, av, cv, kv), a.warmup, a.iters)
        emit({**head, 'op': 'torch operations: stabilize', 'us': round(us, 1), 'us_batches': batches})
        us, batches = device_us(lambda: torch_unstabilize(y, av, cv / av).to(x.dtype), a.warmup, a.iters)
        emit({**head, 'op': 'torch operations: unstabilize (algebraic)', 'us': round(us, 1), 'us_batches': batches})
        if name == 'float32':
            us, batches = device_us(lambda: td.estimate_channel_noise(x), a.warmup, a.iters)
            emit({**head, 'op': 'estimate_channel_noise', 'us': round(us, 1), 'us_batches': batches})
        del y
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text('\n'.join([f'# profiles/noiseprofile_bench.py --warmup {a.warmup} --iters {a.iters} on {torch.cuda.get_device_name(0)}', *lines]) + '\n')


if __name__ == '__main__':
    main()
