"""ColorLUT.process (csrc/colorlut.hip) at 12 MP next to the torch composition of the same transform.

One 4096 x 3072 x 3 frame, float16 -> float16 and uint8 -> uint8.  Cases: no stage (the streaming floor), the matrix alone, a 3 x 1024
shaper alone, and a 3D LUT of N = 17 (nodes staged in LDS, and gathered from global memory with `global_nodes`), N = 33 and N = 65,
tetrahedral and trilinear, plus the whole chain matrix -> shaper -> LUT.  Beside them the torch way: `frame @ M.T` and a 5-D
`grid_sample` on the LUT as a (1, 3, N, N, N) volume (trilinear only, float types only: a uint8 frame is converted first and back after,
as a user would have to).  Device time per call between two HIP events on one stream around a batch of back-to-back calls, after
warm-up calls of the same shape; three batches per figure, the fastest is reported and all are listed.  spec_bytes: the frame read once
and written once.  One process; run it under a time limit:

  timeout -k 10 600 python3 profiles/colorlut_bench.py [--warmup 5] [--iters 20] [--out profiles/r14/colorlut_bench.txt]
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

MATRIX = [[0.9, 0.15, -0.05], [0.02, 0.8, 0.18], [-0.1, 0.25, 0.85]]


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


def look(n):
    """A mild grade: a gamma on every axis and a little cross-talk, (N, N, N, 3) indexed [b, g, r]."""
    axis = np.arange(n, dtype=np.float64) / (n - 1)
    b, g, r = np.meshgrid(axis, axis, axis, indexing='ij')
    p = np.stack((r, g, b), axis=-1) ** 0.9
    return (p @ np.asarray(MATRIX).T).astype(np.float32)


def torch_composition(frame, matrix, volume):
    """matmul + grid_sample: what the same transform costs without the kernel (trilinear; the coordinate tensor is as large as the frame)."""
    x = frame if frame.is_floating_point() else frame.to(torch.float16) / 255
    if matrix is not None:
        x = x @ matrix.to(x.dtype).T
    if volume is not None:
        grid = (x * 2 - 1).reshape(1, 1, *x.shape)                      # (1, 1, H, W, 3): x = r, y = g, z = b
        x = torch.nn.functional.grid_sample(volume.to(x.dtype), grid, mode='bilinear', padding_mode='border', align_corners=True)[0, :, 0].permute(1, 2, 0).contiguous()
    return x if frame.is_floating_point() else (x.clamp(0, 1) * 255).round().to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'r14' / 'colorlut_bench.txt'))
    a = ap.parse_args()
    assert a.warmup >= 5 and a.iters >= 20
    dev = torch.device('cuda', 0)
    w, h = 4096, 3072
    lines = []

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    g = torch.Generator(device='cpu').manual_seed(14)
    base = torch.rand((h, w, 3), generator=g)
    shaper = np.stack([np.linspace(0, 1, 1024) ** p for p in (0.45, 0.5, 0.55)])
    luts = {n: look(n) for n in (17, 33, 65)}
    for dtype in (torch.float16, torch.uint8):
        x = (base * 255).round().to(torch.uint8).to(dev) if dtype == torch.uint8 else base.to(dtype).to(dev)
        nbytes = 2 * x.numel() * x.element_size()
        head = {'size': [w, h], 'dtype': str(dtype).split('.')[-1], 'spec_bytes': nbytes}

        def run(label, obj, **extra):
            us, batches = device_us(lambda: obj.process(x), a.warmup, a.iters)
            emit({**head, 'op': label, 'us': round(us, 1), 'us_batches': batches, 'GB_per_s': round(nbytes / us * 1e-3, 1), 'lds_bytes': obj.lds_bytes(), **extra})
            return us

        run('ColorLUT no stage', td.ColorLUT(dev))
        run('ColorLUT matrix', td.ColorLUT.from_matrix(dev, MATRIX))
        run('ColorLUT shaper 3x1024', td.ColorLUT(dev, shaper=shaper))
        for n in (17, 33, 65):
            for interpolation in ('tetrahedral', 'trilinear'):
                obj = td.ColorLUT(dev, lut=luts[n], interpolation=interpolation)
                staged = run(f'ColorLUT N={n} {interpolation}' + (' staged' if n == 17 else ''), obj)
                if n == 17:
                    obj.global_nodes = True
                    run(f'ColorLUT N={n} {interpolation} global', obj, staged_us=round(staged, 1))
        run('ColorLUT matrix + shaper + N=33 tetrahedral', td.ColorLUT(dev, matrix=MATRIX, shaper=shaper, lut=luts[33]))
        run('ColorLUT matrix + shaper + N=17 tetrahedral', td.ColorLUT(dev, matrix=MATRIX, shaper=shaper, lut=luts[17]))
        matrix = torch.tensor(MATRIX, device=dev)
        for n in (17, 33):
            volume = torch.from_numpy(luts[n]).to(dev).permute(3, 0, 1, 2).unsqueeze(0).contiguous()
            for label, m, v in ((f'torch matmul + grid_sample N={n} trilinear', matrix, volume), (f'torch grid_sample N={n} trilinear', None, volume)):
                try:
                    us, batches = device_us(lambda: torch_composition(x, m, v), a.warmup, a.iters)
                    emit({**head, 'op': label, 'us': round(us, 1), 'us_batches': batches})
                except RuntimeError as e:
                    emit({**head, 'op': label, 'error': str(e).splitlines()[0][:160]})
        del x
        torch.cuda.empty_cache()
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text('\n'.join([f'# profiles/colorlut_bench.py --warmup {a.warmup} --iters {a.iters} on {torch.cuda.get_device_name(0)}', *lines]) + '\n')


if __name__ == '__main__':
    main()
