"""Filmic.process (csrc/filmic.hip) at 12 MP against the reference's reinhard_tonemap on the same frame, against a device copy of the
same bytes and against the same arithmetic composed from torch operations.

4096 x 3072 frames of float32 and float16 to uint8, the default curve and sRGB, under each norm.  On the same frames, in the same
process:
  * reinhard: reinhard_tonemap(frame, metrics, params) to uint8, the mapper the stage takes the place of in ImageProcessor;
  * copy: a uint8 buffer of (source bytes + destination bytes) / 2 copied to another -- as many bytes read and written together as
    the stage moves;
  * torch: the steps of the header from torch operations (the index from the float's bits, gathers of the tables, the ratios, the
    gamut step, the encoding) in float32; it is held to the stage's bytes and the count of differing bytes is reported.
Device time per call between two HIP events on one stream around a batch of back-to-back calls, after warm-up calls of the same
shape; three batches per figure, the fastest is reported and all are listed.

  python3 profiles/filmic_bench.py [--warmup 5] [--iters 20] [--out profiles/r24/filmic_bench.txt]

On a shared machine run it with a time limit of its own, e.g.  timeout -k 10 300 python3 profiles/filmic_bench.py && next step.
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


def torch_composition(f):
    """The stage from torch operations, float32 arithmetic: a callable frame -> uint8 frame."""
    T, D = f.curve_table[0], f.curve_table[1]
    G = f.encode_table
    weights = torch.tensor(f.weights, device=T.device)
    xmin, xmax = 2.0 ** -20, 4096.0 - 2.0 ** -12

    def look(table, value, ev_min):
        bits = value.view(torch.int32)
        i = (((bits >> 23) - 127 - ev_min) * 32 + ((bits >> 18) & 31)).long()
        frac = (bits & 0x3FFFF).float() / 262144.0
        lo, hi = table[i], table[i + 1]
        return lo + frac * (hi - lo)

    def run(x):
        p = torch.nan_to_num(x.float() * f.exposure, nan=0.0, posinf=xmax, neginf=0.0).clamp(0.0, xmax)
        if f.norm == 'none':
            o = look(T, p.clamp(xmin, xmax), -20)
        else:
            if f.norm == 'max':
                n = p.amax(-1)
            elif f.norm == 'luma':
                n = (p * weights).sum(-1)
            else:
                den = (p * p).sum(-1)
                n = torch.where(den > 0, (p * p * p).sum(-1) / den.clamp_min(1e-38), torch.zeros_like(den))
            nc = n.clamp(xmin, xmax)
            y, d = look(T, nc, -20)[..., None], look(D, nc, -20)[..., None]
            o = y * (1.0 + d * (p / nc[..., None] - 1.0))
            m = o.amax(-1, keepdim=True)
            pulled = torch.where(y >= 1.0, torch.ones_like(o), y + (o - y) * ((1.0 - y) / (m - y).clamp_min(1e-30)))
            o = torch.where(m > 1.0, pulled, o)
        oc = o.clamp(0.0, 1.0 - 2.0 ** -24)
        v = torch.where(oc < 2.0 ** -16, oc * 65536.0 * G[0], look(G, oc.clamp_min(2.0 ** -16), -16))
        return torch.round(v.clamp(0.0, 1.0) * 255.0).to(torch.uint8)

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--size', type=int, nargs=2, default=(4096, 3072), metavar=('W', 'H'))
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'r24' / 'filmic_bench.txt'))
    a = ap.parse_args()
    assert a.warmup >= 5 and a.iters >= 20
    assert torch.cuda.is_available(), 'the measurement needs the GPU: there is no fallback'
    dev = torch.device('cuda', 0)
    w, h = a.size
    lines = []

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    # a scene of coloured patches over twelve stops, a tenth of it above white
    rng = np.random.default_rng(7)
    patches = rng.uniform(0.05, 1.0, (h // 48 + 1, w // 48 + 1, 3)).repeat(48, 0).repeat(48, 1)[:h, :w]
    level = np.exp2(rng.uniform(-10.0, 2.0, (h // 48 + 1, w // 48 + 1, 1))).repeat(48, 0).repeat(48, 1)[:h, :w]
    frame = torch.from_numpy((patches * level * rng.uniform(0.8, 1.0, (h, w, 1))).astype(np.float32)).to(dev)
    del patches, level
    params = td.TonemapParameters(1.0, 1.0, 0.8, 0.0)
    for dtype in (torch.float32, torch.float16):
        x = frame.to(dtype)
        nbytes = x.numel() * x.element_size() + x.numel()
        a_buf = torch.zeros(nbytes // 2, dtype=torch.uint8, device=dev)
        b_buf = torch.empty_like(a_buf)
        copy_us, copy_batches = device_us(lambda: b_buf.copy_(a_buf), a.warmup, a.iters)
        emit({'size': [w, h], 'src': str(dtype), 'dst': 'torch.uint8', 'op': 'copy (as many bytes read and written together)', 'us': round(copy_us, 1),
              'us_batches': copy_batches, 'bytes': nbytes, 'GB_per_s': round(nbytes / copy_us * 1e-3, 1)})
        metrics = td.compute_image_metrics([x], stride=8, min_gray=1e-4)
        reinhard_us, reinhard_batches = device_us(lambda: td.reinhard_tonemap(x, metrics, params), a.warmup, a.iters)
        emit({'size': [w, h], 'src': str(dtype), 'dst': 'torch.uint8', 'op': 'reinhard_tonemap', 'us': round(reinhard_us, 1), 'us_batches': reinhard_batches,
              'GB_per_s': round(nbytes / reinhard_us * 1e-3, 1), 'over_copy': round(reinhard_us / copy_us, 2)})
        for norm in ('max', 'luma', 'power', 'none'):
            f = td.Filmic(dev, norm=norm)
            us, batches = device_us(lambda: f.process(x), a.warmup, a.iters)
            compose = torch_composition(f)
            torch_us, torch_batches = device_us(lambda: compose(x), a.warmup, a.iters)
            got, ref = f.process(x), compose(x)
            differing = int((got != ref).sum().item())
            step = int((got.int() - ref.int()).abs().max().item())
            emit({'size': [w, h], 'src': str(dtype), 'dst': 'torch.uint8', 'op': f"Filmic.process norm='{norm}' encoding='srgb'", 'us': round(us, 1), 'us_batches': batches,
                  'bytes': nbytes, 'GB_per_s': round(nbytes / us * 1e-3, 1), 'over_copy': round(us / copy_us, 2), 'over_reinhard': round(us / reinhard_us, 2),
                  'torch_us': round(torch_us, 1), 'torch_us_batches': torch_batches, 'torch_over_stage': round(torch_us / us, 1),
                  'bytes_differing_from_torch': differing, 'largest_difference_in_codes': step, 'lds_bytes': f.lds_bytes})
            del compose, got, ref, f
        del x, a_buf, b_buf
        torch.cuda.empty_cache()
    path = Path(a.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text('\n'.join([f'# profiles/filmic_bench.py --warmup {a.warmup} --iters {a.iters} on {torch.cuda.get_device_name(0)}', *lines]) + '\n')


if __name__ == '__main__':
    main()
