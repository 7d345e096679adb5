"""Wavelet.process (csrc/wavelet.hip) at 12 MP and 50 MP against the Wiener call BASELINE config 5 runs today.

float16 frames of 3 channels (4096 x 3072 and 8192 x 6144), luma/chroma mode, S = 3 and S = 5 scales, thresholds from
Wavelet.from_sigma(sigma 0.05).  On the same frames, in the same process: Wiener.process C = 3 (tile 32, overlap 4, sigma 0.05).
Device time per call between two HIP events on one stream around a batch of back-to-back calls, after warm-up calls of the same
shape; three batches per figure, the fastest is reported and all are listed.  The bytes are those of DESIGN.md 3.9 (what each launch
reads and writes once per pixel, aprons not counted); the time of each launch comes from the library's own event timer in a pass of
its own (profile_enable), which serialises nothing else.

  python3 profiles/wavelet_bench.py [--warmup 5] [--iters 20] [--out profiles/r12/wavelet_bench.txt]
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
from torch_darktable import _native  # noqa: E402


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


def spec_bytes_per_pixel(scales, channels=3, esz=2):
    """the fine launch reads the frame; up to two scales it writes the frame, otherwise two float32 planes per channel.
    A coarse launch reads two planes per channel; the last writes the frame, the others two planes."""
    if scales <= td.Wavelet.FUSED:
        return 2 * channels * esz
    coarse = scales - td.Wavelet.FUSED
    return channels * (esz + 8) + (coarse - 1) * channels * 16 + channels * (8 + esz)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'r12' / 'wavelet_bench.txt'))
    a = ap.parse_args()
    assert a.warmup >= 5 and a.iters >= 20
    dev = torch.device('cuda', 0)
    lines = []

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    for w, h in ((4096, 3072), (8192, 6144)):
        x = torch.from_numpy(np.random.default_rng(7).random((h, w, 3), dtype=np.float32)).to(dev).half()
        wiener = td.Wiener(dev, (w, h), overlap_factor=4, tile_size=32)
        wiener_us, wiener_batches = device_us(lambda: wiener.process(x, 0.05), a.warmup, a.iters)
        emit({'size': [w, h], 'op': 'Wiener.process C=3 (32, 4) sigma 0.05, float16', 'us': round(wiener_us, 1), 'us_batches': wiener_batches})
        for scales in (3, 5):
            wav = td.Wavelet.from_sigma(dev, (w, h), (0.05, 0.05, 0.05), scales=scales)
            us, batches = device_us(lambda: wav.process(x), a.warmup, a.iters)
            _native.profile_enable(True, 'tdk_wavelet(')
            for _ in range(a.iters):
                wav.process(x)
            torch.cuda.synchronize()
            report = _native.profile_report()
            _native.profile_enable(False)
            per_launch = {name: round(ms * 1e3 / n, 1) for name, (n, ms) in sorted(report.items())}
            nbytes = spec_bytes_per_pixel(scales) * w * h
            emit({'size': [w, h], 'op': f'Wavelet.process ycc S={scales}, float16', 'us': round(us, 1), 'us_batches': batches,
                  'spec_bytes': nbytes, 'GB_per_s': round(nbytes / us * 1e-3, 1), 'us_per_launch': per_launch,
                  'slowest_launch': max(per_launch, key=per_launch.get), 'workspace_bytes': wav.workspace_bytes(3),
                  'lds_bytes': wav.lds_bytes(3, torch.float16), 'wavelet_over_wiener': round(us / wiener_us, 2)})
            del wav
        del x, wiener
        torch.cuda.empty_cache()
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text('\n'.join([f'# profiles/wavelet_bench.py --warmup {a.warmup} --iters {a.iters} on {torch.cuda.get_device_name(0)}', *lines]) + '\n')


if __name__ == '__main__':
    main()
