"""RawCodec.encode and .decode (csrc/rawcodec.hip) at 12 MP and 50 MP next to yardsticks that are not the code under test.

Frame: a 12-bit ramp along the row with Poisson-Gaussian noise (variance a*s + b on the signal s in 0..1; a = 1e-4, b = 4e-6 for the
timings), as uint16 codes and as packed 12-bit bytes.  Per size, in one process:
  encode from uint16 and from packed bytes: the whole call, and the device time of each of its three launches from the library's
    per-kernel event timer (tdk_profile_*), in a pass of its own;
  decode into uint16, float32, float16 and the two packed orders: the whole call, and the device time of its one launch from the same
    timer (the difference is what the host needs to enqueue a call, where that is the longer of the two);
  a device-to-device copy of the uint16 frame and of the packed frame (each byte read once and written once);
  decode12_float on the packed frame -- the kernel a packed upload goes through today;
  the host-to-device copy from pinned memory of the packed frame and of the stream (its length at the measured ratio).
Also the compression ratio on three noise levels, (a, b) = (2e-5, 1e-6), (1e-4, 4e-6), (4e-4, 1e-5), against the packed form.  No
frame of a real sensor is at hand: the figures are for the synthetic scene only.
Device time per call between two HIP events on one stream around a batch of back-to-back calls, after warm-up calls of the same shape;
five batches per figure, the MEDIAN is reported and all are listed.  One process; run it under a time limit:

  timeout -k 10 600 python3 profiles/rawcodec_bench.py [--warmup 5] [--iters 200] [--out profiles/r21/rawcodec_bench.txt]
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


def launches_us(fn, iters, prefix):
    """{kernel name: device us per launch} from the library's event timer."""
    _native.profile_enable(True, prefix)
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    report = _native.profile_report()
    _native.profile_enable(False)
    return {name: round(ms * 1e3 / count, 1) for name, (count, ms) in report.items()}


def noisy_ramp(w, h, a, b, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    s = torch.linspace(0.02, 0.9, w, device=dev)[None, :].expand(h, w)
    noisy = s + torch.sqrt(a * s + b) * torch.randn((h, w), device=dev, generator=g)
    return (noisy * 4095.0).round().clamp(0, 4095).to(torch.int16).view(torch.uint16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=200)   # a window of 5 to 50 ms
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'r21' / 'rawcodec_bench.txt'))
    a = ap.parse_args()
    assert a.warmup >= 5 and a.iters >= 20
    dev = torch.device('cuda', 0)
    lines = []

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    for w, h in ((4096, 3072), (8192, 6144)):
        codec = td.RawCodec(dev, (w, h))
        head = {'size': [w, h]}
        for na, nb in ((2e-5, 1e-6), (1e-4, 4e-6), (4e-4, 1e-5)):
            frame = noisy_ramp(w, h, na, nb, dev, seed=21)
            n = int(codec.encode(frame).length.item())
            emit({**head, 'op': 'compression of the noisy 12-bit ramp', 'a': na, 'b': nb, 'stream_bytes': n, 'bits_per_site': round(8 * n / (w * h), 3),
                  'times_smaller_than_packed12': round(codec.packed_bytes() / n, 3)})
        frame = noisy_ramp(w, h, 1e-4, 4e-6, dev, seed=21)
        packed = td.encode12_u16(frame.reshape(-1))
        out = torch.empty(codec.max_stream_bytes(), dtype=torch.uint8, device=dev)
        res = codec.encode(frame, out=out)
        n = int(res.length.item())
        stream = res.data[:n].clone()
        assert torch.equal(codec.decode(stream).view(torch.int16), frame.view(torch.int16))
        assert torch.equal(codec.decode(stream, output=td.PackedFormat.Packed12), packed)

        copy16_us, batches = device_us(lambda: frame.view(torch.int16).clone(), a.warmup, a.iters)
        emit({**head, 'op': 'device copy of the uint16 frame', 'bytes': 2 * w * h, 'us': round(copy16_us, 1), 'us_batches': batches})
        copy12_us, batches = device_us(lambda: packed.clone(), a.warmup, a.iters)
        emit({**head, 'op': 'device copy of the packed frame', 'bytes': packed.numel(), 'us': round(copy12_us, 1), 'us_batches': batches})
        us, batches = device_us(lambda: td.decode12_float(packed), a.warmup, a.iters)
        emit({**head, 'op': 'decode12_float of the packed frame', 'us': round(us, 1), 'us_batches': batches})

        for name, run in (('uint16', lambda: codec.encode(frame, out=out)), ('packed 12', lambda: codec.encode(packed, out=out, packed_format=td.PackedFormat.Packed12))):
            us, batches = device_us(run, a.warmup, a.iters)
            emit({**head, 'op': f'RawCodec.encode from {name}', 'stream_bytes': n, 'us': round(us, 1), 'us_batches': batches, 'times_the_uint16_copy': round(us / copy16_us, 2),
                  'launches_us': launches_us(run, a.iters, 'tdk_rawcodec')})
        target = torch.empty(w * h * 4, dtype=torch.uint8, device=dev)
        for name, output, size in (('uint16', torch.uint16, 2), ('float32', torch.float32, 4), ('float16', torch.float16, 2)):
            view = target[:w * h * size].view(output).view(h, w)
            run = lambda: codec.decode(stream, output=output, out=view)
            us, batches = device_us(run, a.warmup, a.iters)
            emit({**head, 'op': f'RawCodec.decode into {name}', 'bytes_read': n, 'bytes_written': w * h * size, 'us': round(us, 1), 'us_batches': batches,
                  'times_the_uint16_copy': round(us / copy16_us, 2), 'launches_us': launches_us(run, a.iters, 'tdk_rawcodec')})
        for fmt in (td.PackedFormat.Packed12, td.PackedFormat.Packed12_IDS):
            view = target[:packed.numel()]
            run = lambda: codec.decode(stream, output=fmt, out=view)
            us, batches = device_us(run, a.warmup, a.iters)
            emit({**head, 'op': f'RawCodec.decode into {fmt.name}', 'bytes_read': n, 'bytes_written': packed.numel(), 'us': round(us, 1), 'us_batches': batches,
                  'times_the_packed_copy': round(us / copy12_us, 2), 'launches_us': launches_us(run, a.iters, 'tdk_rawcodec')})

        pinned_packed, pinned_stream = packed.cpu().pin_memory(), stream.cpu().pin_memory()
        landing = torch.empty(packed.numel(), dtype=torch.uint8, device=dev)
        us12, batches12 = device_us(lambda: landing.copy_(pinned_packed, non_blocking=True), a.warmup, a.iters)
        usz, batchesz = device_us(lambda: landing[:n].copy_(pinned_stream, non_blocking=True), a.warmup, a.iters)
        emit({**head, 'op': 'host-to-device copy from pinned memory', 'packed_bytes': packed.numel(), 'packed_us': round(us12, 1), 'packed_us_batches': batches12,
              'stream_bytes': n, 'stream_us': round(usz, 1), 'stream_us_batches': batchesz})
        del frame, packed, out, stream, target, landing
        torch.cuda.empty_cache()

    out_path = Path(a.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text('\n'.join([f'# profiles/rawcodec_bench.py --warmup {a.warmup} --iters {a.iters} on {torch.cuda.get_device_name(0)}', *lines]) + '\n')


if __name__ == '__main__':
    main()
