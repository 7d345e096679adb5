"""ScaledDemosaic (csrc/scaled_demosaic.hip) on a 12 MP mosaic at ratios 2, 3, 4 and 8 from float32, binary16 and packed 12-bit
sources, beside

  (a) RCD.process + Resize to the same size on the same sitting: the path the stage replaces, the yardstick;
  (b) a device copy of the bytes the call reads and writes: what reading the mosaic once costs;
  (c) ImageProcessor.process_preview against process_resized at resize_width = W / 2 and W / 4, whole chain.

Device time per call between two HIP events around a batch of back-to-back calls, after warm-up calls of the same shape; the stage
and the yardstick alternate, three batches each per figure, the fastest is reported and all three are listed.  A row whose stage is
not below (a) is marked: the stage is what (a) is for, so that is a finding and wants its reason written beside the table.

  python3 profiles/scaled_demosaic_bench.py [--size 4096x3072] [--warmup 5] [--iters 50] [--out profiles/r30/scaled_demosaic_bench.txt]
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
from torch_darktable.pipeline import Debayer, ImageProcessingSettings, ImageProcessor, ToneMapper  # noqa: E402

GAINS = (1.9, 1.0, 1.6)


def batch_us(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


def alternating_us(fns, warmup, iters):
    """{name: (fastest batch, the three batches)} of several callables, warmed up and then timed in turn, three rounds."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(3):
        for name, fn in fns.items():
            times[name].append(batch_us(fn, iters))
    return {name: (min(t), [round(v, 1) for v in t]) for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', default='4096x3072')
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'r30' / 'scaled_demosaic_bench.txt'))
    a = ap.parse_args()
    assert a.warmup >= 5 and a.iters >= 50
    assert torch.cuda.is_available(), 'this measurement needs the GPU: there is no fallback'
    w, h = map(int, a.size.split('x'))
    dev, pattern = torch.device('cuda', 0), td.BayerPattern.RGGB
    codes = torch.from_numpy(np.random.default_rng(7).integers(0, 4096, (h, w)).astype(np.uint16)).to(dev)
    packed = td.encode12_u16(codes.view(-1))
    mosaic32 = td.decode12_float(packed).view(h, w)
    gains = torch.tensor(GAINS, device=dev)
    rcd = td.RCD(dev, (w, h), pattern)
    lines, rows = [], []

    def emit(row):
        rows.append(row)
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    for ratio in (2, 3, 4, 8):
        ow, oh = w // ratio, h // ratio
        stage, resize = td.ScaledDemosaic(dev, (w, h), pattern, (ow, oh)), td.Resize(dev, (w, h), (ow, oh))
        for kind in ('float32', 'float16', 'packed'):
            storage = torch.float16 if kind == 'float16' else torch.float32
            mosaic = mosaic32.to(storage)
            read = packed.numel() if kind == 'packed' else mosaic.numel() * mosaic.element_size()
            written = ow * oh * 3 * (2 if storage == torch.float16 else 4)
            blob_in, blob_out = torch.empty(read, dtype=torch.uint8, device=dev), torch.empty(read, dtype=torch.uint8, device=dev)
            small_in, small_out = torch.empty(written, dtype=torch.uint8, device=dev), torch.empty(written, dtype=torch.uint8, device=dev)
            if kind == 'packed':
                this = lambda: stage.process_packed(packed, td.PackedFormat.Packed12, gains, storage)
                that = lambda: resize.process(rcd.process_packed(packed, gains, td.PackedFormat.Packed12, storage))
            else:
                this = lambda: stage.process(mosaic, gains)
                that = lambda: resize.process(rcd.process(td.apply_white_balance(mosaic, gains, pattern).unsqueeze(-1)))

            def copy():   # as many bytes read as the stage reads, as many written as it writes (the copy of the source writes them too: an upper bound)
                blob_out.copy_(blob_in)
                small_out.copy_(small_in)

            t = alternating_us({'stage': this, 'rcd_resize': that, 'copy': copy}, a.warmup, a.iters)
            us, ref = t['stage'][0], t['rcd_resize'][0]
            emit({'src': [w, h], 'dst': [ow, oh], 'ratio': ratio, 'source': kind, 'tile': list(stage.tile), 'lds_bytes': stage.lds_bytes(),
                  'stage_us': round(us, 1), 'stage_us_batches': t['stage'][1], 'rcd_resize_us': round(ref, 1), 'rcd_resize_us_batches': t['rcd_resize'][1],
                  'rcd_resize_over_stage': round(ref / us, 2), 'copy_us': round(t['copy'][0], 1), 'copy_us_batches': t['copy'][1],
                  'algorithmic_bytes': read + written, 'stage_GB_per_s': round((read + written) / us * 1e-3, 1), 'not_below_rcd_resize': bool(us >= ref)})

    # (c) the whole chain
    settings = ImageProcessingSettings(postprocess=False, enable_denoise=True, enable_bilateral=True, tone_mapping=ToneMapper.reinhard, debayer=Debayer.rcd)
    for divisor in (2, 4):
        width = max(w, h) // divisor
        p = ImageProcessor((w, h), pattern, td.PackedFormat.Packed12, settings.model_copy(update={'resize_width': width}), dev, GAINS)
        p.preview = td.ScaledDemosaic.longest_edge(dev, (w, h), pattern, width)
        t = alternating_us({'preview': lambda: p.process_preview(packed, 'camera'), 'resized': lambda: p.process_resized(packed, 'camera')}, a.warmup, a.iters)
        emit({'chain': 'process_preview against process_resized', 'src': [w, h], 'dst': list(p.preview.output_size), 'resize_width': width,
              'process_preview_us': round(t['preview'][0], 1), 'process_preview_us_batches': t['preview'][1], 'process_resized_us': round(t['resized'][0], 1),
              'process_resized_us_batches': t['resized'][1], 'resized_over_preview': round(t['resized'][0] / t['preview'][0], 2)})

    lines.append(json.dumps({'device': torch.cuda.get_device_name(0), 'warmup': a.warmup, 'iters': a.iters}))
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text('\n'.join(lines) + '\n')
    print(f'wrote {out}')


if __name__ == '__main__':
    main()
