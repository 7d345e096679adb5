"""The tone mapper's table form against the per-pixel kernel it stands in for (csrc/tonemap.hip, include/tdk_hip_tables.h), alone
on one 12 MP binary16 frame, under the library's event timer.

    python profiles/tonemap_table_bench.py [--runs 5] [--launches 20]      # both forms alternating, on two frames
    python profiles/tonemap_table_bench.py --once table|direct [--frame chain|noise]   # 3 launches, no timer: for a counter pass

Frames: `chain` is what the benchmark hands to the tone mapper (bench.py's Lab chain on its first synthetic mosaic, with that frame's
metrics); `noise` is uniform random in [0, 1], where the 64 lanes of a gather touch 64 different cache lines of the table.
The per-pixel kernel is run through verification_paths(tonemap_direct=True): it is the kernel the table form replaced, unchanged.
The first row is what the event timer reads for a launch that does next to nothing: the floor under every other figure."""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / 'torch-darktable_amd'))
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

W, H = 4096, 3072


def frames(td, dev):
    from torch_darktable.synthetic import synthetic_bayer

    rcd = td.RCD(dev, (W, H), td.BayerPattern.RGGB)
    wiener = td.Wiener(dev, (W, H), overlap_factor=4, tile_size=32)
    bilateral = td.Bilateral(dev, (W, H), sigma_s=2.0, sigma_r=0.2)
    lum = torch.empty((H, W), dtype=torch.float32, device=dev)
    ab = torch.empty((H, W, 2), dtype=torch.float32, device=dev)
    acc = td.tonemap.MetricsAccumulator(dev, stride=8)
    rgb = rcd.process(synthetic_bayer(H, W, seed=1234, device=dev).to(torch.float16))
    wiener.process_log_luminance_lab(rgb, 0.075, luminance_out=lum, chroma_out=ab)
    chain = bilateral.process_lab(lum, ab, 0.4, out_dtype=torch.float16, metrics=acc)
    metrics = acc.finish()
    torch.manual_seed(7)
    noise = torch.rand((H, W, 3), device=dev).to(torch.float16)
    torch.cuda.synchronize()
    return {'chain': (chain, metrics), 'noise': (noise, td.compute_image_metrics([noise], stride=8))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--once', choices=('table', 'direct'))
    ap.add_argument('--frame', choices=('chain', 'noise'), default='chain')
    args = ap.parse_args()
    import torch_darktable as td
    from torch_darktable import _native
    from torch_darktable.torch_darktable_extension import verification_paths

    dev = torch.device('cuda', 0)
    params = td.TonemapParameters(gamma=0.75, intensity=2.0, light_adapt=1.0, vibrance=0.0)
    data = frames(td, dev)

    def run(form, frame, n):
        x, m = data[frame]
        with verification_paths(tonemap_direct=form == 'direct'):
            for _ in range(n):
                out = td.reinhard_tonemap(x, m, params)
        torch.cuda.synchronize()
        return out

    if args.once:
        run(args.once, args.frame, 3)
        return
    # what the event timer reads for a launch that does next to nothing (one workgroup zeroing eight floats): the floor under every figure below
    scratch = torch.zeros(8, dtype=torch.float32, device=dev)
    floor = []
    for _ in range(args.runs):
        _native.profile_enable(True, 'tdk_image_metrics_init')
        for _ in range(args.launches):
            _native.check(_native.lib.tdk_image_metrics_init(scratch.data_ptr(), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        n, ms = _native.profile_report()['tdk_image_metrics_init']
        _native.profile_enable(False)
        floor.append(ms / n * 1e3)
    print('== timer floor (tdk_image_metrics_init)  ' + '  '.join(f'{v:7.2f}' for v in floor) + ' us per launch')
    for frame in data:
        same = torch.equal(run('table', frame, 1), run('direct', frame, 1))
        print(f'== {frame}: table form equals the per-pixel kernel: {same}; metrics {[round(v, 4) for v in data[frame][1].tolist()]}')
        rows = {}
        for _ in range(args.runs):
            for form in ('direct', 'table'):
                run(form, frame, 2)
                _native.profile_enable(True, 'tdk_tonemap')
                run(form, frame, args.launches)
                report = _native.profile_report()
                _native.profile_enable(False)
                for name, (n, ms) in report.items():
                    rows.setdefault((form, name), []).append(ms / n * 1e3)
        for (form, name), us in rows.items():
            print(f'  {form:7s} {name:22s} ' + '  '.join(f'{v:7.2f}' for v in us) + f'      min {min(us):.2f}  max {max(us):.2f} us per launch')


if __name__ == '__main__':
    main()
