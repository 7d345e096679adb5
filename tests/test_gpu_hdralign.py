"""GPU: exposure brackets of a moving rig (torch_darktable.MotionHdrMerge, include/tdk_hip_hdralign.h) against the NumPy restatement of
the specification, tests/hdralign_spec.py (held to literal loops and to the block's purpose in tests/test_hdralign_spec.py).

Every bit of the output, every byte of the mask and of the pyramids and every integer of the fields and costs must be the
restatement's: there is no tolerance anywhere in this file and no site is excluded.  Shapes are sized by the two tiles -- 32 x 32
sites of a workgroup of the merge, 64 x 32 of a displacement -- and are the smallest that reach the paths: one cell, one merge tile, a
seam of merge tiles inside a motion tile, a seam of motion tiles, and ragged edges in both axes.  The brackets, the classes of special
samples and the comparison are those of tests/test_gpu_hdrmerge.py."""
import numpy as np
import pytest
import torch

import hdralign_spec as spec
import hdrmerge_spec as hspec
import motion_spec as mspec
import test_gpu_hdrmerge as plain        # the brackets, upload, bits, same (nothing of it is collected here)
import test_motion_spec as chartlib      # the chart and its crops

pytestmark = pytest.mark.gpu

F = np.float32
MODEL, EXPOSURES, SHUTTER, PATTERNS, TORCH = plain.MODEL, plain.EXPOSURES, plain.SHUTTER, plain.PATTERNS, plain.TORCH
SIZES = [(2, 2), (34, 30), (64, 32), (66, 34), (130, 66), (200, 100)]   # (w, h)
FIELDS = ('zeros', 'uniform', 'random', 'extreme', 'outside')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a visible MI355X'
    return torch.device('cuda', 0)


def fields_of(kind, nf, w, h, ref, seed=0):
    """Hand-made displacements; the row of ref holds what must never be read."""
    ny, nx = mspec.tiles(w, h)
    rng = np.random.default_rng(seed + 7 * w + h)
    fields = np.zeros((nf, ny, nx, 2), np.int16)
    if kind == 'uniform':
        for f in range(nf):
            fields[f] = (2 * ((f % 5) - 2), 4 * (f % 4) - 2)   # even, another one per frame
    elif kind == 'random':
        fields[:] = rng.integers(-78, 79, fields.shape)         # per tile, odd values among them
    elif kind == 'extreme':
        fields[:] = rng.choice(np.array([32767, -32767, -32768, 0, 2], np.int16), fields.shape)
    elif kind == 'outside':
        fields[:] = rng.integers(-6, 7, fields.shape)
        fields[(ref + 1) % nf] = (2 * h + 2, -2)                # one frame wholly outside, at every tile
    elif kind != 'zeros':
        raise KeyError(kind)
    fields[ref] = 12345
    return fields


def run(td, dev, w, h, kind='random', nf=3, ref=0, pattern='RGGB', src=np.float32, out=None, offsets=(1, 0, 3), kinds=plain.KINDS, exposures=EXPOSURES, seed=0,
        edit=None, what='', **kw):
    """One aligned merge with given fields against the restatement, with and without the mask."""
    e = exposures[nf]
    frames = plain.bracket(w, h, e, src, kinds, seed, td.HdrMerge.TILE)
    if edit:
        edit(frames)
    fields = fields_of(kind, nf, w, h, ref, seed)
    m = td.NoiseModel(torch.from_numpy(np.asarray(MODEL, F)).to(dev))
    merge = td.MotionHdrMerge(dev, (w, h), td.BayerPattern[pattern], m, **kw)
    xs = [plain.upload(x, dev, offsets[f % len(offsets)]) for f, x in enumerate(frames)]
    device_fields = torch.from_numpy(fields).to(dev)
    out_dtype = None if out is None else TORCH[out]
    got, got_mask = merge.process(xs, e, ref=ref, out_dtype=out_dtype, return_mask=True, fields=device_fields)
    alone = merge.process(xs, e, ref=ref, out_dtype=out_dtype, fields=device_fields)
    torch.cuda.synchronize()
    want, want_mask = spec.merge(frames, e, fields, MODEL, PATTERNS[pattern], ref, out_dtype=out, **kw)
    what = f'{what} {kind} {w}x{h} F={nf} ref={ref}'
    ok = plain.same(got, got_mask, want, want_mask, what)
    ok = plain.same(alone, None, want, want_mask, what + ' (mask=NULL)') and ok
    if kind == 'zeros':   # ... and the plain merge on the GPU, bit for bit, mask included
        base, base_mask = td.HdrMerge(dev, (w, h), td.BayerPattern[pattern], m, **kw).process(xs, e, ref=ref, out_dtype=out_dtype, return_mask=True)
        same_bits = torch.equal(base.view(torch.int32 if base.dtype == torch.float32 else torch.int16), got.view(torch.int32 if got.dtype == torch.float32 else torch.int16))
        if not (same_bits and torch.equal(base_mask, got_mask)):
            print(f'{what}: differs from HdrMerge.process')
            ok = False
    return ok


# ------------------------------------------------------------------ 1. the merge with hand-made fields
@pytest.mark.parametrize('kind', FIELDS)
@pytest.mark.parametrize('which', range(len(SIZES)))
def test_every_size_and_class_of_field(td, dev, which, kind):
    w, h = SIZES[which]
    assert run(td, dev, w, h, kind, radius=2 + which % 2, what=f'radius {2 + which % 2}')


@pytest.mark.parametrize('radius', [2, 3])
@pytest.mark.parametrize('nf', [2, 3, 8])
def test_every_frame_count_anchor_and_radius(td, dev, nf, radius):
    ok = True
    for ref in sorted({0, nf // 2, nf - 1}):
        for kind in ('random', 'outside'):
            ok = run(td, dev, 130, 66, kind, nf=nf, ref=ref, radius=radius, what='anchor') and ok
    assert ok


@pytest.mark.parametrize('pattern', list(PATTERNS))
def test_every_pattern(td, dev, pattern):
    for radius in (2, 3):
        assert run(td, dev, 66, 34, 'random', pattern=pattern, radius=radius, what=pattern)


@pytest.mark.parametrize('src', [np.float32, np.float16], ids=['src32', 'src16'])
@pytest.mark.parametrize('out', [np.float32, np.float16], ids=['out32', 'out16'])
def test_every_combination_of_storage_types(td, dev, src, out):
    ok = True
    for radius, offsets, nf, kind in ((2, (1, 3, 5), 3, 'random'), (3, (0,), 8, 'uniform'), (2, (0, 1), 3, 'zeros')):
        ok = run(td, dev, 130, 66, kind, nf=nf, ref=1, pattern='GRBG', src=src, out=out, radius=radius, offsets=offsets, what=f'{src.__name__}/{out.__name__}') and ok
    assert ok


@pytest.mark.parametrize('kind', plain.KINDS)
def test_every_class_of_input_alone(td, dev, kind):
    ok = True
    for w, h in ((66, 34), (200, 100)):
        for nf, fields in ((3, 'random'), (8, 'uniform')):
            ok = run(td, dev, w, h, fields, nf=nf, ref=nf - 2, kinds=(kind,), seed=7, what=kind) and ok
    assert ok


def test_every_frame_blown_near_an_edge(td, dev):
    """Rule 5: where the shortest frame's displaced sample lies outside the frame the site takes ref; no site is NaN."""
    def blow(frames):
        for x in frames:
            x[:7, -9:] = 1.0
            x[-5:, :6] = 1.0
            x[28:36, 60:70] = 1.0   # across a seam of motion tiles
    ok = True
    for ref in (0, 1, 2):   # (frame 2 is the shortest of EXPOSURES[3])
        for kind in ('uniform', 'random', 'outside', 'extreme'):
            ok = run(td, dev, 130, 66, kind, ref=ref, kinds=('noise',), edit=blow, what='blown at the edges') and ok
    assert ok
    frames = plain.bracket(130, 66, EXPOSURES[3], kinds=('noise',))
    blow(frames)
    fields = fields_of('uniform', 3, 130, 66, 0)
    out, mask = spec.merge(frames, EXPOSURES[3], fields, MODEL, hspec.RGGB, 0)
    assert not np.isnan(out).any() and (mask[:4, -4:] & 8).all() and (mask[:4, -4:] & 7 == 0).all()   # frame 2 reads (0, 6) further on: outside


def test_exposures_that_are_no_whole_stops_and_other_parameters(td, dev):
    ok = True
    for nf in sorted(SHUTTER):
        ok = run(td, dev, 130, 66, 'random', nf=nf, ref=nf - 1, src=np.float16 if nf % 2 else np.float32, exposures=SHUTTER, radius=2 + nf % 2, what='shutter times') and ok
    for kw in (dict(pixel_threshold=None), dict(thresholds=(0.8, 1.1), pixel_threshold=2.0), dict(clip=0.5)):
        ok = run(td, dev, 66, 34, 'random', what=str(kw), **kw) and ok
    assert ok


# ------------------------------------------------------------------ 2. pyramids, fields and costs
def chart_bracket(w, h, exposures, shifts, seed=0, gain=1.3, dtype=np.float32):
    """The chart of tests/test_motion_spec.py shot as a bracket, frame f panned by shifts[f] (frame_f[p + shift] is the anchor's p), with
    model noise, the sensor saturating at 1."""
    big = chartlib.chart(h + 2 * chartlib.PAD, w + 2 * chartlib.PAD)
    rng = np.random.default_rng(seed)
    top = max(exposures)
    frames = []
    for e, s in zip(exposures, shifts):
        clean = gain * chartlib.crop(big, h, w, -s[0], -s[1]) * (e / top)
        frames.append(np.minimum(clean + rng.normal(size=clean.shape) * np.sqrt(3e-4 * clean + 2e-6), 1.0).astype(dtype))
    return frames


def same_alignment(merge, frames, exposures, ref, what):
    """The pyramids of every frame, and the fields and costs of every frame but ref, against the restatement."""
    me = merge.motion
    want_fields, want_costs, want_pyramids = spec.align(frames, exposures, ref, me.levels, me.search, me.zero_bias, me.white_level)
    pyramids, fields, costs = merge._workspace(len(frames), merge.fields().device)
    ok = True
    for f in range(len(frames)):
        for k in range(me.levels):
            got = me.level(pyramids[f // 2], f % 2, k).cpu().numpy()
            if not np.array_equal(got, want_pyramids[f][k]):
                print(f'{what}: level {k} of frame {f} differs at {np.count_nonzero(got != want_pyramids[f][k])} values')
                ok = False
        if f != ref:
            if not np.array_equal(fields[f].cpu().numpy(), want_fields[f]):
                print(f'{what}: the field of frame {f} differs: {fields[f].cpu().numpy().tolist()} != {want_fields[f].tolist()}')
                ok = False
            if not np.array_equal(costs[f].view(torch.int32).cpu().numpy().view(np.uint32), want_costs[f]):
                print(f'{what}: the costs of frame {f} differ')
                ok = False
    return ok, want_fields


@pytest.mark.parametrize('src', [np.float32, np.float16], ids=['src32', 'src16'])
def test_pyramids_fields_and_costs_with_exposures_on_the_device(td, dev, src):
    """Shutter times that are no whole stops, as a device tensor (ref must then be given); two levels and a small search on a ragged
    size, the defaults on a larger one; special samples in the frames."""
    m = td.NoiseModel(torch.from_numpy(MODEL).to(dev))
    ok = True
    for (w, h), nf, ref, motion in (((130, 66), 3, 1, dict(levels=2, search=2, zero_bias=0)), ((200, 100), 4, 0, dict(levels=4, search=3, zero_bias=40)),
                                     ((256, 192), 8, 5, None)):
        exposures = SHUTTER[nf]
        shifts = [(0, 0) if f == ref else (2 * (f % 3) - 2, 4 - 4 * (f % 2)) for f in range(nf)]
        frames = chart_bracket(w, h, exposures, shifts, seed=nf, dtype=src)
        frames[0][5, 7], frames[1][h - 1, w - 1], frames[nf - 1][h // 2, 3] = np.nan, np.inf, -1.0
        me = None if motion is None else td.MotionEstimate(dev, (w, h), **motion)
        merge = td.MotionHdrMerge(dev, (w, h), td.BayerPattern.RGGB, m, motion=me)
        xs = [plain.upload(x, dev, f % 3) for f, x in enumerate(frames)]
        exp = torch.tensor(exposures, dtype=torch.float32, device=dev)
        got = merge.align(xs, exp, ref=ref)
        torch.cuda.synchronize()
        assert got.data_ptr() == merge.fields().data_ptr() and tuple(got.shape) == (nf, *mspec.tiles(w, h), 2) and tuple(merge.costs().shape) == tuple(got.shape)
        ok = same_alignment(merge, frames, exposures, ref, f'{w}x{h} F={nf}')[0] and ok
    with pytest.raises(ValueError, match='ref=None needs exposures the host holds'):
        merge.align(xs, exp)
    assert ok


# ------------------------------------------------------------------ 3. end to end
def test_a_panned_chart_bracket_end_to_end(td, dev):
    """256 x 192, three frames, every frame but the anchor panned by its own shift: the fields are estimated (2 F launches) and the
    interior tiles give the shifts; out, mask, fields and costs are the restatement's."""
    w, h = 256, 192
    exposures, shifts = (1.0, 0.25, 1 / 16), ((0, 0), (-4, 8), (4, -4))
    frames = chart_bracket(w, h, exposures, shifts, seed=3)
    m = td.NoiseModel(torch.from_numpy(MODEL).to(dev))
    merge = td.MotionHdrMerge(dev, (w, h), td.BayerPattern.RGGB, m)
    xs = [plain.upload(x, dev) for x in frames]
    out, mask = merge.process(xs, exposures, return_mask=True)   # ref=None: the longest exposure, frame 0
    torch.cuda.synchronize()
    ok, fields = same_alignment(merge, frames, exposures, 0, 'end to end')
    want, want_mask, want_fields, _ = spec.process(frames, exposures, MODEL, hspec.RGGB)
    assert np.array_equal(fields, want_fields)
    assert plain.same(out, mask, want, want_mask, 'end to end') and ok
    found = [float((fields[f] == np.array(shifts[f])).all(-1).mean()) for f in (1, 2)]
    print(f'tiles that give the shift of their frame: {found}')   # (the purpose is held on the restatement; no tile of a frame this narrow is interior)
    assert fields[1:].any()
    # the estimated fields given by hand: one launch, the same bits
    again = merge.process(xs, exposures, fields=merge.fields().clone())
    assert torch.equal(again.view(torch.int32), out.view(torch.int32))


def test_a_captured_call_follows_frames_and_exposures_rewritten_in_place(td, dev):
    w, h = 130, 66
    m = td.NoiseModel(torch.from_numpy(MODEL).to(dev))
    merge = td.MotionHdrMerge(dev, (w, h), td.BayerPattern.RGGB, m, motion=td.MotionEstimate(dev, (w, h), levels=2, search=3, zero_bias=50))
    brackets = [((1.0, 0.25, 1 / 16), ((0, 0), (2, -2), (-4, 4))), ((1.0, 0.5, 0.125), ((0, 0), (-2, 6), (0, 0))), ((1 / 30, 1 / 125, 1 / 500), ((0, 0), (4, 4), (-6, -2)))]
    first = chart_bracket(w, h, *brackets[0], seed=0)
    xs = [plain.upload(x, dev) for x in first]
    exp = torch.tensor(brackets[0][0], dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        merge.prepare(3)
        merge.process(xs, exp, ref=0)   # the warm-up
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            out, mask = merge.process(xs, exp, ref=0, return_mask=True)
        torch.cuda.synchronize()
        for n, (exposures, shifts) in enumerate(brackets):
            frames = chart_bracket(w, h, exposures, shifts, seed=10 + n)
            for x, new in zip(xs, frames):
                x.copy_(torch.from_numpy(new))
            exp.copy_(torch.tensor(exposures, dtype=torch.float32))
            graph.replay()
            torch.cuda.synchronize()
            ok, fields = same_alignment(merge, frames, exposures, 0, f'replay {n}')
            want, want_mask = spec.merge(frames, exposures, fields, MODEL, hspec.RGGB, 0)
            assert plain.same(out, mask, want, want_mask, f'replay {n}') and ok
            assert fields[1:].any()   # something moved
        eager, eager_mask = merge.process(xs, exp, ref=0, return_mask=True)   # bit-reproducible
        torch.cuda.synchronize()
    assert torch.equal(eager.view(torch.int32), out.view(torch.int32)) and torch.equal(eager_mask, mask)


# ------------------------------------------------------------------ 4. pipeline
def test_process_bracket_is_the_stages_called_by_hand(td, dev):
    from torch_darktable import tonemap
    from torch_darktable.pipeline.util import lerp

    w, h = 96, 64
    exposures = (1.0, 0.25, 1 / 16)
    payloads = plain._packed_bracket(td, dev, w, h, exposures)
    m = td.NoiseModel.from_values(0.0, 1.6e-5, dev)
    make = lambda: td.MotionHdrMerge(dev, (w, h), td.BayerPattern.RGGB, m)
    piped, c, by_hand = plain._processor(td, dev, w, h, hdr=make()), plain._processor(td, dev, w, h), make()
    bounds = metrics = None
    for step in range(2):
        out = piped.process_bracket(payloads, exposures, 'cam')
        merged = by_hand.process([c.load_bytes(p) for p in payloads], exposures)
        rgb = c._demosaic(td.apply_white_balance(merged, c.white_balance, td.BayerPattern.RGGB)).to(c.storage_dtype)
        now = tonemap.compute_image_bounds([rgb], stride=8)
        bounds = lerp(bounds if bounds is not None else now, now, 0.3)
        acc = tonemap.MetricsAccumulator(dev, stride=8)
        rgb = c.process_rgb(rgb, bounds, acc)
        now = acc.finish()
        metrics = lerp(metrics if metrics is not None else now, now, 0.3)
        assert out.dtype == torch.uint8 and tuple(out.shape) == (h, w, 3) and torch.equal(out, c.tonemap(rgb, metrics)), step
    assert torch.equal(piped.hdr.fields()[1:], by_hand.fields()[1:])   # the stage aligned: its fields are those of the hand-made call
