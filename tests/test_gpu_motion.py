"""GPU: the motion block (torch_darktable.MotionEstimate, torch_darktable.MotionTemporalDenoise, include/tdk_hip_motion.h) against the
NumPy restatement of the specification, tests/motion_spec.py (held to literal loops and to the block's purpose in
tests/test_motion_spec.py).

Every comparison is to the bit: the levels of the pyramid, the field, the costs, the output, both planes of the state a step wrote
and the frame index.  There is no tolerance anywhere in this file.  Frames are sized by the tile (64 x 32 sites): one cell, exactly one
tile, two-site tail tiles, several tiles with tails, rows that are no multiple of four sites (the per-element path alternates)."""
import numpy as np
import pytest
import torch

import motion_spec as spec
import temporal_spec as tspec

pytestmark = pytest.mark.gpu

F = np.float32
PATTERNS = {'RGGB': tspec.RGGB, 'BGGR': tspec.BGGR, 'GRBG': tspec.GRBG, 'GBRG': tspec.GBRG}
TORCH = {np.float32: torch.float32, np.float16: torch.float16}
MODEL = np.array([[3e-4, 2e-6, 1, 20], [2e-4, 1e-6, 1, 20], [5e-4, 3e-6, 1, 20]], F)
GAINS = np.array([2.0, 1.0, 1.5], F)
SIZES = [(2, 2), (64, 32), (66, 34), (130, 70), (198, 150), (258, 98)]   # (width, height)
IDS = [f'{w}x{h}' for w, h in SIZES]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a visible MI355X'
    return torch.device('cuda', 0)


def upload(a, dev, offset=0):
    """A contiguous device tensor with the contents of `a` that starts `offset` elements behind an allocation's first byte."""
    flat = np.ascontiguousarray(a).reshape(-1)
    buf = torch.empty(flat.size + offset, dtype=torch.from_numpy(flat[:1]).dtype, device=dev)
    buf[offset:].copy_(torch.from_numpy(flat))
    return buf[offset:].view(a.shape)


def bits(a):
    """The bit patterns, with every NaN as one pattern: which NaN an operation returns is not part of the specification."""
    a = np.asarray(a)
    out = a.view(np.int32 if a.dtype == np.float32 else np.int16).copy()
    out[np.isnan(a)] = -1
    return out


def texture(h, w, seed=0, pad=96):
    """A scene with structure in both directions, `pad` sites larger than the frame on every side, in 0.05 .. 0.9."""
    rng = np.random.default_rng(seed)
    base = rng.random((h + 2 * pad + 8, w + 2 * pad + 8))
    smooth = sum(np.roll(base, (a, b), (0, 1)) for a in range(6) for b in range(6)) / 36
    smooth = (smooth - smooth.min()) / (smooth.max() - smooth.min())
    return (0.05 + 0.85 * smooth)[:h + 2 * pad, :w + 2 * pad]


def view(scene, h, w, oy=0, ox=0, pad=96):
    return scene[pad + oy:pad + oy + h, pad + ox:pad + ox + w]


def noisy(rng, clean, dtype=np.float32):
    return (clean + rng.normal(0.0, 1.0, clean.shape) * np.sqrt(3e-4 * clean + 2e-6)).astype(dtype)


def special(frame, rng):
    """A NaN, both infinities, a negative, a zero and a 65504 site: cells with a NaN, an infinite and a negative sum."""
    flat = frame.reshape(-1)
    values = np.array([np.nan, np.inf, -np.inf, -0.25, 0.0, 65504.0], frame.dtype)
    at = rng.choice(flat.size, size=min(flat.size, values.size), replace=False)
    flat[at] = values[:at.size]
    return frame


def same(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        print(f'{what}: {got.dtype} {got.shape}, want {want.dtype} {want.shape}')
        return False
    g, w = (bits(got), bits(want)) if got.dtype.kind == 'f' else (got, want)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        print(f'{what}: differs at {len(bad)} places, first {[tuple(int(v) for v in b) for b in bad[:6]]}: got {[got[tuple(b)] for b in bad[:6]]}, want {[want[tuple(b)] for b in bad[:6]]}')
        return False
    return True


def same_pyramid(me, pyramid, slot, planes, what):
    torch.cuda.synchronize()
    return all([same(f'{what} slot {slot} level {k}', me.level(pyramid, slot, k).cpu().numpy(), planes[k]) for k in range(me.levels)])


def same_state(t, key, out, want, state, what):
    """The output, the two planes the step wrote and the index word against the restatement."""
    torch.cuda.synchronize()
    acc, cnt = t.state(key)
    want_acc, want_cnt = state.next_read()
    ok = all([same(f'{what}: out', out.cpu().numpy(), want), same(f'{what}: acc', acc.cpu().numpy(), want_acc), same(f'{what}: cnt', cnt.cpu().numpy(), want_cnt)])
    idx = int(t.frames(key).item())
    if idx != state.idx:
        print(f'{what}: index {idx}, want {state.idx}')
        ok = False
    return ok


# ------------------------------------------------------------------ 1. pyramid and match
def estimate_case(td, dev, w, h, cur, ref, what, levels=3, search=4, zero_bias=20, white_level=1.0, offset=0):
    """Both pyramids (cur into slot 0, ref into slot 1 of a buffer filled with 0xAB), the field and the costs against the restatement."""
    me = td.MotionEstimate(dev, (w, h), levels=levels, search=search, zero_bias=zero_bias, white_level=white_level)
    pyramid = me.new_pyramid(dev).fill_(0xAB)
    field, costs = me.new_field(dev)
    me.build_pyramid(upload(cur, dev, offset), pyramid, 0)
    me.build_pyramid(upload(ref, dev, offset), pyramid, 1)
    me.match(pyramid, 0, pyramid, 1, field, costs)
    scale = spec.scale_of(white_level)
    pc, pr = spec.pyramid(cur, scale, levels), spec.pyramid(ref, scale, levels)
    want_field, want_costs = spec.match(pc, pr, w, h, search, zero_bias)
    ok = same_pyramid(me, pyramid, 0, pc, what) and same_pyramid(me, pyramid, 1, pr, what)
    ok = same(f'{what}: field', field.cpu().numpy(), want_field) and ok
    ok = same(f'{what}: costs', costs.cpu().numpy(), want_costs) and ok
    # the bytes between a level and the next multiple of 16 are never written
    at, total = me.level_offsets()
    raw = pyramid.cpu().numpy()
    for slot in (0, 1):
        for k, (lh, lw) in enumerate(me.level_sizes()):
            end = slot * total + (at[k + 1] if k + 1 < levels else total)
            ok = bool((raw[slot * total + at[k] + lh * lw:end] == 0xAB).all()) and ok
    return ok, want_field


@pytest.mark.parametrize('size', SIZES, ids=IDS)
@pytest.mark.parametrize('dtype', [np.float32, np.float16], ids=['src32', 'src16'])
def test_pyramid_field_and_costs_of_a_shifted_scene(td, dev, size, dtype):
    w, h = size
    scene = texture(h, w, seed=w + h)
    rng = np.random.default_rng(w * h)
    moved = 0
    for shift, offset in (((2, -4), 0), ((-6, 10), 1), ((0, 0), 0)):
        cur, ref = noisy(rng, view(scene, h, w), dtype), noisy(rng, view(scene, h, w, -shift[0], -shift[1]), dtype)   # ref[p + shift] ~ cur[p]
        ok, field = estimate_case(td, dev, w, h, cur, ref, f'{w}x{h} shift {shift}', offset=offset)
        assert ok
        moved += int((field != 0).any())
    if w >= 130:
        assert moved >= 2   # the shifted pairs gave displacements: the comparison above was not one of zeros


def test_every_levels_and_search(td, dev):
    w, h = 130, 70
    scene = texture(h, w, seed=3)
    rng = np.random.default_rng(5)
    for levels in (1, 2, 3, 4):
        for search in (1, 2, 3, 4):
            d = spec.max_displacement(levels, search)
            shift = (min(d, 8), -min(d, 20))
            cur, ref = noisy(rng, view(scene, h, w)), noisy(rng, view(scene, h, w, -shift[0], -shift[1]))
            ok, _ = estimate_case(td, dev, w, h, cur, ref, f'levels {levels} search {search}', levels=levels, search=search, zero_bias=0)
            assert ok


def test_shifts_beyond_the_search_range_flat_frames_and_special_cells(td, dev):
    w, h = 198, 150
    scene = texture(h, w, seed=9)
    rng = np.random.default_rng(11)
    cur = noisy(rng, view(scene, h, w))
    for shift in ((60, -70), (-96, 96)):   # beyond 38: whatever wins, it is what the restatement says, and within the range
        ok, field = estimate_case(td, dev, w, h, cur, noisy(rng, view(scene, h, w, -shift[0], -shift[1])), f'shift {shift}', zero_bias=0)
        assert ok and np.abs(field).max() <= 38
    for value in (0.0, 0.3, 1.0, 7.0):
        flat = np.full((h, w), value, F)
        ok, field = estimate_case(td, dev, w, h, flat, flat.copy(), f'flat {value}', zero_bias=0)
        assert ok and not field.any()
    ok, _ = estimate_case(td, dev, w, h, cur, np.full((h, w), 0.2, F), 'textured against flat', zero_bias=300)
    assert ok
    for dtype, white in ((np.float32, 1.0), (np.float16, 0.5), (np.float32, 4095.0)):
        a, b = special(noisy(rng, view(scene, h, w), dtype), rng), special(noisy(rng, view(scene, h, w, -2, 4), dtype), rng)
        if white == 4095.0:
            a, b = a * F(4095.0), b * F(4095.0)
        ok, _ = estimate_case(td, dev, w, h, a, b, f'special cells {dtype.__name__} white {white}', white_level=white, offset=1)
        assert ok


def test_slots_follow_the_index_and_no_history_gives_zeros(td, dev):
    w, h = 130, 70
    scene = texture(h, w, seed=13)
    rng = np.random.default_rng(17)
    cur, ref = noisy(rng, view(scene, h, w)), noisy(rng, view(scene, h, w, -4, 6))
    me = td.MotionEstimate(dev, (w, h), zero_bias=10)
    pc, pr = spec.pyramid(cur), spec.pyramid(ref)
    want_field, want_costs = spec.match(pc, pr, w, h, zero_bias=10)
    assert want_field.any()
    x_cur, x_ref = upload(cur, dev), upload(ref, dev)
    index = torch.zeros(4, dtype=torch.int32, device=dev)
    for idx in (0, 1, 2, 5, 0xFFFFFFFF):
        index[0] = idx - (1 << 32) if idx >= 1 << 31 else idx
        for which in (0, 1):
            pyramid = me.new_pyramid(dev).fill_(0xCD)
            field, costs = me.new_field(dev)
            field.fill_(77), costs.view(torch.int32).fill_(77)
            me.build_pyramid(x_cur, pyramid, which, index=index)
            slot = (idx + which) & 1
            assert same_pyramid(me, pyramid, slot, pc, f'idx {idx} which {which}')
            other = me.level_offsets()[1] * (slot ^ 1)
            assert bool((pyramid[other:other + me.level_offsets()[1]] == 0xCD).all())   # the other slot is not touched
            me.build_pyramid(x_ref, pyramid, which ^ 1, index=index)
            assert same_pyramid(me, pyramid, slot ^ 1, pr, f'idx {idx} which {which ^ 1}') and same_pyramid(me, pyramid, slot, pc, 'kept')
            me.match(pyramid, which, pyramid, which ^ 1, field, costs, index=index)
            torch.cuda.synchronize()
            if idx == 0:
                assert not field.cpu().numpy().any() and not costs.cpu().numpy().any()
            else:
                assert same('field', field.cpu().numpy(), want_field) and same('costs', costs.cpu().numpy(), want_costs)
            # without an index the slots are taken as given, and costs are optional
            field.fill_(77)
            me.match(pyramid, slot, pyramid, slot ^ 1, field, None)
            assert same('field without index', field.cpu().numpy(), want_field)
    # two buffers, and the roles exchanged: the displacement of ref against cur
    p0, p1 = me.new_pyramid(dev), me.new_pyramid(dev)
    field, costs = me.new_field(dev)
    me.build_pyramid(x_cur, p0, 1)
    me.build_pyramid(x_ref, p1, 0)
    me.match(p1, 0, p0, 1, field, costs)
    back = spec.match(pr, pc, w, h, zero_bias=10)
    assert same('exchanged field', field.cpu().numpy(), back[0]) and same('exchanged costs', costs.cpu().numpy(), back[1])
    got = me.estimate(x_cur, x_ref, return_costs=True)
    assert same('estimate field', got[0].cpu().numpy(), want_field) and same('estimate costs', got[1].cpu().numpy(), want_costs)
    assert same('estimate', me.estimate(x_cur, x_ref).cpu().numpy(), want_field)


# ------------------------------------------------------------------ 2. the compensated filter under given fields
def filter_frames(h, w, dtype=np.float32, seed=0, count=5):
    """A ramp with signal-dependent noise; the fourth frame has a rectangle moved in and special values."""
    rng = np.random.default_rng(1000 * h + w + seed)
    yy, xx = np.mgrid[0:h, 0:w]
    clean = 0.05 + 0.8 * (xx / max(w - 1, 1)) * (0.4 + 0.6 * yy / max(h - 1, 1))
    frames = []
    for f in range(count):
        scene = clean.copy()
        if f == 3:
            scene[h // 4:h // 4 + max(h // 3, 1), w // 3:w // 3 + max(w // 4, 1)] += 0.3
        x = noisy(rng, scene, dtype)
        frames.append(special(x, rng) if f == 3 else x)
    return frames


def run_fields(td, dev, w, h, fields, what, pattern='RGGB', src=np.float32, state=np.float32, out=None, gains=None, radius=2, offset=0, plain=False, seed=0):
    """tdk_motion_temporal_denoise under the given field of every frame against the restatement, compared after every step; with
    `plain` (zero fields) also against tdk_temporal_denoise on a second state."""
    from torch_darktable._native import check, lib
    from torch_darktable.torch_darktable_extension import _ptr, _stream

    m = td.NoiseModel(torch.from_numpy(MODEL).to(dev))
    t = td.MotionTemporalDenoise(dev, (w, h), td.BayerPattern[pattern], m, radius=radius, state_dtype=TORCH[state])
    t._states[None].fill_(0xFF)   # nothing may depend on what the planes hold before the first frame
    t.reset()
    t2 = td.TemporalDenoise(dev, (w, h), td.BayerPattern[pattern], m, radius=radius, state_dtype=TORCH[state])
    g = None if gains is None else torch.from_numpy(gains).to(dev)
    ref = tspec.State((h, w), state)
    out_np = src if out is None else out
    tag = {np.float32: 0, np.float16: 1}
    ok = True
    for f, (frame, field) in enumerate(zip(filter_frames(h, w, src, seed, len(fields)), fields)):
        x = upload(frame, dev, offset)
        y = torch.empty((h, w), dtype=TORCH[out_np], device=dev)
        fd = torch.from_numpy(np.ascontiguousarray(field, np.int16)).to(dev)
        check(lib.tdk_motion_temporal_denoise(_ptr(x), tag[src], _ptr(y), tag[out_np], _ptr(t._states[None]), tag[state], w, h, PATTERNS[pattern], _ptr(m.model),
                                              _ptr(g), radius, 1.5, 3.0, 16.0, 8.0, 1e-12, _ptr(fd), _stream()))
        want = spec.compensated_step(frame, ref, field, MODEL, PATTERNS[pattern], gains=gains, radius=radius, out_dtype=out_np)
        ok = same_state(t, None, y, want, ref, f'{what} {w}x{h} frame {f + 1}') and ok
        if plain:
            y2 = t2.process(x, gains=g, out_dtype=TORCH[out_np])
            torch.cuda.synchronize()
            ok = same(f'{what} frame {f + 1}: the plain filter', y2.cpu().numpy(), want) and ok
            for a, b in zip(t.state(), t2.state()):
                ok = torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int16), b.view(torch.int32 if b.dtype == torch.float32 else torch.int16)) and ok
            ok = int(t2.frames().item()) == ref.idx and ok
    return ok


def random_field(rng, w, h, limit=78):
    ny, nx = spec.tiles(w, h)
    return (2 * rng.integers(-limit // 2, limit // 2 + 1, (ny, nx, 2))).astype(np.int16)


@pytest.mark.parametrize('size', SIZES, ids=IDS)
@pytest.mark.parametrize('radius', [2, 3])
def test_a_zero_field_is_the_plain_filter(td, dev, size, radius):
    w, h = size
    zero = np.zeros((*spec.tiles(w, h), 2), np.int16)
    for offset in (0, 1):
        assert run_fields(td, dev, w, h, [zero] * 5, f'zero field radius {radius} offset {offset}', radius=radius, offset=offset, plain=True)


@pytest.mark.parametrize('size', SIZES, ids=IDS)
@pytest.mark.parametrize('radius', [2, 3])
def test_random_even_displacements_per_tile(td, dev, size, radius):
    w, h = size
    rng = np.random.default_rng(w + 7 * h + radius)
    near, far = [random_field(rng, w, h, 8) for _ in range(5)], [random_field(rng, w, h) for _ in range(5)]
    assert run_fields(td, dev, w, h, near, f'displacements up to 8, radius {radius}', radius=radius, gains=GAINS)
    assert run_fields(td, dev, w, h, far, f'displacements up to 78, radius {radius}', radius=radius, offset=1)


@pytest.mark.parametrize('src', [np.float32, np.float16], ids=['src32', 'src16'])
@pytest.mark.parametrize('state', [np.float32, np.float16], ids=['state32', 'state16'])
@pytest.mark.parametrize('out', [np.float32, np.float16], ids=['out32', 'out16'])
def test_every_combination_of_storage_types(td, dev, src, state, out):
    w, h = 198, 150
    rng = np.random.default_rng(23)
    for radius, offset in ((2, 1), (3, 0)):
        fields = [random_field(rng, w, h, 12) for _ in range(4)]
        assert run_fields(td, dev, w, h, fields, f'{src.__name__}/{state.__name__}/{out.__name__}', 'GRBG', src=src, state=state, out=out, radius=radius, offset=offset)


@pytest.mark.parametrize('pattern', list(PATTERNS))
def test_every_pattern(td, dev, pattern):
    w, h = 130, 70
    rng = np.random.default_rng(29)
    for radius in (2, 3):
        assert run_fields(td, dev, w, h, [random_field(rng, w, h, 10) for _ in range(4)], pattern, pattern, gains=GAINS, radius=radius)


def test_fields_that_point_outside_the_frame_odd_values_and_the_largest_int16(td, dev):
    w, h = 198, 150
    ny, nx = spec.tiles(w, h)
    uniform = lambda dy, dx: np.broadcast_to(np.array([dy, dx], np.int16), (ny, nx, 2)).copy()
    rng = np.random.default_rng(31)
    for radius in (2, 3):
        # every side: part of the frame keeps its history, the rest restarts
        sides = [uniform(0, 0), uniform(-40, 0), uniform(40, 0), uniform(0, -70), uniform(0, 70), uniform(-78, 78)]
        assert run_fields(td, dev, w, h, sides, f'outside on every side, radius {radius}', radius=radius)
        # whole frame outside, in rows, in columns, and the ends of int16: nothing is read
        gone = [uniform(0, 0), uniform(150, 0), uniform(0, -198), uniform(32767, 32767), uniform(-32768, -32768), uniform(32767, -32768), uniform(-2, 2)]
        assert run_fields(td, dev, w, h, gone, f'nothing inside, radius {radius}', radius=radius, state=np.float16, offset=1)
        # odd values are masked: 3 -> 2, -3 -> -4, 1 -> 0, -1 -> -2
        odd = [uniform(0, 0), uniform(3, -3), uniform(1, 1), uniform(-1, 5), (random_field(rng, w, h, 20) + 1).astype(np.int16)]
        assert run_fields(td, dev, w, h, odd, f'odd values, radius {radius}', radius=radius)


# ------------------------------------------------------------------ 3. end to end
def pan_frames(h, w, step, dtype=np.float32, seed=0, count=5):
    scene = texture(h, w, seed=seed)
    rng = np.random.default_rng(seed + 1)
    return [noisy(rng, view(scene, h, w, f * step[0], f * step[1]), dtype) for f in range(count)]


def same_sequence_step(mt, key, got, want, seq, what):
    """Everything a call of process leaves behind: output, state, index, field, costs, and the pyramid slot of this frame."""
    ok = same_state(mt, key, got, want, seq.state, what)
    ok = same(f'{what}: field', mt.field(key).cpu().numpy(), seq.field) and ok
    ok = same(f'{what}: costs', mt.costs(key).cpu().numpy(), seq.costs) and ok
    wrote = (seq.state.idx - 1) & 1   # the index the call saw (no wrap in these sequences)
    return same_pyramid(mt.motion, mt._buffers[key][0], wrote, seq.slots[wrote], what) and ok


@pytest.mark.parametrize('size', SIZES, ids=IDS)
def test_a_pan_through_process(td, dev, size):
    w, h = size
    m = td.NoiseModel(torch.from_numpy(MODEL).to(dev))
    moved = 0
    for step, radius, dtype, state in (((2, -4), 2, np.float32, np.float32), ((-6, 2), 3, np.float16, np.float16)):
        me = td.MotionEstimate(dev, (w, h), zero_bias=30)
        mt = td.MotionTemporalDenoise(dev, (w, h), td.BayerPattern.RGGB, m, motion=me, radius=radius, state_dtype=TORCH[state])
        seq = spec.Sequence((h, w), state, zero_bias=30)
        for f, frame in enumerate(pan_frames(h, w, step, dtype, seed=w + h)):
            if f == 4:   # after a reset the first frame passes through and the field is zero again
                mt.reset()
                seq.state.reset()
            got = mt.process(upload(frame, dev, f & 1))
            want = seq.step(frame, MODEL, tspec.RGGB, radius=radius)
            assert same_sequence_step(mt, None, got, want, seq, f'pan {step} {w}x{h} frame {f + 1}')
            if f in (0, 4):
                assert not seq.field.any() and np.array_equal(bits(got.cpu().numpy()), bits(frame))
            moved += int(seq.field.any())
    if w >= 130:
        assert moved >= 4   # the pans were seen


def test_default_parameters_gains_and_two_keys(td, dev):
    w, h = 258, 98
    m = td.NoiseModel(torch.from_numpy(MODEL).to(dev))
    mt = td.MotionTemporalDenoise(dev, (w, h), td.BayerPattern.GBRG, m)   # a default estimator: levels 3, search 4, bias 300
    assert (mt.motion.levels, mt.motion.search, mt.motion.zero_bias) == (3, 4, 300)
    mt.prepare(['left', 'right'])
    assert len({b[0].data_ptr() for b in mt._buffers.values()}) == 3 and len({s.data_ptr() for s in mt._states.values()}) == 3
    g = torch.from_numpy(GAINS).to(dev)
    frames = {'left': pan_frames(h, w, (4, 8), seed=1), 'right': pan_frames(h, w, (-2, -6), seed=2)}
    seqs = {k: spec.Sequence((h, w), zero_bias=300) for k in frames}
    for f in range(5):
        for key in (('left', 'right') if f != 2 else ('right',)):   # 'left' misses a frame: the parities of the two keys differ from then on
            got = mt.process(upload(frames[key][f], dev), key=key, gains=g, out_dtype=torch.float16)
            want = seqs[key].step(frames[key][f], MODEL, tspec.GBRG, gains=GAINS, out_dtype=np.float16)
            assert same_sequence_step(mt, key, got, want, seqs[key], f'{key} frame {f + 1}')
    assert seqs['right'].field.any() and int(mt.frames().item()) == 0


def test_a_captured_call_replays_on_refreshed_input(td, dev):
    w, h = 130, 70
    m = td.NoiseModel(torch.from_numpy(MODEL).to(dev))
    mt = td.MotionTemporalDenoise(dev, (w, h), td.BayerPattern.RGGB, m, motion=td.MotionEstimate(dev, (w, h), zero_bias=30))
    mt.prepare(['graph', 'eager'])   # ahead of the capture: the captured call allocates nothing but its result
    frames = pan_frames(h, w, (2, -4), seed=5, count=4)
    x = upload(frames[0], dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            out = mt.process(x, key='graph')
    torch.cuda.synchronize()
    assert int(mt.frames('graph').item()) == 0   # a capture runs nothing
    replayed, fields = [], []
    for frame in frames[:3]:
        x.copy_(torch.from_numpy(frame))
        graph.replay()
        replayed.append(out.clone())
        fields.append(mt.field('graph').clone())
    torch.cuda.synchronize()
    seq = spec.Sequence((h, w), zero_bias=30)
    for f, frame in enumerate(frames[:3]):
        eager = mt.process(upload(frame, dev), key='eager')
        want = seq.step(frame, MODEL, tspec.RGGB)
        assert torch.equal(replayed[f].view(torch.int32), eager.view(torch.int32)), f
        assert same(f'replay {f + 1}: out', eager.cpu().numpy(), want) and same(f'replay {f + 1}: field', fields[f].cpu().numpy(), seq.field)
    assert seq.field.any()
    assert same_sequence_step(mt, 'graph', replayed[2], want, seq, 'graph') and same_sequence_step(mt, 'eager', eager, want, seq, 'eager')


def test_pipeline_with_a_compensated_denoiser_is_the_stages_called_by_hand(td, dev):
    from torch_darktable import tonemap
    from torch_darktable.pipeline import ImageProcessingSettings, ImageProcessor, ImageTransform, ToneMapper
    from torch_darktable.pipeline.util import lerp
    w, h = 192, 128
    settings = ImageProcessingSettings(moving_average=0.3, postprocess=False, enable_denoise=True, enable_bilateral=True, tone_mapping=ToneMapper.reinhard)
    processor = lambda **kw: ImageProcessor((w, h), td.BayerPattern.RGGB, td.PackedFormat.Packed12, settings, dev, (1.4, 1.0, 1.3), transforms=ImageTransform.none, **kw)
    big = torch.from_numpy(texture(h + 16, w + 16, seed=104, pad=0)).float()
    gen = torch.Generator(device='cpu').manual_seed(7)
    packed = []
    for f in range(3):   # the scene pans by (2, 4) sites per frame
        clean = big[8 + 2 * f:8 + 2 * f + h, 8 + 4 * f:8 + 4 * f + w]
        packed.append(td.encode12_float((clean + 0.004 * torch.randn(clean.shape, generator=gen)).clamp(0.0, 1.0).to(dev).reshape(-1)))
    m = td.NoiseModel.from_values(0.0, 1.6e-5, dev)
    make = lambda: td.MotionTemporalDenoise(dev, (w, h), td.BayerPattern.RGGB, m, max_frames=8.0)
    piped, plain, c, by_hand = processor(temporal=make()), processor(), processor(), make()
    bounds = metrics = None
    for f, raw in enumerate(packed):
        out = piped.process(raw, 'cam')
        mosaic = by_hand.process(c.load_bytes(raw), key='cam')
        rgb = c._demosaic(td.apply_white_balance(mosaic, c.white_balance, td.BayerPattern.RGGB)).to(c.storage_dtype)
        now = tonemap.compute_image_bounds([rgb], stride=8)
        bounds = lerp(bounds if bounds is not None else now, now, 0.3)
        acc = tonemap.MetricsAccumulator(dev, stride=8)
        rgb = c.process_rgb(rgb, bounds, acc)
        now = acc.finish()
        metrics = lerp(metrics if metrics is not None else now, now, 0.3)
        assert torch.equal(out, c.tonemap(rgb, metrics)), f
        assert torch.equal(out, plain.process(raw, 'cam')) == (f == 0)   # the first frame passes through; the later ones are averaged
    assert torch.equal(piped.temporal.field('cam'), by_hand.field('cam')) and int(piped.temporal.frames('cam').item()) == 3
    assert (piped.temporal.field('cam').cpu() == torch.tensor([2, 4], dtype=torch.int16)).all()   # the pan was found ...
    assert float((piped.temporal.state('cam')[1] > 1).float().mean()) > 0.8                          # ... and the history followed it
