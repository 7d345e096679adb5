"""GPU: ImageProcessor with its added stages combined, branch by branch (scene, parameters, table: tests/pipeline_stack.py, held to
what they claim by tests/test_pipeline_stack.py).  Each stage's kernel is held to its restatement in its own test file; this file
holds the composition: which stages run, in which order, on what, with which key, and who converts to the storage type.

1. every branch of load_image -- {temporal} x {raw_correction} x {chromatic} x {highlights} x {RCD, LMMSE} x {float32, float16}, 64
   cases -- against the public operators called one by one in the documented order, two cameras, three calls;
2. the mosaic the demosaic is given with all four raw stages on, and on the bracket path, against the chain of the NumPy
   restatements from the unpacked 12-bit codes: the anchor that depends on no GPU result;
3. every stage that combines on a sequence in one processor, from bytes to the oriented uint8 frames, against the chain by hand;
   bounds and metrics after every call; the settings' own tone mapper and bounds under the same stack; the compressed entry point;
4. process_bracket with the plain and with the motion-aligned merge under the same stack;
5. the witnesses: taking any one stage out changes the result, and swapping any adjacent pair of the order changes the frame.

The by-hand side runs the same kernels on the same inputs with its own instance of every stage (a stage that kept history would
otherwise advance twice), so every comparison is exact: torch.equal on bytes, bit patterns with every NaN as one pattern on floats.

Measured on an MI355X: the slowest test takes 0.54 s (the first one, the sixteen RCD float32 branches: it loads the library), the
full stack in float32 0.21 s, every other under 0.1 s."""

import numpy as np
import pytest
import torch

import pipeline_stack as ps

pytestmark = pytest.mark.gpu

W, H = ps.W, ps.H
RAW_ORDER = ('raw_correction', 'temporal', 'chromatic', 'highlights')    # as load_image documents it; `hdr` stands where `temporal` does


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a visible MI355X'
    return torch.device('cuda', 0)


def tbits(t):
    """The bit patterns of a float tensor, every NaN as one pattern."""
    out = t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).clone()
    out[torch.isnan(t)] = -1
    return out


def same(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return torch.equal(a, b) if not a.dtype.is_floating_point else torch.equal(tbits(a), tbits(b))


def same_as_numpy(t, want, what):
    got = t.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.argwhere(ps.bits(got) != ps.bits(want))
    if len(bad):
        print(f'{what}: {len(bad)} of {want.size} values differ, first at {bad[0]}: got {got[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r}')
    return len(bad) == 0


_uploaded = {}


def upload(dev, frame, padding):
    """The packed payload of a frame of codes on the device; uploaded once and never written."""
    key = (frame.tobytes(), padding)
    if key not in _uploaded:
        _uploaded[key] = torch.from_numpy(ps.payload(frame, padding)).to(dev)
    return _uploaded[key]


def image_set(dev, call, padding):
    return {name: upload(dev, ps.codes(name, call), padding) for name in ps.NAMES}


def bracket(dev, call, padding):
    return [upload(dev, f, padding) for f in ps.bracket_codes(call)]


class Hand:
    """The chain composed by hand from the public operators, with its own instance of every stage named in `on`."""

    def __init__(self, td, dev, on, storage, padding, variant=None):
        from torch_darktable.pipeline import ImageTransform
        self.td, self.dev, self.padding = td, dev, padding
        self.storage = getattr(torch, storage)
        self.kit = {n: ps.stage(td, dev, n, variant) for n in on if n != 'resize_width'}
        s, pattern = ps.settings(), td.BayerPattern[ps.PATTERN]
        self.pattern = pattern
        self.rcd = td.RCD(dev, (W, H), pattern)
        self.post = td.PostProcess(dev, (W, H), pattern, color_smoothing_passes=s.color_smoothing_passes, green_eq_local=False, green_eq_global=True,
                                   green_eq_threshold=s.green_eq_threshold)
        self.plain = ps.processor(td, dev, {}, storage)     # process_rgb and the settings' tone mapper: the reference's stages
        self.resize = td.Resize(dev, (W, H), (ps.RESIZE_WIDTH, ps.RESIZE_WIDTH * H // W)) if 'resize_width' in on else None
        self.gains = torch.tensor(ps.GAINS, dtype=torch.float32, device=dev)
        self.transforms = {n: ImageTransform[t] for n, t in ps.TRANSFORMS.items()}
        self.bounds = self.metrics = None
        self.mapped = None     # the tone-mapped frames of the last call, in front of `look`

    # ---- the raw half
    def body(self, data):
        assert data.numel() == W * H * 3 // 2 + self.padding
        return data[:data.numel() - self.padding] if self.padding else data

    def decode(self, data):
        return self.td.decode12(self.body(data), torch.float32, self.td.PackedFormat.Packed12).view(H, W)

    def prepare(self, data, gains=None):
        return self.kit['raw_correction'].process_packed(self.body(data), self.td.PackedFormat.Packed12, white_balance=gains)

    def balance(self, mosaic):
        if 'highlights' in self.kit:
            return self.kit['highlights'].process(mosaic, self.gains)
        return self.td.apply_white_balance(mosaic, self.gains, self.pattern)

    def demosaic(self, mosaic):
        if 'demosaic' in self.kit:
            rgb = self.kit['demosaic'].process(mosaic.unsqueeze(-1), out_dtype=self.storage)     # the stage converts at its own store
        else:
            rgb = self.rcd.process(mosaic.unsqueeze(-1))
        return self.post.process(rgb).to(self.storage)

    def load(self, data, name, white_balance_by=None, trace=None):
        """load_image: decode | raw_correction -> temporal -> chromatic -> highlights | white balance -> demosaic -> storage type.
        white_balance_by: the table's word for who applies the gains (None: highlights if there, else apply_white_balance);
        trace: a list that receives the mosaic behind every stage."""
        trace = [] if trace is None else trace
        if white_balance_by == 'fused':     # decode + white balance + RCD as one kernel, which writes the storage type itself
            return self.post.process(self.rcd.process_packed(self.body(data), self.gains, self.td.PackedFormat.Packed12, self.storage))
        by_raw = white_balance_by == 'raw_correction'
        mosaic = self.prepare(data, self.gains if by_raw else None) if 'raw_correction' in self.kit else self.decode(data)
        trace.append(mosaic)
        if 'temporal' in self.kit:
            mosaic = self.kit['temporal'].process(mosaic, key=name)
            trace.append(mosaic)
        return self.after_merge(mosaic, trace, balanced=by_raw)

    def load_bracket(self, datas, trace=None):
        trace = [] if trace is None else trace
        mosaics = [self.prepare(d) if 'raw_correction' in self.kit else self.decode(d) for d in datas]
        trace.append(mosaics)
        mosaic = self.kit['hdr'].process(mosaics, ps.EXPOSURES)
        trace.append(mosaic)
        return self.after_merge(mosaic, trace)

    def after_merge(self, mosaic, trace, balanced=False):
        if 'chromatic' in self.kit:
            mosaic = self.kit['chromatic'].correct(mosaic)
            trace.append(mosaic)
        if not balanced:
            mosaic = self.balance(mosaic)
            trace.append(mosaic)
        return self.demosaic(mosaic)

    # ---- the frame half
    def apply(self, name, img):
        stage = self.kit[name]
        if name == 'chroma_denoise' and 'noise_model' in self.kit:
            m = self.kit['noise_model']
            return m.unstabilize(stage.process(m.stabilize(img, gains=self.gains)), gains=self.gains, out_dtype=img.dtype)
        return stage.process(img)

    def frame_stages(self, img, order=ps.FRAME_STAGES):
        for name in order:
            if name in self.kit:
                img = self.apply(name, img)
        return img

    def finish(self, names, frames):
        """_process_frames from the demosaiced frames on: ({name: full size}, {name: resized}), both sharpened and oriented."""
        from torch_darktable import tonemap
        from torch_darktable.pipeline.transform import transform
        from torch_darktable.pipeline.util import lerp
        k = self.kit
        frames = [self.frame_stages(img) for img in frames]
        now = k['exposure'].bounds(frames) if 'exposure' in k else tonemap.compute_image_bounds(frames, stride=8)
        self.bounds = lerp(self.bounds if self.bounds is not None else now, now, ps.MOVING_AVERAGE)
        acc = tonemap.MetricsAccumulator(self.dev, stride=8)
        frames = [self.plain.process_rgb(img, self.bounds, acc) for img in frames]
        now = acc.finish()
        self.metrics = lerp(self.metrics if self.metrics is not None else now, now, ps.MOVING_AVERAGE)
        self.mapped = [k['filmic'].process(img) if 'filmic' in k else self.plain.tonemap(img, self.metrics) for img in frames]
        graded = [k['look'].process(img) for img in self.mapped] if 'look' in k else self.mapped
        out = []
        for scaled in (graded, [self.resize.process(img) for img in graded] if self.resize is not None else graded):
            sharp = [k['sharpen'].process(img) for img in scaled] if 'sharpen' in k else scaled
            out.append({name: transform(img, self.transforms[name]) for name, img in zip(names, sharp)})
        return tuple(out)

    def step(self, datas):
        """One call on an image set."""
        return self.finish(list(datas), [self.load(d, name) for name, d in datas.items()])


def build(td, dev, on, storage, padding, variant=None):
    """The processor with the stages named in `on`."""
    stages = {n: ps.stage(td, dev, n, variant) for n in on if n != 'resize_width'}
    return ps.processor(td, dev, stages, storage, padding, resize_width=ps.RESIZE_WIDTH if 'resize_width' in on else 0)


def oriented(name, resized):
    w, h = (ps.RESIZE_WIDTH, ps.RESIZE_WIDTH * H // W) if resized else (W, H)
    return (w, h, 3) if ps.TRANSFORMS[name] in ('rotate_90', 'rotate_270', 'transpose', 'transverse') else (h, w, 3)


# ------------------------------------------------------------------ 1. every branch of load_image
@pytest.mark.parametrize('storage', ps.STORAGES)
@pytest.mark.parametrize('demosaic', ps.DEMOSAICS)
def test_every_branch_of_load_image_is_the_operators_called_one_by_one(td, dev, demosaic, storage):
    cases = ps.raw_cases(demosaic, storage)
    assert len(cases) == 16
    for case in cases:
        what = (ps.case_id(case), demosaic, storage)
        on = [n for n in ps.RAW_STAGES if getattr(case, n)] + (['demosaic'] if demosaic == 'lmmse' else [])
        proc, hand = build(td, dev, on, storage, case.padding), Hand(td, dev, on, storage, case.padding)
        assert proc.padding == case.padding and (proc.demosaic is not None) == (demosaic == 'lmmse')
        handed = []     # the white_balance the processor gave to raw_correction, call by call
        if case.raw_correction:
            inner = proc.raw_correction.process_packed
            proc.raw_correction.process_packed = lambda *a, white_balance=None, **kw: (handed.append(white_balance), inner(*a, white_balance=white_balance, **kw))[1]
        for call in range(ps.CALLS):
            for name, data in image_set(dev, call, case.padding).items():
                got = proc.load_image(data, name)
                want = hand.load(data, name, case.white_balance_by)
                assert got.dtype == getattr(torch, storage) and tuple(got.shape) == (H, W, 3), what
                assert same(got, want), (*what, name, call)
        if case.raw_correction:     # the table says which side applies the white balance
            assert len(handed) == ps.CALLS * len(ps.NAMES) and all((g is not None) == (case.white_balance_by == 'raw_correction') for g in handed), what
        if case.temporal:           # the image name is the key of the history
            for t in (proc.temporal, hand.kit['temporal']):
                assert [int(t.frames(n).item()) for n in ps.NAMES] == [ps.CALLS] * len(ps.NAMES) and int(t.frames().item()) == 0, what


# ------------------------------------------------------------------ 2. the mosaic in front of the demosaic
def recorded(proc):
    """Wrap `_demosaic`: the list that receives what it is given."""
    seen, inner = [], proc._demosaic
    proc._demosaic = lambda mosaic: (seen.append(mosaic.clone()), inner(mosaic))[1]
    return seen


@pytest.mark.parametrize('demosaic', ps.DEMOSAICS)
def test_the_mosaic_in_front_of_the_demosaic_is_the_chain_of_the_restatements(td, dev, demosaic):
    on = list(RAW_ORDER) + (['demosaic'] if demosaic == 'lmmse' else [])
    proc, hand = build(td, dev, on, 'float32', ps.PADDING), Hand(td, dev, on, 'float32', ps.PADDING)
    assert tuple(np.float32(v) for v in proc.chromatic.center) == ps.geometry()[:2] and np.float32(proc.chromatic.rn) == ps.geometry()[2]
    seen, traces = recorded(proc), []
    for call in range(ps.CALLS):
        for name, data in image_set(dev, call, ps.PADDING).items():
            proc.load_image(data, name)
            traces.append([])
            hand.load(data, name, trace=traces[-1])
    assert len(seen) == ps.CALLS * len(ps.NAMES)
    chains = {name: ps.sequence_chain(name) for name in ps.NAMES}
    n = 0
    for call in range(ps.CALLS):
        for name in ps.NAMES:
            want = chains[name][call]
            # stage by stage first, so that a difference names its stage
            assert len(traces[n]) == len(RAW_ORDER)
            for stage, got, expected in zip(RAW_ORDER, traces[n], want):
                assert same_as_numpy(got, expected, (name, call, 'behind', stage)), (name, call, stage)
            assert seen[n].dtype == torch.float32 and same_as_numpy(seen[n], want[3], (name, call, 'what _demosaic is given')), (name, call)
            n += 1


def test_the_merged_mosaic_in_front_of_the_demosaic_is_the_chain_of_the_restatements(td, dev):
    on = ['raw_correction', 'hdr', 'chromatic', 'highlights', 'demosaic']
    proc, hand = build(td, dev, on, 'float32', ps.PADDING), Hand(td, dev, on, 'float32', ps.PADDING)
    seen = recorded(proc)
    for call in range(ps.BRACKET_CALLS):
        datas, trace = bracket(dev, call, ps.PADDING), []
        proc.load_bracket(datas, ps.EXPOSURES)
        hand.load_bracket(datas, trace)
        frames, merged, corrected, balanced = ps.bracket_chain(call)
        for f, (got, expected) in enumerate(zip(trace[0], frames)):
            assert same_as_numpy(got, expected, (call, 'frame', f, 'behind raw_correction')), (call, f)
        for stage, got, expected in zip(('hdr', 'chromatic', 'highlights'), trace[1:], (merged, corrected, balanced)):
            assert same_as_numpy(got, expected, (call, 'behind', stage)), (call, stage)
        assert same_as_numpy(seen[call], balanced, (call, 'what _demosaic is given')), call
    assert len(seen) == ps.BRACKET_CALLS


# ------------------------------------------------------------------ 3. everything on
@pytest.mark.parametrize('storage', ps.STORAGES)
def test_the_full_stack_from_bytes_to_the_oriented_frame(td, dev, storage):
    on = ps.FULL_STACK
    resized, full, compressed = (build(td, dev, on, storage, ps.PADDING) for _ in range(3))
    hand = Hand(td, dev, on, storage, ps.PADDING)
    # the second processor: the settings' own tone mapper and the minimum and maximum as bounds meet the full stack too
    fewer = tuple(n for n in on if n not in ('filmic', 'exposure'))
    second, second_hand = build(td, dev, fewer, storage, ps.PADDING), Hand(td, dev, fewer, storage, ps.PADDING)
    assert second.filmic is None and second.exposure is None and resized.filmic is not None and resized.exposure is not None
    codec = td.RawCodec(dev, (W, H))
    for call in range(ps.CALLS):
        datas = image_set(dev, call, ps.PADDING)
        got_small, got_full = resized.process_image_set_resized(datas), full.process_image_set(datas)
        streams = {name: codec.encode(d[:d.numel() - ps.PADDING], packed_format=td.PackedFormat.Packed12) for name, d in datas.items()}
        got_compressed = compressed.process_image_set_compressed(streams, codec)
        want_full, want_small = hand.step(datas)
        second_small, (_, second_want) = second.process_image_set_resized(datas), second_hand.step(datas)
        assert list(got_small) == list(got_full) == list(got_compressed) == list(second_small) == list(ps.NAMES)
        for name in ps.NAMES:
            what = (storage, name, call)
            assert got_small[name].dtype == got_full[name].dtype == torch.uint8, what
            assert tuple(got_small[name].shape) == oriented(name, True) and tuple(got_full[name].shape) == oriented(name, False), what
            assert torch.equal(got_full[name], want_full[name]), what
            assert torch.equal(got_small[name], want_small[name]), what
            assert torch.equal(got_compressed[name], got_full[name]) and int(compressed.compressed_status[name].item()) == 0, what
            assert torch.equal(second_small[name], second_want[name]) and not torch.equal(second_small[name], got_small[name]), what
        for p in (resized, full, compressed):
            assert same(p.bounds, hand.bounds) and same(p.metrics, hand.metrics), (storage, call)
        assert same(second.bounds, second_hand.bounds) and same(second.metrics, second_hand.metrics), (storage, call)
        assert not same(second.bounds, hand.bounds)
    for p in (resized, full, compressed, second):     # per-name state
        assert int(p.temporal.frames('left').item()) == int(p.temporal.frames('right').item()) == ps.CALLS and int(p.temporal.frames().item()) == 0


# ------------------------------------------------------------------ 4. the bracket path
@pytest.mark.parametrize('storage', ps.STORAGES)
@pytest.mark.parametrize('variant', ['plain', 'motion'])
def test_process_bracket_under_the_full_stack(td, dev, variant, storage):
    on = ps.BRACKET_STACK
    proc, hand = build(td, dev, on, storage, ps.PADDING, variant), Hand(td, dev, on, storage, ps.PADDING, variant)
    assert type(proc.hdr) is (td.MotionHdrMerge if variant == 'motion' else td.HdrMerge)
    for call in range(ps.BRACKET_CALLS):
        datas = bracket(dev, call, ps.PADDING)
        got = proc.process_bracket(datas, ps.EXPOSURES, 'left')
        want = hand.finish(['left'], [hand.load_bracket(datas)])[0]['left']     # process_bracket does not resize
        assert got.dtype == torch.uint8 and tuple(got.shape) == oriented('left', False) and torch.equal(got, want), (variant, storage, call)
        assert same(proc.bounds, hand.bounds) and same(proc.metrics, hand.metrics), (variant, storage, call)
        if variant == 'motion':     # the stage aligned: its fields are those of the hand-made call
            assert torch.equal(proc.hdr.fields()[1:], hand.kit['hdr'].fields()[1:])
    # `process` of a processor with the stage is what it is without it
    with_hdr, without = build(td, dev, on, storage, ps.PADDING, variant), build(td, dev, [n for n in on if n != 'hdr'], storage, ps.PADDING)
    assert with_hdr.hdr is not None and without.hdr is None
    for call in range(2):
        data = upload(dev, ps.codes('left', call), ps.PADDING)
        assert torch.equal(with_hdr.process(data, 'left'), without.process(data, 'left')), (variant, storage, call)


# ------------------------------------------------------------------ 5. the test can tell
def run(td, dev, on, storage):
    """(the frames of every call, the bounds after the last) of process_image_set_resized."""
    proc = build(td, dev, on, storage, ps.PADDING)
    return [proc.process_image_set_resized(image_set(dev, call, ps.PADDING)) for call in range(ps.CALLS)], proc.bounds


@pytest.mark.parametrize('storage', ps.STORAGES)
def test_taking_any_one_stage_out_changes_the_result(td, dev, storage):
    whole, whole_bounds = run(td, dev, ps.FULL_STACK, storage)
    for name in ps.FULL_STACK:
        # (noise_model is the transform around chroma_denoise: it cannot stay without it)
        on = [n for n in ps.FULL_STACK if n != name and not (name == 'chroma_denoise' and n == 'noise_model')]
        frames, bounds = run(td, dev, on, storage)
        differs = [a[n].shape != b[n].shape or not torch.equal(a[n], b[n]) for a, b in zip(frames, whole) for n in ps.NAMES]
        print(storage, 'without', name, ': frames that differ', sum(differs), 'of', len(differs), 'bounds differ', not same(bounds, whole_bounds))
        assert any(differs), (storage, name)
        if name == 'exposure':
            assert not same(bounds, whole_bounds), storage


@pytest.mark.parametrize('storage', ps.STORAGES)
def test_swapping_an_adjacent_pair_of_the_raw_half_changes_the_frame(td, dev, storage):
    """The second frame of a camera (the first passes through the temporal stage) in the documented order and with each adjacent
    pair swapped.  raw_correction behind temporal is the same correction on the decoded mosaic, its levels in the mosaic's units."""
    on = list(RAW_ORDER) + ['demosaic']

    def second_frame(swapped=None):
        hand = Hand(td, dev, on, storage, 0)
        k = hand.kit
        unit = td.RawPrepare(dev, (W, H), hand.pattern, black=[b / 4095.0 for b in ps.BLACK], white=ps.WHITE / 4095.0, hot=True, dead=True,
                             shading=torch.from_numpy(ps.shading_grid()))
        ops = {'raw_correction': lambda m: unit.process(m), 'temporal': lambda m: k['temporal'].process(m, key='left'),
               'chromatic': k['chromatic'].correct, 'highlights': hand.balance}
        order = list(RAW_ORDER)
        if swapped is not None:
            i = order.index(swapped[0])
            assert order[i + 1] == swapped[1]
            order[i], order[i + 1] = order[i + 1], order[i]
        for call in range(2):
            data = upload(dev, ps.codes('left', call), 0)
            if order[0] == 'raw_correction':
                mosaic, rest = hand.prepare(data), order[1:]
            else:
                mosaic, rest = hand.decode(data), order
            for name in rest:
                mosaic = ops[name](mosaic)
        return hand.demosaic(mosaic)

    documented = second_frame()
    again = Hand(td, dev, on, storage, 0)
    for call in range(2):
        want = again.load(upload(dev, ps.codes('left', call), 0), 'left')
    assert same(documented, want)     # the harness composes what load_image composes
    for pair in zip(RAW_ORDER, RAW_ORDER[1:]):
        assert not same(second_frame(pair), documented), (storage, pair)


@pytest.mark.parametrize('storage', ps.STORAGES)
def test_swapping_an_adjacent_pair_of_the_frame_half_changes_the_frame(td, dev, storage):
    hand = Hand(td, dev, ps.FULL_STACK, storage, ps.PADDING)
    datas = image_set(dev, 0, ps.PADDING)
    loaded = [hand.load(d, name) for name, d in datas.items()]
    documented = [hand.frame_stages(img) for img in loaded]
    order = [n for n in ps.FRAME_STAGES]
    assert all(n in hand.kit for n in order)
    for i in range(len(order) - 1):
        swapped = order[:i] + [order[i + 1], order[i]] + order[i + 2:]
        assert not same(hand.frame_stages(loaded[0], swapped), documented[0]), (storage, order[i], order[i + 1])
    # the bounds are measured behind the last frame stage, not in front of it
    behind, in_front = hand.kit['exposure'].bounds(documented), hand.kit['exposure'].bounds([hand.frame_stages(img, order[:-1]) for img in loaded])
    assert not same(behind, in_front), storage
    # the output half on the tone-mapped bytes: look -> resize -> sharpen
    hand.finish(list(datas), loaded)
    mapped, look, resize, sharpen = hand.mapped[0], hand.kit['look'], hand.resize, hand.kit['sharpen']
    assert mapped.dtype == torch.uint8
    assert not torch.equal(look.process(resize.process(mapped)), resize.process(look.process(mapped))), storage
    graded = look.process(mapped)
    assert not torch.equal(resize.process(sharpen.process(graded)), sharpen.process(resize.process(graded))), storage
