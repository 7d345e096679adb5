"""GPU: the scene-referred tone mapping (torch_darktable.Filmic, csrc/filmic.hip) gives every bit or byte of the NumPy restatement
tests/filmic_spec.py of include/tdk_hip_filmic.h -- over the norms and storage types, the pixel counts around a lane's group of 16, a
workgroup's step and the grid's stride, offset views, the special samples, the table nodes, the gamut step, streams, graphs that
follow a rewritten exposure and curve, and ImageProcessor.filmic."""

import ctypes

import numpy as np
import pytest
import torch

import filmic_spec as spec

pytestmark = pytest.mark.gpu

SRC = [np.float32, np.float16]
DST = [np.uint8, np.float16, np.float32]
TORCH = {np.float32: torch.float32, np.float16: torch.float16, np.uint8: torch.uint8}
TAG = {np.float32: 0, np.float16: 1, np.uint8: 2}
NORMS = ['max', 'luma', 'power', 'none']
GROUP, WG_STEP = 16, 512 * 16   # pixels of a lane and of a workgroup per step (csrc/filmic.hip: FM_PIX, FM_THREADS)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


samples = spec.samples


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view({4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def same_bits(got, expected, what):
    g, e = bits(got), bits(expected)
    assert g.shape == e.shape, (what, g.shape, e.shape)
    bad = np.argwhere(g != e)
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), g[tuple(bad[0])], e[tuple(bad[0])])


def want(f, x, out_dtype, exposure=1.0, **kw):
    return spec.filmic(x, f.host_curve.numpy(), None if f.host_encode is None else f.host_encode.numpy(), exposure, spec.NORMS[f.norm], f.weights, out_dtype, **kw)


_OBJECTS = {}


def stage(td, dev, kind='filmic', norm='max', encoding='srgb'):
    """One object per configuration for the module; the tests that rewrite exposure or curve build their own."""
    key = (kind, norm, encoding)
    if key not in _OBJECTS:
        if kind == 'vivid':   # all the saturation kept up to white: the gamut step has the most to do
            _OBJECTS[key] = td.Filmic(dev, desaturate=(0.0, 0.0), norm=norm, encoding=encoding)
        else:
            _OBJECTS[key] = {'filmic': td.Filmic, 'sigmoid': td.Filmic.sigmoid}[kind](dev, norm=norm, encoding=encoding)
    return _OBJECTS[key]


def at_offset(t, elements):
    """A contiguous copy of CUDA tensor `t` that starts `elements` elements past an aligned allocation."""
    pool = torch.zeros(t.numel() + elements + 16, dtype=t.dtype, device=t.device)
    assert pool.data_ptr() % 256 == 0
    v = pool[elements:elements + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() == pool.data_ptr() + elements * t.element_size()
    return v


# ------------------------------------------------------------------ 1. norms, storage types, encodings
@pytest.mark.parametrize('src', SRC, ids=['f32', 'f16'])
@pytest.mark.parametrize('norm', NORMS)
def test_every_norm_and_pair_of_types_gives_the_restatements_bits(td, dev, norm, src):
    x = samples(6000 + 7, src, seed=NORMS.index(norm))
    device_x = torch.from_numpy(x).to(dev)
    for kind, encoding in (('filmic', 'srgb'), ('filmic', None), ('sigmoid', 'srgb'), ('vivid', None)):
        f = stage(td, dev, kind, norm, encoding)
        for dst in DST:
            out = f.process(device_x, out_dtype=TORCH[dst])
            assert out.dtype == TORCH[dst] and out.shape == device_x.shape
            same_bits(out, want(f, x, dst), (kind, norm, encoding, src.__name__, dst.__name__))


def test_the_samples_meet_their_cases(td, dev):
    """What the table above is for: the gamut step fires under 'luma' and 'power' and never under 'max', on both sides of y = 1;
    samples sit on nodes, below the first and above the last; the encoding meets its linear part, its last node and values at 1."""
    x = samples(6000 + 7, np.float32, seed=1)
    for norm in ('luma', 'power'):
        f = stage(td, dev, 'vivid', norm, None)
        linear, fires = want(f, x, np.float32, return_fires=True)
        assert fires.sum() > 200, (norm, fires.sum())
        T = f.host_curve.numpy()[0]
        assert T.max() == 1.0   # ... so y >= 1 is met where the norm is at white or above, and y < 1 below it
        assert linear[fires].max() <= 1.0 + 2.0 ** -22 and (linear[fires].max(axis=-1) > 0.99).all()
    _, fires = want(stage(td, dev, 'filmic', 'max', 'srgb'), x, np.float32, return_fires=True)
    assert not fires.any()
    p = x[np.isfinite(x)]
    nodes = spec.nodes().astype(np.float32)
    assert np.isin(p, nodes).sum() >= 30 and (p[p > 0] < spec.XMIN).any() and (p > spec.XMAX).any()
    linear = want(stage(td, dev, 'filmic', 'max', None), x, np.float32)
    assert (linear == 1.0).any() and ((linear > 0) & (linear < spec.ENC_LO)).any()
    assert want(stage(td, dev, 'filmic', 'max', 'srgb'), x, np.uint8).max() == 255


# ------------------------------------------------------------------ 2. pixel counts
@pytest.mark.parametrize('shape', [(1,), (15,), (16,), (17,), (3, 5), (7, 33), (WG_STEP + GROUP + 3,)], ids=str)
def test_pixel_counts_around_a_group_and_a_workgroup_step(td, dev, shape):
    n = int(np.prod(shape))
    for src, dst, norm in ((np.float32, np.uint8, 'max'), (np.float16, np.float16, 'power'), (np.float16, np.float32, 'luma')):
        pool = samples(n + 300, src, seed=n)
        x = np.ascontiguousarray((pool[300:] if n <= 300 else pool[:n]).reshape(*shape, 3))   # small frames take coloured pixels, not only specials
        f = stage(td, dev, 'filmic', norm, 'srgb')
        out = f.process(torch.from_numpy(x).to(dev), out_dtype=TORCH[dst])
        assert out.shape == x.shape
        same_bits(out, want(f, x, dst), (shape, src.__name__, dst.__name__, norm))


def test_more_groups_than_the_grid_covers_in_one_pass(td, dev):
    """The grid is at most three workgroups per compute unit; this frame has more than twice the groups that many lanes take at once, so
    every lane runs its stride loop at least twice.  The stage is pointwise: the frame repeats a block of an odd pixel count, and the
    restatement is computed for the block."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    block = 4099
    reps = (2 * (3 * cus) * WG_STEP) // block + 2
    assert reps * block // GROUP > 2 * (3 * cus) * 512
    x = samples(block, np.float16, seed=5)
    f = stage(td, dev, 'filmic', 'power', 'srgb')
    frame = torch.from_numpy(x).to(dev).repeat(reps, 1)
    assert frame.shape == (reps * block, 3)
    out = f.process(frame)
    assert out.dtype == torch.uint8
    expected = torch.from_numpy(want(f, x, np.uint8)).to(dev)
    assert torch.equal(out.view(reps, block, 3), expected.expand(reps, block, 3))


# ------------------------------------------------------------------ 3. views
@pytest.mark.parametrize('src', SRC, ids=['f32', 'f16'])
def test_offset_and_non_contiguous_views(td, dev, src):
    """Contiguous views at element offsets 1 to 3 on either side are taken: the side that the head cannot align moves element by
    element.  A non-contiguous view is refused."""
    n = 1000 + 5
    x = samples(n, src, seed=9)
    device_x = torch.from_numpy(x).to(dev)
    f = stage(td, dev, 'filmic', 'luma', 'srgb')
    for dst in DST:
        expected = want(f, x, dst)
        for off_src in (0, 1, 2, 3):
            for off_dst in (0, 1, 2, 3):
                view = at_offset(device_x, off_src)
                pool = torch.zeros(3 * n + 32, dtype=TORCH[dst], device=dev)
                out = pool[off_dst:off_dst + 3 * n].view(n, 3)
                assert f.process(view, out_dtype=TORCH[dst], out=out) is out
                same_bits(out, expected, (src.__name__, dst.__name__, off_src, off_dst))
                assert float(pool[:off_dst].float().abs().sum()) == 0 and float(pool[off_dst + 3 * n:].float().abs().sum()) == 0   # nothing written outside
    wide = torch.zeros((66, 140, 3), dtype=TORCH[src], device=dev)
    with pytest.raises(RuntimeError, match='contiguous'):
        f.process(wide[:, :130])
    with pytest.raises(RuntimeError, match='contiguous'):
        f.process(torch.zeros((3, 64), dtype=TORCH[src], device=dev).t())
    with pytest.raises(RuntimeError, match='contiguous'):
        f.process(device_x, out_dtype=torch.float32, out=torch.zeros((n, 6), device=dev)[:, :3])
    with pytest.raises(ValueError, match='three channels'):
        f.process(torch.zeros((66, 130, 1), dtype=TORCH[src], device=dev))
    with pytest.raises(ValueError, match='float32 or float16'):
        f.process(torch.zeros((66, 130, 3), dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match='out must be'):
        f.process(device_x, out=torch.zeros((n, 3), device=dev))
    assert f.process(torch.zeros((0, 3), dtype=TORCH[src], device=dev)).shape == (0, 3)


def test_odd_byte_offsets_through_the_c_entry_point(td, dev):
    from torch_darktable._native import lib

    n = 777
    f = stage(td, dev, 'filmic', 'max', 'srgb')
    weights = (ctypes.c_float * 3)(*f.weights)
    stream = torch.cuda.current_stream().cuda_stream
    for src, element_offset in ((np.float16, 1), (np.float16, 5), (np.float32, 3)):
        x = samples(n, src, seed=11)
        view = at_offset(torch.from_numpy(x).to(dev), element_offset)
        for byte_offset in (1, 3, 5, 15):
            pool = torch.zeros(3 * n + 64, dtype=torch.uint8, device=dev)
            out = pool[byte_offset:byte_offset + 3 * n]
            assert out.data_ptr() % 2 == 1
            rc = lib.tdk_filmic(view.data_ptr(), out.data_ptr(), f.curve_table.data_ptr(), f.encode_table.data_ptr(), f.exposure.data_ptr(), n, TAG[src], 2, 0, weights, 0,
                                stream)
            assert rc == 0, lib.tdk_last_error()
            torch.cuda.synchronize()
            same_bits(out.view(n, 3), want(f, x, np.uint8), (src.__name__, element_offset, byte_offset))
            assert int(pool[:byte_offset].sum()) == 0 and int(pool[byte_offset + 3 * n:].sum()) == 0   # nothing written outside


# ------------------------------------------------------------------ 4. state: exposure, streams, graphs
def test_exposure_is_read_from_device_memory(td, dev):
    x = samples(3000, np.float32, seed=13)
    device_x = torch.from_numpy(x).to(dev)
    f = td.Filmic(dev, norm='power')
    for value in (1.0, 2.5, 0.0, 2.0 ** -6):
        f.set_exposure(value)
        same_bits(f.process(device_x, out_dtype=torch.float32), want(f, x, np.float32, exposure=value), value)
    on_device = torch.tensor([0.18], device=dev) / torch.tensor([0.0461], device=dev)   # computed on the stream; nothing waits for it
    f.set_exposure(on_device)
    same_bits(f.exposure, on_device, 'the tensor')
    same_bits(f.process(device_x), want(f, x, np.uint8, exposure=np.float32(on_device.item())), 'a device tensor')


def test_two_streams(td, dev):
    x = samples(WG_STEP * 3 + 11, np.float16, seed=17)
    device_x = torch.from_numpy(x).to(dev)
    f = stage(td, dev, 'sigmoid', 'luma', 'srgb')
    one = f.process(device_x)
    s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    for s in (s1, s2):
        s.wait_stream(torch.cuda.current_stream())
    outs = []
    for _ in range(3):
        with torch.cuda.stream(s1):
            oa = f.process(device_x)
        with torch.cuda.stream(s2):
            ob = f.process(device_x, out_dtype=torch.float16)
        outs.append((oa, ob))
    torch.cuda.synchronize()
    for oa, ob in outs:
        assert torch.equal(oa, one)
        same_bits(ob, want(f, x, np.float16), 'the second stream')
    same_bits(one, want(f, x, np.uint8), 'two streams')


def test_graph_follows_a_rewritten_exposure_and_curve(td, dev):
    """An object built on the side stream and captured there without a warm-up call (the tables and the exposure exist since
    construction); a replay equals the restatement, and after exposure and curve are rewritten the restatement of the new ones."""
    x = samples(5000, np.float16, seed=19)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        device_x = torch.from_numpy(x).to(dev)
        f = td.Filmic(dev, norm='luma')
        with torch.cuda.graph(graph, stream=stream):
            captured = f.process(device_x)
        graph.replay()
        stream.synchronize()
        first = want(f, x, np.uint8)
        same_bits(captured, first, 'replay')
        f.set_exposure(3.0)
        graph.replay()
        stream.synchronize()
        second = want(f, x, np.uint8, exposure=3.0)
        same_bits(captured, second, 'replay after the exposure was rewritten')
        f.set_curve(contrast=1.2, black_ev=-6.5, desaturate=(0.3, 0.8))
        f.set_exposure(torch.tensor([0.75], device=dev))
        graph.replay()
        stream.synchronize()
        third = want(f, x, np.uint8, exposure=0.75)
        same_bits(captured, third, 'replay after the curve was rewritten')
        same_bits(f.curve_table, f.host_curve, 'the tables on the device')
        f.set_curve(lambda v: v / (1.0 + v))
        graph.replay()
        stream.synchronize()
        same_bits(captured, want(f, x, np.uint8, exposure=0.75), 'replay after a curve of the caller')
    assert not np.array_equal(first, second) and not np.array_equal(second, third)


# ------------------------------------------------------------------ 5. pipeline
def _processor(td, dev, w, h, **kw):
    from torch_darktable.pipeline import Debayer, ImageProcessingSettings, ImageProcessor, ImageTransform, ToneMapper
    settings = ImageProcessingSettings(moving_average=0.3, postprocess=False, enable_denoise=True, enable_bilateral=True, tone_mapping=ToneMapper.reinhard,
                                       debayer=Debayer.bilinear)
    return ImageProcessor((w, h), td.BayerPattern.RGGB, td.PackedFormat.Packed12, settings, dev, (1.9, 1.0, 1.6), transforms=ImageTransform.none, **kw)


@pytest.mark.parametrize('storage', [torch.float32, torch.float16])
def test_pipeline_runs_it_in_place_of_the_tone_mapper(td, dev, storage):
    w, h = 128, 96
    rng = np.random.default_rng(23)
    yy, xx = np.mgrid[0:h, 0:w]
    scene = np.clip(0.05 + 0.9 * (xx / w) * (0.5 + 0.5 * np.sin(yy / 7.0)) + rng.normal(0, 0.01, (h, w)), 0, 1).astype(np.float32)
    packed = {name: td.encode12_float(torch.from_numpy(np.roll(scene, k, axis=1)).to(dev).reshape(-1)) for k, name in enumerate(('left', 'right'))}
    f = td.Filmic(dev, norm='power')
    f.set_exposure(1.7)

    # the processor without the stage, with the frames its tone mapper is given kept
    by_hand = _processor(td, dev, w, h, storage_dtype=storage)
    assert by_hand.filmic is None
    seen, mapper = [], by_hand.tonemap
    by_hand.tonemap = lambda img, metrics=None: (seen.append(img.clone()), mapper(img, metrics))[1]
    never = by_hand.process_image_set(packed)
    assert len(seen) == 2 and seen[0].dtype in (torch.float32, torch.float16)
    expected = [f.process(img) for img in seen]

    with_stage = _processor(td, dev, w, h, storage_dtype=storage)
    with_stage.filmic = f
    assert with_stage.filmic is f
    got = with_stage.process_image_set(packed)
    assert sorted(got) == ['left', 'right']
    for name, frame, source in zip(packed, expected, seen):
        assert got[name].dtype == torch.uint8 and torch.equal(got[name], frame), name
        assert not torch.equal(got[name], never[name])
        same_bits(frame, want(f, source.cpu().numpy(), np.uint8, exposure=1.7), (name, 'the restatement'))
    assert torch.equal(with_stage.bounds, by_hand.bounds) and torch.equal(with_stage.metrics, by_hand.metrics)   # computed as before

    # None: the bytes of the processor that never had one
    with_stage.filmic = None
    cleared = _processor(td, dev, w, h, storage_dtype=storage)
    cleared.filmic = f
    cleared.filmic = None
    again = cleared.process_image_set(packed)
    for name in packed:
        assert torch.equal(again[name], never[name]), name
