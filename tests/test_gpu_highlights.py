"""GPU: the highlight stage (include/tdk_hip_highlights.h, csrc/highlights.hip, torch_darktable.Highlights) against
`highlights_ref`, the float32 restatement of the specification in tests/test_highlights_spec.py, on that module's cases.  Every
comparison is on the raw bits, of the frame and of the integer statistics: no tolerance anywhere."""

import functools
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location('highlights_spec', Path(__file__).resolve().parent / 'test_highlights_spec.py')
spec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(spec)
highlights_ref, CASES, GAINS, PATTERNS, bits = spec.highlights_ref, spec.CASES, spec.GAINS, spec.PATTERNS, spec.bits

DTYPES = [np.float32, np.float16]
TORCH = {np.float32: torch.float32, np.float16: torch.float16}
FRAMES = ['2x2', '4x6', '130x18', '258x34', '200x50', 'low0', 'none']


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a visible MI355X'
    return torch.device('cuda', 0)


@functools.lru_cache(maxsize=None)
def want(name, pattern, gains, in_dtype, out_dtype, mode='opposed'):
    """The restatement of one case, computed once and shared."""
    L, kw = CASES[name]
    return highlights_ref(L.astype(in_dtype), GAINS[gains], PATTERNS[pattern], mode=mode, out_dtype=out_dtype, **kw)


def make(td, dev, name, pattern, mode='opposed'):
    L, kw = CASES[name]
    return td.Highlights(dev, L.shape[::-1], getattr(td.BayerPattern, pattern), mode=mode, **kw)


def at_offset(t, elements):
    """A contiguous copy of CUDA tensor `t` that starts `elements` elements past an aligned allocation."""
    pool = torch.zeros(t.numel() + elements + 16, dtype=t.dtype, device=t.device)
    assert pool.data_ptr() % 256 == 0
    v = pool[elements:elements + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() == pool.data_ptr() + elements * t.element_size()
    return v


def same_bits(got, expected, what):
    got = got.cpu().numpy()
    assert got.dtype == expected.dtype and got.shape == expected.shape, (what, got.dtype, expected.dtype, got.shape, expected.shape)
    bad = np.argwhere(bits(got) != bits(expected))
    if len(bad):
        print(f'{what}: {len(bad)} of {expected.size} values differ, first at {bad[0]}: got {got[tuple(bad[0])]!r} want {expected[tuple(bad[0])]!r}')
    assert len(bad) == 0, what


def source(dev, name, in_dtype, offset=0):
    src = torch.from_numpy(CASES[name][0].astype(in_dtype)).to(dev)
    return at_offset(src, offset) if offset else src


# ------------------------------------------------------------------ 1. the bits of every case
@pytest.mark.parametrize('out_dtype', DTYPES)
@pytest.mark.parametrize('in_dtype', DTYPES)
@pytest.mark.parametrize('pattern', sorted(PATTERNS))
def test_opposed_gives_the_restatements_bits_and_integers(td, dev, pattern, in_dtype, out_dtype):
    for name in FRAMES:
        for gains in GAINS:
            what = (name, pattern, gains, in_dtype.__name__, out_dtype.__name__)
            out_w, sum_w, cnt_w, chroma_w = want(name, pattern, gains, in_dtype, out_dtype)
            h = make(td, dev, name, pattern)
            src = source(dev, name, in_dtype)
            out = h.process(src, GAINS[gains], out_dtype=TORCH[out_dtype])
            assert out.is_contiguous() and out.data_ptr() != src.data_ptr()
            total, cnt = h.statistics(src, GAINS[gains])
            assert total.dtype == torch.int64 and cnt.dtype == torch.int64
            print(what, 'sum', total.tolist(), 'cnt', cnt.tolist(), 'want', sum_w.tolist(), cnt_w.tolist())
            assert total.tolist() == sum_w.tolist() and cnt.tolist() == cnt_w.tolist(), what
            same_bits(h.chrominance(src, GAINS[gains]), chroma_w, (*what, 'chrominance'))
            same_bits(out, out_w, what)


@pytest.mark.parametrize('out_dtype', DTYPES)
@pytest.mark.parametrize('in_dtype', DTYPES)
def test_clip_mode(td, dev, in_dtype, out_dtype):
    for name in ('2x2', '130x18', '258x34', '200x50'):
        for pattern in sorted(PATTERNS):
            for gains in GAINS:
                h = make(td, dev, name, pattern, mode='clip')
                out = h.process(source(dev, name, in_dtype), GAINS[gains], out_dtype=TORCH[out_dtype])
                same_bits(out, want(name, pattern, gains, in_dtype, out_dtype, 'clip')[0], (name, pattern, gains, 'clip'))
    assert h.lds_bytes() == 0


@pytest.mark.parametrize('in_dtype', DTYPES)
def test_input_view_at_an_odd_element_offset(td, dev, in_dtype):
    """The buffer does not start on a site pair: loads go per element."""
    for name in ('130x18', '258x34', '4x6'):
        for mode in ('opposed', 'clip'):
            for offset in (1, 3):
                h = make(td, dev, name, 'GRBG', mode)
                src = source(dev, name, in_dtype, offset)
                assert src.data_ptr() % (2 * src.element_size()) != 0
                out_w, sum_w, cnt_w, _ = want(name, 'GRBG', 'daylight', in_dtype, np.float32, mode)
                same_bits(h.process(src, GAINS['daylight']), out_w, (name, mode, offset))
                if mode == 'opposed':
                    total, cnt = h.statistics(src, GAINS['daylight'])
                    assert total.tolist() == sum_w.tolist() and cnt.tolist() == cnt_w.tolist()


def test_output_at_an_odd_element_offset_through_the_c_entry_point(td, dev):
    from torch_darktable._native import lib

    for name, dtype, tag in (('258x34', np.float32, 0), ('130x18', np.float16, 1)):
        L, kw = CASES[name]
        h = make(td, dev, name, 'BGGR')
        src = source(dev, name, dtype)
        pool = torch.zeros(L.size + 40, dtype=src.dtype, device=dev)
        out = pool[3:3 + L.size]
        gains = torch.tensor(GAINS['daylight'], dtype=torch.float32, device=dev)
        ws = torch.zeros(h.workspace_bytes() + 16, dtype=torch.uint8, device=dev)[5:]
        rc = lib.tdk_highlights(src.data_ptr(), tag, out.data_ptr(), tag, ws.data_ptr(), L.shape[1], L.shape[0], PATTERNS['BGGR'], gains.data_ptr(),
                                h.threshold, h.low, h.min_count, 1, None, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.tdk_last_error()
        torch.cuda.synchronize()
        same_bits(out.view(L.shape), want(name, 'BGGR', 'daylight', dtype, dtype)[0], name)
        assert float(pool[:3].float().abs().max()) == 0 and float(pool[3 + L.size:].float().abs().max()) == 0   # nothing written outside


# ------------------------------------------------------------------ 2. identities
@pytest.mark.parametrize('dtype', DTYPES)
def test_without_a_clipped_site_it_is_the_plain_white_balance(td, dev, dtype):
    L = CASES['none'][0]
    for pattern in sorted(PATTERNS):
        h = make(td, dev, 'none', pattern)
        src = source(dev, 'none', dtype)
        bayer = getattr(td.BayerPattern, pattern)
        # gains that keep every v <= 1: the bits of apply_white_balance everywhere
        mild = torch.tensor((1.1, 1.0, 1.15), dtype=torch.float32, device=dev)
        out = h.process(src, mild, out_dtype=TORCH[dtype])
        assert float(out.max()) <= 1.0
        assert torch.equal(out.view(torch.uint8), td.apply_white_balance(src, mild, bayer).view(torch.uint8))
        # daylight gains: fmaxf(L * g, 0), above 1 too; the white balance's bits where v <= 1
        day = torch.tensor(GAINS['daylight'], dtype=torch.float32, device=dev)
        out = h.process(src, day, out_dtype=TORCH[dtype])
        plain = td.apply_white_balance(src, day, bayer)
        assert float(out.max()) > 1.0 and torch.equal(out[out <= 1].view(torch.uint8), plain[out <= 1].view(torch.uint8))
        g = np.asarray(GAINS['daylight'], dtype=np.float32)[spec.colour_map(*L.shape, PATTERNS[pattern])]
        same_bits(out, np.fmax(L.astype(dtype).astype(np.float32) * g, np.float32(0)).astype(dtype), pattern)
        total, cnt = h.statistics(src, day)
        assert total.tolist() == [0, 0, 0] and cnt.tolist() == [0, 0, 0]


def test_supplied_chrominance_gives_the_same_bits_and_is_used_as_it_is(td, dev):
    for name in ('258x34', '200x50', '130x18'):
        for dtype in DTYPES:
            h = make(td, dev, name, 'RGGB')
            src = source(dev, name, dtype)
            out = h.process(src, GAINS['daylight'])
            chroma = h.chrominance(src, GAINS['daylight'])
            assert torch.equal(h.process(src, GAINS['daylight'], chrominance=chroma).view(torch.int32), out.view(torch.int32))
            L, kw = CASES[name]
            given = (0.5, -0.25, 0.125)
            expected = highlights_ref(L.astype(dtype), GAINS['daylight'], PATTERNS['RGGB'], chroma=given, **kw)[0]
            same_bits(h.process(src, GAINS['daylight'], chrominance=given), expected, (name, 'given chrominance'))


# ------------------------------------------------------------------ 3. streams and graphs
def test_two_objects_on_two_streams_agree(td, dev):
    name = '258x34'
    src = source(dev, name, np.float32)
    gains = torch.tensor(GAINS['daylight'], dtype=torch.float32, device=dev)
    a, b = make(td, dev, name, 'RGGB'), make(td, dev, name, 'RGGB')
    s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    for s in (s1, s2):
        s.wait_stream(torch.cuda.current_stream())
    outs = []
    for _ in range(3):
        with torch.cuda.stream(s1):
            oa = a.process(src, gains)
        with torch.cuda.stream(s2):
            ob = b.process(src, gains)
        outs.append((oa, ob))
    torch.cuda.synchronize()
    expected = want(name, 'RGGB', 'daylight', np.float32, np.float32)[0]
    for oa, ob in outs:
        assert torch.equal(oa.view(torch.int32), ob.view(torch.int32))
        same_bits(oa, expected, 'two streams')


def test_graph_capture_from_the_first_call(td, dev):
    """An object built on the side stream and captured there without a warm-up call (its workspace exists since construction); two
    replays equal the eager result bit for bit."""
    name = '258x34'
    src = source(dev, name, np.float16)
    gains = torch.tensor(GAINS['green_largest'], dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        h = make(td, dev, name, 'GBRG')
        with torch.cuda.graph(graph, stream=stream):
            captured = h.process(src, gains)
    eager = make(td, dev, name, 'GBRG').process(src, gains)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured.view(torch.int32), eager.view(torch.int32))
    same_bits(captured, want(name, 'GBRG', 'green_largest', np.float16, np.float32)[0], 'graph')


# ------------------------------------------------------------------ 4. pipeline
def _processor(td, dev, w, h, **kw):
    from torch_darktable.pipeline import Debayer, ImageProcessingSettings, ImageProcessor, ImageTransform, ToneMapper
    settings = ImageProcessingSettings(moving_average=0.3, postprocess=False, enable_denoise=True, enable_bilateral=True, tone_mapping=ToneMapper.reinhard,
                                       debayer=Debayer.bilinear)
    return ImageProcessor((w, h), td.BayerPattern.RGGB, td.PackedFormat.Packed12, settings, dev, GAINS['daylight'], transforms=ImageTransform.none, **kw)


def test_pipeline_rebuilds_highlights_in_front_of_the_demosaic(td, dev):
    """128 x 96, the 5x5 bilinear demosaic (reach: two sites).  With highlights=h the demosaiced frame differs from the plain one
    only within that reach of a site where the restatement differs from the plain white balance; highlights=None is the plain chain."""
    w, h = 128, 96
    L = spec.scene(h, w, 7, blobs=[(30, 40, 5.0), (70, 100, 4.0)])
    packed = td.encode12_float(torch.from_numpy(L).to(dev).reshape(-1))
    plain = _processor(td, dev, w, h)
    hl = td.Highlights(dev, (w, h), td.BayerPattern.RGGB)
    rebuilt = _processor(td, dev, w, h, highlights=hl)
    decoded = plain.load_bytes(packed).cpu().numpy()
    out_w = highlights_ref(decoded, GAINS['daylight'], PATTERNS['RGGB'])[0]
    g = np.asarray(GAINS['daylight'], dtype=np.float32)[spec.colour_map(h, w, PATTERNS['RGGB'])]
    changed = bits(out_w) != bits(np.fmin(np.fmax(decoded * g, np.float32(0)), np.float32(1)))
    assert 100 < changed.sum() < changed.size // 2
    reach = np.zeros((h + 4, w + 4), dtype=bool)
    for di in range(5):
        for dj in range(5):
            reach[di:di + h, dj:dj + w] |= changed
    reach = reach[2:-2, 2:-2]
    a, b = plain.load_image(packed), rebuilt.load_image(packed)
    assert a.dtype == b.dtype and a.shape == b.shape == (h, w, 3)
    differs = (a != b).any(dim=2).cpu().numpy()
    assert differs.any() and not (differs & ~reach).any()
    same_bits(hl.process(plain.load_bytes(packed), plain.white_balance), out_w, 'the mosaic the demosaic gets')
    out = rebuilt.process(packed, 'cam')
    assert out.dtype == torch.uint8 and tuple(out.shape) == (h, w, 3)
    # None, and the argument left out, is today's chain; so is every debayer setting
    assert plain.highlights is None
    assert torch.equal(_processor(td, dev, w, h, highlights=None).process(packed, 'cam'), _processor(td, dev, w, h).process(packed, 'cam'))
    # with the sensor correction in front: its gains are left to the highlight stage
    rp = td.RawPrepare(dev, (w, h), td.BayerPattern.RGGB, black=0.0, white=4095.0)
    both = _processor(td, dev, w, h, highlights=hl, raw_correction=rp)
    assert torch.equal(both.load_image(packed), b)
    half = _processor(td, dev, w, h, highlights=hl, storage_dtype=torch.float16).load_image(packed)
    assert half.dtype == torch.float16 and torch.equal(half, b.to(torch.float16))
