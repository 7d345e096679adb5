"""CPU-only: the ninth header include/tdk_hip_highlights.h (highlight reconstruction) -- it parses to exactly its five declarations
(exports and the ctypes table: tests/test_header_abi.py), its source is part of the build's source hash,
every argument error of tdk_highlights and tdk_highlights_chrominance is reported on the host
before any HIP call, and the Python front-end torch_darktable.Highlights and the pipeline hook raise the error types of the other
operators."""

import inspect
import re
from pathlib import Path

import pytest

from abi_header import declarations, load_build_module

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / 'include' / 'tdk_hip_highlights.h'
EXPECTED = ['tdk_highlights', 'tdk_highlights_abi_version', 'tdk_highlights_chrominance', 'tdk_highlights_lds_bytes', 'tdk_highlights_workspace_bytes']
F32, F16, U8 = 0, 1, 2
CLIP, OPPOSED = 0, 1
RGGB = 0x94949494


def test_header_declares_the_highlights_surface(td):
    from torch_darktable import _native

    decls = declarations(HEADER)
    assert sorted(decls) == EXPECTED
    text = HEADER.read_text()
    assert re.search(r'#define TDK_HIGHLIGHTS_ABI_VERSION 1\b', text)
    assert re.search(r'#define TDK_HL_CLIP 0\b', text) and re.search(r'#define TDK_HL_OPPOSED 1\b', text)
    assert '#include "tdk_hip.h"' in text and 'extern "C"' in text
    assert decls['tdk_highlights'] == ('int', ['const void* src', 'int src_dtype', 'void* dst', 'int dst_dtype', 'void* workspace', 'int width', 'int height',
                                               'uint32_t pattern', 'const float* gains', 'float threshold', 'float low', 'int min_count', 'int mode',
                                               'const float* chroma', 'tdk_stream_t stream'])
    assert decls['tdk_highlights_chrominance'] == ('int', ['const void* src', 'int src_dtype', 'void* workspace', 'int width', 'int height', 'uint32_t pattern',
                                                           'const float* gains', 'float threshold', 'float low', 'int min_count', 'long long* stats',
                                                           'float* chroma', 'tdk_stream_t stream'])
    assert decls['tdk_highlights_workspace_bytes'] == ('size_t', []) and decls['tdk_highlights_lds_bytes'] == ('size_t', ['int mode'])
    for formula in ('v       = L * g[c]', 'clipped = (L >= t)', 'cl[k]   = t * g[k]', 'm   = fminf(fminf(cl[0], cl[1]), cl[2])', 'out = fminf(fmaxf(v, 0.0f), m)',
                    'mean_k = S_k / (float)n_k', 'ref = 0.5f * (mean_a + mean_b)', 'v > low * cl[c]', 'fabsf(d) <= 64.0f', 'q = (long long)rintf(d * 1048576.0f)',
                    'chroma[c] = cnt[c] >= min_count ? (float)((double)sum[c] / ((double)cnt[c] * 1048576.0)) : 0.0f', 'out = fmaxf(v, ref + chroma[c])',
                    'out = fmaxf(v, 0.0f)'):
        assert formula in text, formula
    assert (_native.TDK_HL_CLIP, _native.TDK_HL_OPPOSED) == (CLIP, OPPOSED)
    assert _native.ABI_VERSIONS['tdk_highlights_abi_version'] == (1, 'highlights ABI')
    assert (ROOT / 'torch-darktable_amd' / 'csrc' / 'highlights.hip') in load_build_module()._inputs()


def test_highlights_invalid_arguments_fail_on_the_host(td):
    from torch_darktable._native import lib

    fake = 1 << 20   # never dereferenced: every check below happens before anything touches device memory or a device
    names = ['src', 'src_dtype', 'dst', 'dst_dtype', 'ws', 'w', 'h', 'pattern', 'gains', 'threshold', 'low', 'min_count', 'mode', 'chroma', 'stream']
    args = [fake, F32, fake + (1 << 24), F32, fake + (1 << 26), 64, 48, RGGB, fake + (1 << 27), 0.98, 0.2, 64, OPPOSED, None, None]

    def call(**change):
        a = list(args)
        for k, v in change.items():
            a[names.index(k)] = v
        return lib.tdk_highlights(*a)

    def fails(needle, **change):
        assert call(**change) == 1 and needle in lib.tdk_last_error(), (change, lib.tdk_last_error())

    for k in ('src', 'dst', 'gains'):
        fails(b'null pointer', **{k: None})
    fails(b'null pointer (workspace', ws=None)
    for k in ('w', 'h'):
        for v in (0, -2, 1, 65536):
            fails(b'frame size', **{k: v})
        for v in (3, 65535):
            fails(b'must be even', **{k: v})
    for k in ('src_dtype', 'dst_dtype'):
        for d in (U8, 3, -1):
            fails(b'dtype', **{k: d})
    for p in (0, 0x94949495, 0xffffffff):
        fails(b'Bayer pattern', pattern=p)
    for m in (2, -1, 7):
        fails(b'mode', mode=m)
    for t in (0.0, -0.5, 1.5, float('nan'), float('inf')):
        fails(b'threshold', threshold=t)
    for v in (-0.1, 1.0, 2.0, float('nan')):
        fails(b'low', low=v)
    for v in (0, -3):
        fails(b'min_count', min_count=v)
    fails(b'TDK_HL_CLIP takes no workspace', mode=CLIP)
    fails(b'TDK_HL_CLIP takes no workspace', mode=CLIP, ws=None, chroma=fake + (1 << 28))
    # overlap, in bytes of the dtypes
    nbytes = 64 * 48 * 4
    for dst in (fake, fake + 64, fake - nbytes + 4, fake + nbytes - 4):
        fails(b'src and dst overlap', dst=dst)
    fails(b'src and dst overlap', dst=fake + nbytes // 2 - 2, src_dtype=F16)
    fails(b'gains and dst overlap', gains=fake + (1 << 24) + 8)
    fails(b'chroma and dst overlap', chroma=fake + (1 << 24) + nbytes - 4)
    for ws in (fake + 16, fake + (1 << 24) - 64, fake + (1 << 27) - 100):
        fails(b'workspace overlaps', ws=ws)

    cnames = ['src', 'src_dtype', 'ws', 'w', 'h', 'pattern', 'gains', 'threshold', 'low', 'min_count', 'stats', 'chroma', 'stream']
    cargs = [fake, F16, fake + (1 << 26), 64, 48, RGGB, fake + (1 << 27), 0.98, 0.2, 64, fake + (1 << 28), fake + (1 << 29), None]

    def cfails(needle, **change):
        a = list(cargs)
        for k, v in change.items():
            a[cnames.index(k)] = v
        assert lib.tdk_highlights_chrominance(*a) == 1 and needle in lib.tdk_last_error(), (change, lib.tdk_last_error())

    for k in ('src', 'gains', 'ws'):
        cfails(b'null pointer', **{k: None})
    cfails(b'null pointer (stats and chroma', stats=None, chroma=None)
    cfails(b'frame size', w=0)
    cfails(b'must be even', h=47)
    cfails(b'dtype', src_dtype=U8)
    cfails(b'Bayer pattern', pattern=1)
    cfails(b'threshold', threshold=0.0)
    cfails(b'low', low=1.0)
    cfails(b'min_count', min_count=0)
    cfails(b'aligned to 8', stats=fake + (1 << 28) + 4)
    cfails(b'workspace overlaps', ws=fake + 8)
    cfails(b'stats overlaps', stats=fake + 64)
    cfails(b'chroma overlaps', chroma=fake + (1 << 28) + 40)
    assert b'tdk_highlights_chrominance:' in lib.tdk_last_error()


def test_workspace_and_lds_queries(td):
    from torch_darktable._native import lib

    assert lib.tdk_highlights_workspace_bytes() == 256 * 48 + 8   # a 48-byte record per workgroup of the statistics launch: a few KB
    assert lib.tdk_highlights_lds_bytes(CLIP) == 0
    assert 0 < lib.tdk_highlights_lds_bytes(OPPOSED) <= 65536
    for bad in (2, -1, 100):
        assert lib.tdk_highlights_lds_bytes(bad) == 0


def test_package_exports_highlights(td):
    import torch_darktable

    assert torch_darktable.Highlights is torch_darktable.highlights.Highlights
    assert 'Highlights' in torch_darktable.__all__ and 'highlights' in torch_darktable.__all__
    assert torch_darktable.highlights.__all__ == ['Highlights']
    for name in ('process', 'chrominance', 'statistics', 'lds_bytes'):
        assert callable(getattr(torch_darktable.Highlights, name)), name
    import test_highlights_spec
    assert torch_darktable.Highlights.TILE == test_highlights_spec.TILE
    params = inspect.signature(torch_darktable.Highlights.__init__).parameters
    assert list(params) == ['self', 'device', 'image_size', 'bayer_pattern', 'mode', 'threshold', 'low', 'min_count']
    assert [params[k].default for k in ('mode', 'threshold', 'low', 'min_count')] == ['opposed', 0.98, 0.2, 64]
    params = inspect.signature(torch_darktable.Highlights.process).parameters
    assert list(params) == ['self', 'mosaic', 'white_balance', 'out_dtype', 'chrominance'] and params['chrominance'].default is None


def test_pipeline_takes_a_highlights_stage(td):
    import torch
    from torch_darktable.pipeline import ImageProcessingSettings, ImageProcessor

    params = inspect.signature(ImageProcessor.__init__).parameters
    assert 'highlights' in params and params['highlights'].default is None
    cuda = torch.device('cuda', 0)
    make = lambda wb=(1.5, 1.0, 1.4), **kw: ImageProcessor((64, 48), td.BayerPattern.RGGB, td.PackedFormat.Packed12, ImageProcessingSettings(), cuda, wb, **kw)  # noqa: E731
    with pytest.raises(TypeError, match='highlights must be a Highlights'):
        make(highlights=object())
    with pytest.raises(ValueError, match=r'highlights is for \(32, 48\) RGGB'):
        make(highlights=td.Highlights(cuda, (32, 48), td.BayerPattern.RGGB))
    with pytest.raises(ValueError, match=r'highlights is for \(64, 48\) BGGR'):
        make(highlights=td.Highlights(cuda, (64, 48), td.BayerPattern.BGGR))
    with pytest.raises(ValueError, match='highlights needs white_balance'):
        make(wb=None, highlights=td.Highlights(cuda, (64, 48), td.BayerPattern.RGGB))
    assert 'highlights' not in inspect.signature(ImageProcessor.from_camera_settings).parameters
    assert not any('highlight' in name for name in ImageProcessingSettings.model_fields)


def test_python_front_end_raises_the_error_types_of_the_other_operators(td):
    import torch

    cuda = torch.device('cuda', 0)   # a device object only: without a GPU nothing below reaches one
    H, RG = td.Highlights, td.BayerPattern.RGGB
    with pytest.raises(ValueError, match='CUDA'):
        H(torch.device('cpu'), (64, 48), RG)
    for size in ((0, 48), (64, 0), (65536, 48)):
        with pytest.raises(ValueError, match='dimensions must be 2'):
            H(cuda, size, RG)
    for size in ((63, 48), (64, 47)):
        with pytest.raises(ValueError, match='must be even'):
            H(cuda, size, RG)
    with pytest.raises(ValueError, match='bayer pattern'):
        H(cuda, (64, 48), 0)
    with pytest.raises(ValueError, match='mode'):
        H(cuda, (64, 48), RG, mode='blend')
    for t in (0.0, -1.0, 1.01, float('nan')):
        with pytest.raises(ValueError, match='threshold'):
            H(cuda, (64, 48), RG, threshold=t)
    for v in (-0.1, 1.0, float('nan')):
        with pytest.raises(ValueError, match='low'):
            H(cuda, (64, 48), RG, low=v)
    for v in (0, -1, 2.5):
        with pytest.raises(ValueError, match='min_count'):
            H(cuda, (64, 48), RG, min_count=v)

    h = H(cuda, (64, 48), RG)
    assert (h.width, h.height, h.image_size, h.mode, h.threshold, h.low, h.min_count) == (64, 48, (64, 48), 'opposed', 0.98, 0.2, 64)
    assert repr(h) == 'Highlights(64x48, RGGB, mode=opposed, threshold=0.98, low=0.2, min_count=64)'
    assert 0 < h.lds_bytes() <= 65536 and H(cuda, (64, 48), RG, mode='clip').lds_bytes() == 0
    assert h.workspace_bytes() == 256 * 48 + 8

    with pytest.raises(AssertionError, match='2 dimensions'):
        h.process(torch.zeros(48, 64, 1), (1.5, 1.0, 1.4))
    with pytest.raises(RuntimeError, match='expected'):
        h.process(torch.zeros(48, 32), (1.5, 1.0, 1.4))
    with pytest.raises(RuntimeError, match='CUDA'):
        h.process(torch.zeros(48, 64), (1.5, 1.0, 1.4))   # no CPU fallback
    with pytest.raises(RuntimeError, match='CUDA'):
        h.statistics(torch.zeros(48, 64), (1.5, 1.0, 1.4))
    with pytest.raises(RuntimeError, match='CUDA'):
        h.chrominance(torch.zeros(48, 64), (1.5, 1.0, 1.4))
