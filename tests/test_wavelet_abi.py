"""CPU-only: the eighth header include/tdk_hip_wavelet.h (wavelet denoiser) -- it parses to exactly its five declarations
(exports and the ctypes table: tests/test_header_abi.py), every argument error of
tdk_wavelet is reported on the host before any HIP call, the workspace and LDS queries answer 0 for what the call rejects, and the
Python front-end torch_darktable.Wavelet and the pipeline hook exist and raise the error types of the other operators."""

import ctypes
import inspect
import re
from pathlib import Path

import pytest

from abi_header import declarations, load_build_module

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / 'include' / 'tdk_hip_wavelet.h'
EXPECTED = ['tdk_wavelet', 'tdk_wavelet_abi_version', 'tdk_wavelet_band_norms', 'tdk_wavelet_lds_bytes', 'tdk_wavelet_workspace_bytes']
F32, F16, U8 = 0, 1, 2
YCC = 1


def test_header_declares_the_wavelet_surface(td):
    from torch_darktable import _native

    decls = declarations(HEADER)
    assert sorted(decls) == EXPECTED
    text = HEADER.read_text()
    assert re.search(r'#define TDK_WAVELET_ABI_VERSION 1\b', text)
    assert re.search(r'#define TDK_WAVELET_YCC 1\b', text) and re.search(r'#define TDK_WAVELET_MAX_SCALES 5\b', text)
    assert '#include "tdk_hip.h"' in text and 'extern "C"' in text
    assert decls['tdk_wavelet'] == ('int', ['const void* src', 'void* dst', 'void* workspace', 'int width', 'int height', 'int channels', 'int dtype',
                                            'int scales', 'const float* thresholds', 'int flags', 'tdk_stream_t stream'])
    assert decls['tdk_wavelet_band_norms'] == ('int', ['int scales', 'float* norms'])
    assert decls['tdk_wavelet_workspace_bytes'] == ('size_t', ['int width', 'int height', 'int channels', 'int scales'])
    assert decls['tdk_wavelet_lds_bytes'] == ('size_t', ['int channels', 'int dtype', 'int scales', 'int flags'])
    for formula in ('Y  = (0.25f*r + 0.5f*g) + 0.25f*b', 'Cb = b - g', 'Cr = r - g', 'g = Y - 0.25f*(Cb + Cr)', 'r = Cr + g', 'b = Cb + g',
                    'h = (0.0625f*(c_s[-2p] + c_s[+2p]) + 0.25f*(c_s[-p] + c_s[+p])) + 0.375f*c_s[0]', 'd_s = c_s - c_{s+1}',
                    "d'_s = |d_s| > t ? copysignf(|d_s| - t, d_s) : 0", "acc = acc + d'_s", 'y = acc + c_S'):
        assert formula in text, formula
    assert (_native.TDK_WAVELET_YCC, _native.TDK_WAVELET_MAX_SCALES) == (YCC, 5)
    assert _native.ABI_VERSIONS['tdk_wavelet_abi_version'] == (1, 'wavelet ABI')
    assert (ROOT / 'torch-darktable_amd' / 'csrc' / 'wavelet.hip') in load_build_module()._inputs()


def test_wavelet_invalid_arguments_fail_on_the_host(td):
    from torch_darktable._native import lib

    fake = 1 << 20   # never dereferenced: every check below happens before anything touches device memory or a device
    good = (ctypes.c_float * 15)(*([0.01] * 15))
    names = ['src', 'dst', 'ws', 'w', 'h', 'c', 'dtype', 'scales', 'thresholds', 'flags', 'stream']
    args = [fake, fake + (1 << 24), fake + (1 << 26), 64, 48, 3, F32, 4, good, 0, None]

    def call(**change):
        a = list(args)
        for k, v in change.items():
            a[names.index(k)] = v
        return lib.tdk_wavelet(*a)

    for k in ('src', 'dst', 'thresholds'):
        assert call(**{k: None}) == 1 and b'null pointer' in lib.tdk_last_error(), k
    for k in ('w', 'h'):
        for v in (0, -3, 65536):
            assert call(**{k: v}) == 1 and b'frame size' in lib.tdk_last_error(), (k, v)
    for c in (0, 2, 4):
        assert call(c=c) == 1 and b'channels' in lib.tdk_last_error(), c
    for d in (U8, 3, -1):
        assert call(dtype=d) == 1 and b'dtype' in lib.tdk_last_error(), d
    for s in (0, -1, 6):
        assert call(scales=s) == 1 and b'scales' in lib.tdk_last_error(), s
    for bad in (-0.1, float('nan'), float('inf')):
        for k in (0, 5, 11):
            t = (ctypes.c_float * 15)(*good)
            t[k] = bad
            assert call(thresholds=t) == 1 and b'thresholds[%d]' % k in lib.tdk_last_error(), (k, bad)
    beyond = (ctypes.c_float * 15)(*good)
    beyond[12] = float('nan')                      # past scales * channels: never read
    assert call(thresholds=beyond, dtype=7) == 1 and b'dtype' in lib.tdk_last_error()
    for f in (2, 4, -1, 3):
        assert call(flags=f) == 1 and b'flags' in lib.tdk_last_error(), f
    assert call(c=1, flags=YCC) == 1 and b'TDK_WAVELET_YCC needs three channels' in lib.tdk_last_error()
    # overlap, in bytes of the dtype: the same pointer, dst inside src, src inside dst, and the last byte
    nbytes = 64 * 48 * 3 * 4
    for dst in (fake, fake + 64, fake - nbytes + 4, fake + nbytes - 4):
        assert call(dst=dst) == 1 and b'overlap' in lib.tdk_last_error(), dst
    assert call(dst=fake + nbytes // 2 - 2, dtype=F16) == 1 and b'overlap' in lib.tdk_last_error()
    # the workspace: needed beyond the fused scales, and then clear of both frames
    assert call(ws=None) == 1 and b'null pointer (workspace' in lib.tdk_last_error()
    assert call(ws=None, scales=3) == 1 and b'workspace' in lib.tdk_last_error()
    assert call(ws=fake + 16) == 1 and b'workspace overlaps' in lib.tdk_last_error()
    assert call(ws=fake + (1 << 24) - 64) == 1 and b'workspace overlaps' in lib.tdk_last_error()


def test_workspace_and_lds_queries(td):
    from torch_darktable._native import lib

    ws, lds = lib.tdk_wavelet_workspace_bytes, lib.tdk_wavelet_lds_bytes
    for bad in ((0, 48, 3, 4), (64, 0, 3, 4), (65536, 48, 3, 4), (64, 65536, 3, 4), (64, 48, 2, 4), (64, 48, 0, 4), (64, 48, 3, 0), (64, 48, 3, 6), (64, 48, 3, -1)):
        assert ws(*bad) == 0, bad
    for bad in ((0, F32, 3, 0), (2, F32, 3, 0), (4, F32, 3, 0), (3, U8, 3, 0), (3, -1, 3, 0), (3, F32, 0, 0), (3, F32, 6, 0), (3, F32, 3, 2), (3, F32, 3, -1),
                (1, F32, 3, YCC), (1, F16, 1, YCC)):
        assert lds(*bad) == 0, bad
    fused = td.Wavelet.FUSED
    assert fused == 2 and td.Wavelet.TILE == (32, 32)
    for c in (1, 3):
        for s in range(1, 6):
            for w, h in ((1, 1), (61, 47), (64, 48), (4000, 3000)):
                b = ws(w, h, c, s)
                if s <= fused:
                    assert b == 0, (w, h, c, s)
                else:   # float32 planes with rows of whole 16-byte groups: acc and c, and a second c when two coarse launches follow
                    sets = 2 if s == fused + 1 else 3
                    assert b == sets * c * ((w + 3) // 4 * 4) * h * 4 + 16, (w, h, c, s, b)
            for dtype in (F32, F16):
                for flags in (0,) + ((YCC,) if c == 3 else ()):
                    b = lds(c, dtype, s, flags)
                    fine = (c + 1) * 36 * 36 * 4 if s == 1 else (c + 2) * 44 * 44 * 4
                    assert b == (fine if s <= fused else max(fine, 25600)), (c, dtype, s, flags, b)
                    assert 0 < b <= 65536
    assert lds(3, F16, 5, YCC) == 38720 and 4 * 38720 <= 160 * 1024   # four workgroups of the fine launch per CU


def test_package_exports_wavelet(td):
    import torch_darktable

    assert torch_darktable.Wavelet is torch_darktable.wavelet.Wavelet
    assert 'Wavelet' in torch_darktable.__all__ and 'wavelet' in torch_darktable.__all__
    assert torch_darktable.wavelet.__all__ == ['Wavelet']
    for name in ('process', 'process_luminance', 'process_log_luminance', 'from_sigma'):
        assert callable(getattr(torch_darktable.Wavelet, name)), name
    from torch_darktable import torch_darktable_extension as ext   # its extra exports are a closed list: nothing of the wavelet
    assert not any('wavelet' in n.lower() for n in dir(ext))


def test_pipeline_takes_a_chroma_denoiser_and_the_settings_stay_pinned(td):
    import torch
    from torch_darktable.pipeline import ImageProcessingSettings, ImageProcessor

    params = list(inspect.signature(ImageProcessor.__init__).parameters)
    assert params[-1] == 'raw_correction' and params[-3:] == ['sharpen', 'chroma_denoise', 'raw_correction']
    assert inspect.signature(ImageProcessor.__init__).parameters['chroma_denoise'].default is None
    cuda = torch.device('cuda', 0)
    make = lambda **kw: ImageProcessor((64, 48), td.BayerPattern.RGGB, td.PackedFormat.Packed12, ImageProcessingSettings(), cuda, None, **kw)  # noqa: E731
    with pytest.raises(TypeError, match='chroma_denoise must be a Wavelet'):
        make(chroma_denoise=object())
    with pytest.raises(TypeError, match='sharpen must be a Sharpen'):
        make(sharpen=object())
    with pytest.raises(ValueError, match='chroma_denoise is for 32x48'):
        make(chroma_denoise=td.Wavelet(cuda, (32, 48)))
    with pytest.raises(ValueError, match='three channels'):
        make(chroma_denoise=td.Wavelet(cuda, (64, 48), 2, [[0.1], [0.1]]))
    assert 'chroma_denoise' not in inspect.signature(ImageProcessor.from_camera_settings).parameters
    assert not any('wavelet' in name or 'chroma_denoise' in name for name in ImageProcessingSettings.model_fields)


def test_python_front_end_raises_the_error_types_of_the_other_operators(td):
    import torch

    cuda = torch.device('cuda', 0)   # a device object only: without a GPU nothing below reaches one (with one, a Wavelet allocates its workspace)
    W = td.Wavelet
    with pytest.raises(ValueError, match='CUDA'):
        W(torch.device('cpu'), (64, 48))
    for size in ((0, 48), (64, 0), (65536, 48)):
        with pytest.raises(ValueError, match='dimensions'):
            W(cuda, size)
    for s in (0, 6, -1):
        with pytest.raises(ValueError, match='scales'):
            W(cuda, (64, 48), scales=s)
        with pytest.raises(ValueError, match='scales'):
            W.from_sigma(cuda, (64, 48), (0.01, 0.01, 0.01), scales=s)
    for t in (-0.1, float('nan'), float('inf'), [0.1, 0.1, 0.1, -1.0], [[0.1, 0.1, float('nan')]] * 4):
        with pytest.raises(ValueError, match='finite'):
            W(cuda, (64, 48), 4, t)
    for t in ([0.1, 0.1], [0.1] * 5, [[0.1] * 3] * 3):
        with pytest.raises(ValueError, match='thresholds must be one value'):
            W(cuda, (64, 48), 4, t)
    for t in ([[0.1, 0.1]] * 4, [[0.1] * 3, [0.1] * 3, [0.1], [0.1] * 3]):
        with pytest.raises(ValueError, match='threshold rows'):
            W(cuda, (64, 48), 4, t)
    with pytest.raises(ValueError, match='ycc needs three channels'):
        W(cuda, (64, 48), 2, [[0.1], [0.1]], ycc=True)
    for sigma in ((0.1, -0.1, 0.1), (0.1, float('nan'), 0.1)):
        with pytest.raises(ValueError, match='sigma'):
            W.from_sigma(cuda, (64, 48), sigma)
    with pytest.raises(ValueError, match='strength'):
        W.from_sigma(cuda, (64, 48), (0.1, 0.1, 0.1), strength=-1.0)

    w = W(cuda, (64, 48))
    assert (w.width, w.height, w.scales, w.ycc, w.channels) == (64, 48, 4, False, None) and w.thresholds == ((0.0,),) * 4
    assert repr(w) == 'Wavelet(64x48, scales=4, ycc=False, thresholds=((0.0,), (0.0,), (0.0,), (0.0,)))'
    assert w.workspace_bytes() == 3 * 3 * 64 * 48 * 4 + 16 and W(cuda, (64, 48), 2).workspace_bytes() == 0
    assert w.lds_bytes(3, torch.float16) == 38720 and w.lds_bytes(1, torch.float32) == 25600
    assert w.lds_bytes(3, torch.uint8) == 0 and w.lds_bytes(2, torch.float32) == 0
    # from_sigma: t[s][k] = strength * sigma_k * n_s, formed in double and rounded once
    from torch_darktable.wavelet import band_norms
    n = band_norms(3)
    s = W.from_sigma(cuda, (64, 48), (0.03, 0.01, 0.02), scales=3, strength=2.0)
    f32 = lambda v: ctypes.c_float(v).value  # noqa: E731
    per = ((0.03 ** 2 + 4 * 0.01 ** 2 + 0.02 ** 2) ** 0.5 / 4.0, (0.02 ** 2 + 0.01 ** 2) ** 0.5, (0.03 ** 2 + 0.01 ** 2) ** 0.5)
    assert s.ycc and s.channels == 3 and s.thresholds == tuple(tuple(f32(2.0 * p * n[i]) for p in per) for i in range(3))
    plain = W.from_sigma(cuda, (64, 48), (0.03, 0.01, 0.02), scales=2, ycc=False)
    assert not plain.ycc and plain.thresholds == tuple(tuple(f32(3.0 * p * n[i]) for p in (0.03, 0.01, 0.02)) for i in range(2))

    with pytest.raises(AssertionError, match='3 dimensions'):
        w.process(torch.zeros(48, 64))
    with pytest.raises(RuntimeError, match='expected'):
        w.process(torch.zeros(48, 32, 3))
    with pytest.raises(ValueError, match='channels'):
        w.process(torch.zeros(48, 64, 2))
    with pytest.raises(RuntimeError, match='CUDA'):
        w.process(torch.zeros(48, 64, 3))   # no CPU fallback
