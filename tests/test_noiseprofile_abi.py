"""CPU-only: the header include/tdk_hip_noise.h (noise profile) -- it parses to exactly its six declarations (exports and the ctypes
table: tests/test_header_abi.py), every argument error of its three entry points is reported on the host before any HIP call, the
workspace and LDS queries give the documented sizes, and the Python front-end torch_darktable.NoiseProfile / NoiseModel and the
pipeline hook exist and validate their arguments without a device."""

import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

from abi_header import declarations

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / 'include' / 'tdk_hip_noise.h'
EXPECTED = ['tdk_noise_abi_version', 'tdk_noise_lds_bytes', 'tdk_noise_profile', 'tdk_noise_stabilize', 'tdk_noise_unstabilize', 'tdk_noise_workspace_bytes']
F32, F16, U8, U16 = 0, 1, 2, 3
RGGB = 0x94949494
GRID, LEVELS = 512, 128
LDS = 3 * 32 * 128 * 4 + 3 * 32 * 8 + 10 * 8 + 4 * 16 * 64 * 2 + 4 * 16 * 4


def record(bins):   # uint32 levels, then the sums and the nine counters of 8 bytes
    return 3 * bins * LEVELS * 4 + (3 * bins + 9) * 8


def test_header_declares_the_noise_surface(td):
    from torch_darktable import _native

    decls = declarations(HEADER)
    assert sorted(decls) == EXPECTED
    text = HEADER.read_text()
    for define in ('TDK_NOISE_ABI_VERSION 1', 'TDK_NOISE_MAX_BINS 32', 'TDK_NOISE_MAX_FRAMES 16', 'TDK_NOISE_LEVELS 128', 'TDK_NOISE_MEDIAN_FACTOR 0.9796',
                   f'TDK_NOISE_GRID {GRID}', 'TDK_NOISE_STRIP_BYTES 512', 'TDK_NOISE_ALGEBRAIC 0', 'TDK_NOISE_UNBIASED 1'):
        assert re.search(rf'#define {re.escape(define)}(?!\d)', text), define
    assert '#include "tdk_hip.h"' in text and '#include "tdk_hip_stats.h"' in text and 'extern "C"' in text
    assert decls['tdk_noise_profile'] == ('int', ['const void* const* frames', 'int num_frames', 'int dtype', 'void* workspace', 'int width', 'int height',
                                                  'uint32_t pattern', 'int bins', 'float white', 'int clip_lo', 'int clip_hi', 'int min_count', 'long long* counts',
                                                  'float* model', 'float* curve', 'tdk_stream_t stream'])
    transform = ['const void* src', 'int src_dtype', 'void* dst', 'int dst_dtype', 'int64_t count', 'int width', 'int channels', 'uint32_t pattern',
                 'const float* model', 'const float* gains', 'float sigma_out']
    assert decls['tdk_noise_stabilize'] == ('int', transform + ['tdk_stream_t stream'])
    assert decls['tdk_noise_unstabilize'] == ('int', transform + ['int inverse', 'tdk_stream_t stream'])
    assert decls['tdk_noise_workspace_bytes'] == decls['tdk_noise_lds_bytes'] == ('size_t', ['int bins'])
    assert decls['tdk_noise_abi_version'] == ('int', [])
    for formula in ('q = (int) rintf(fminf(fmaxf(x * scale, 0), 65535))', 'scale = fl32(65535 / white)', 'p = 2*(i & 1) + (j & 1)', 'k = (pattern >> (2*p)) & 3',
                    'h(r, c) = 2*q(r, c) - q(r, c-1) - q(r, c+1)', 'v(r, c) = 2*q(r, c) - q(r-1, c) - q(r+1, c)', 'i = ((S >> 6) * I) >> 16',
                    'f = (E >> (e - 2)) & 3, l = min(4*(e - 8) + f + 1, 127)', 'E_lo(l) = (4 + ((l-1) & 3)) << (((l-1) >> 2) + 6)',
                    'r = ceil(0.5 * (double)n) clamped to [1, n]', 'frac = (double)(r - cum(l* - 1)) / (double)hist[k][i][l*]',
                    'E_med = (double)E_lo(l*) + frac * ((double)E_lo(l* + 1) - (double)E_lo(l*))', 'v_i = (E_med / (576.0 * kappa)) * (ws * ws)',
                    'x_i = (((double)sumS[k][i] / (64.0 * (double)n)) / 65535.0) * (double)white', 'w_i = (double)n / (v_i * v_i)',
                    'det = Sw * Swxx - Swx * Swx', 'a = (Sw * Swxv - Swx * Swv) / det;   b = (Swxx * Swv - Swx * Swxv) / det', 'a = 0, b = Swv / Sw',
                    'b = 0, a = Swxv / Swxx', "a' = g * a;   b' = (g * g) * b;   c = 0.375f * (a' * a') + b';   k = (2.0f * s) / a'",
                    "y = k * sqrtf(fmaxf(a' * x + c, 0.0f))", "y = (s * x) / sqrtf(b')", "x = d * sqrtf(b')", "x = ((a' * (d * d)) * 0.25f) - (c / a')",
                    'D = fmaxf(d, 1.2247449f)', '(0.30618622f / D)', '(1.375f / D2)', '(0.76546554f / (D2 * D))', "x = a' * fmaxf(I, 0.0f)",
                    'Decisions the issue left open'):
        assert formula in text, formula
    assert (_native.TDK_NOISE_MAX_BINS, _native.TDK_NOISE_MAX_FRAMES, _native.TDK_NOISE_LEVELS) == (32, 16, 128)
    assert (_native.TDK_NOISE_GRID, _native.TDK_NOISE_STRIP_BYTES, _native.TDK_NOISE_MEDIAN_FACTOR) == (GRID, 512, 0.9796)
    assert (_native.TDK_NOISE_ALGEBRAIC, _native.TDK_NOISE_UNBIASED) == (0, 1)
    assert _native.ABI_VERSIONS['tdk_noise_abi_version'] == (1, 'noise ABI')
    assert _native.lib.tdk_noise_abi_version() == 1
    names = [row[0] for row in _native.HEADERS]
    assert names[-3:] == ['tdk_hip_stats.h', 'tdk_hip_noise.h', 'tdk_hip_lut.h']   # in front of the last row, as the stats row was


def test_noise_profile_invalid_arguments_fail_on_the_host(td):
    from torch_darktable._native import lib

    fake = 1 << 30   # never dereferenced: every check below happens before anything touches device memory or a device
    frames = (ctypes.c_void_p * 2)(fake, fake + (1 << 24))
    workspace, counts, model, curve = fake + (1 << 26), fake + (3 << 26), fake + (4 << 26), fake + (5 << 26)
    names = ['frames', 'num_frames', 'dtype', 'workspace', 'width', 'height', 'pattern', 'bins', 'white', 'clip_lo', 'clip_hi', 'min_count', 'counts', 'model',
             'curve', 'stream']
    args = [frames, 2, F32, workspace, 640, 480, RGGB, 32, 1.0, 1, 64224, 32, counts, model, curve, None]

    def call(**change):
        a = list(args)
        for k, v in change.items():
            a[names.index(k)] = v
        return lib.tdk_noise_profile(*a)

    def rejected(word, **change):
        return call(**change) == 1 and word in lib.tdk_last_error()

    for k in ('frames', 'workspace', 'counts', 'model', 'curve'):
        assert rejected(b'null pointer', **{k: None}), k
    assert rejected(b'frames[1]', frames=(ctypes.c_void_p * 2)(fake, None))
    for v in (0, -1, 17):
        assert rejected(b'num_frames', num_frames=v), v
    for v in (U8, 4, -1):
        assert rejected(b'dtype', dtype=v), v
    for k in ('width', 'height'):
        for v in (0, -2, 65536):
            assert rejected(b'frame size', **{k: v}), (k, v)
        for v in (641, 65535):
            assert rejected(b'even', **{k: v}), (k, v)
    assert rejected(b'Bayer pattern', pattern=0x12345678) and rejected(b'Bayer pattern', pattern=0)
    for v in (1, 0, -5, 33):
        assert rejected(b'bins', bins=v), v
    for v in (0.0, -1.0, float('nan'), float('inf'), 1e-40):
        assert rejected(b'white', white=v), v
    for lo, hi in ((-1, 100), (5, 4), (0, 65536), (70000, 70001)):
        assert rejected(b'clip', clip_lo=lo, clip_hi=hi), (lo, hi)
    for v in (0, -1):
        assert rejected(b'min_count', min_count=v), v
    assert rejected(b'aligned to 8', counts=counts + 4)
    frame_bytes = 640 * 480 * 4
    for k in ('workspace', 'counts', 'model', 'curve'):
        assert rejected(b'frames[0] overlaps', **{k: fake + 64}), k
        assert rejected(b'frames[1] overlaps', **{k: fake + (1 << 24) + frame_bytes - 8}), k
    ws_bytes = lib.tdk_noise_workspace_bytes(32)
    assert rejected(b'overlap', counts=workspace + ws_bytes - 8) and rejected(b'overlap', model=counts + 8) and rejected(b'overlap', curve=model + 44)
    assert rejected(b'frames[0] overlaps', dtype=U16, counts=fake + 640 * 480 * 2 - 8)   # a 16-bit frame is half as long


def test_transform_invalid_arguments_fail_on_the_host(td):
    from torch_darktable._native import lib

    fake = 1 << 30
    src, dst, model, gains = fake, fake + (1 << 24), fake + (1 << 26), fake + (2 << 26)
    names = ['src', 'src_dtype', 'dst', 'dst_dtype', 'count', 'width', 'channels', 'pattern', 'model', 'gains', 'sigma_out', 'inverse', 'stream']
    args = [src, F32, dst, F16, 640 * 480 * 3, 0, 3, 0, model, gains, 1.0, 1, None]

    for fn, forward in ((lib.tdk_noise_stabilize, True), (lib.tdk_noise_unstabilize, False)):
        def rejected(word, **change):
            a = list(args)
            for k, v in change.items():
                a[names.index(k)] = v
            if forward:
                del a[names.index('inverse')]
            return fn(*a) == 1 and word in lib.tdk_last_error() and (b'tdk_noise_stabilize' if forward else b'tdk_noise_unstabilize') in lib.tdk_last_error()

        for k in ('src', 'dst', 'model'):
            assert rejected(b'null pointer', **{k: None}), k
        for k in ('src_dtype', 'dst_dtype'):
            for v in (U8, U16, -1):
                assert rejected(b'dtype', **{k: v}), (k, v)
        for v in (0, -4):
            assert rejected(b'count', count=v), v
        for v in (0, 2, 4):
            assert rejected(b'channels', channels=v), v
        assert rejected(b'multiple of channels', count=640 * 480 * 3 + 1)
        assert rejected(b'Bayer pattern', pattern=7, channels=1, width=640, count=640 * 480)
        assert rejected(b'channels = 1', pattern=RGGB, channels=3, width=640, count=640 * 480)
        for width in (0, 641, 65536):
            assert rejected(b'mosaic width', pattern=RGGB, channels=1, width=width, count=640 * 480), width
        assert rejected(b'rows', pattern=RGGB, channels=1, width=640, count=640 * 480 + 2) and rejected(b'rows', pattern=RGGB, channels=1, width=640, count=640 * 481)
        for v in (0.0, -1.0, float('nan'), float('inf')):
            assert rejected(b'sigma_out', sigma_out=v), v
        assert rejected(b'overlap', dst=src + 64) and rejected(b'overlap', dst=src) and rejected(b'overlap', src=dst + 640 * 480 * 3 * 2 - 2)
        assert rejected(b'overlap dst', model=dst + 16) and rejected(b'overlap dst', gains=dst + 640 * 480 * 3 * 2 - 4)
        if not forward:
            for v in (-1, 2):
                assert rejected(b'inverse', inverse=v), v


def test_workspace_and_lds_queries(td):
    from torch_darktable._native import lib

    ws, lds = lib.tdk_noise_workspace_bytes, lib.tdk_noise_lds_bytes
    for bad in (1, 0, -4, 33):
        assert ws(bad) == 0 and lds(bad) == 0, bad
    for bins in (2, 7, 31, 32):
        assert ws(bins) == GRID * record(bins) + 8 and record(bins) % 8 == 0, bins
        assert lds(bins) == LDS
    assert LDS <= 64 * 1024 and 2 * LDS <= 160 * 1024   # two workgroups share a compute unit
    assert ws(32) < 32 << 20


def test_package_exports_noiseprofile(td):
    import torch_darktable

    for name in ('NoiseProfile', 'NoiseModel', 'NoiseStatistics'):
        assert getattr(torch_darktable, name) is getattr(torch_darktable.noiseprofile, name)
    assert {'NoiseProfile', 'NoiseModel', 'NoiseStatistics', 'noiseprofile'} <= set(torch_darktable.__all__)
    assert torch_darktable.noiseprofile.__all__ == ['NoiseProfile', 'NoiseModel', 'NoiseStatistics']
    assert (torch_darktable.NoiseProfile.GRID, torch_darktable.NoiseProfile.STRIP_BYTES, torch_darktable.NoiseProfile.LEVELS) == (GRID, 512, LEVELS)
    for name in ('estimate', 'statistics', 'lds_bytes', 'workspace_bytes'):
        assert callable(getattr(torch_darktable.NoiseProfile, name)), name
    params = inspect.signature(torch_darktable.NoiseProfile.__init__).parameters
    assert list(params) == ['self', 'device', 'image_size', 'bayer_pattern', 'bins', 'white', 'clip', 'min_count', 'max_frames']
    assert [params[k].default for k in ('bins', 'white', 'clip', 'min_count', 'max_frames')] == [32, 1.0, (1, 64224), 32, 1]
    params = inspect.signature(torch_darktable.NoiseModel.stabilize).parameters
    assert list(params) == ['self', 'x', 'bayer_pattern', 'gains', 'sigma_out', 'out_dtype']
    import torch
    assert [params[k].default for k in ('bayer_pattern', 'gains', 'sigma_out', 'out_dtype')] == [None, None, 1.0, torch.float32]
    params = inspect.signature(torch_darktable.NoiseModel.unstabilize).parameters
    assert list(params) == ['self', 'y', 'bayer_pattern', 'gains', 'sigma_out', 'inverse', 'out_dtype']
    assert [params[k].default for k in ('bayer_pattern', 'gains', 'sigma_out', 'inverse', 'out_dtype')] == [None, None, 1.0, 'unbiased', None]
    for name in ('from_values', 'from_dict', 'to_dict', 'a', 'b', 'valid'):
        assert hasattr(torch_darktable.NoiseModel, name), name
    assert 'demosaic' in torch_darktable.noiseprofile.__doc__ and 'approximation' in torch_darktable.noiseprofile.__doc__


def test_pipeline_takes_a_noise_model(td):
    import torch
    from torch_darktable.pipeline import CameraSettings, ImageProcessingSettings, ImageProcessor

    params = inspect.signature(ImageProcessor.__init__).parameters
    # (the tests of the earlier stages pin the arguments from highlights on: a new stage goes in front of them, to be passed by keyword)
    names = list(params)
    assert names[names.index('exposure') + 1:names.index('highlights')] == ['noise_model'] and params['noise_model'].default is None
    dev = torch.device('cuda', 0)
    build = lambda **kw: ImageProcessor((64, 48), td.BayerPattern.RGGB, td.PackedFormat.Packed12, ImageProcessingSettings(), dev, None, **kw)
    model = td.NoiseModel.from_values(2e-4, 1e-6, torch.device('cpu'))
    for wrong in (object(), (2e-4, 1e-6), td.Wavelet(dev, (64, 48))):
        with pytest.raises(TypeError, match='noise_model must be a NoiseModel'):
            build(noise_model=wrong, chroma_denoise=td.Wavelet(dev, (64, 48)))
    with pytest.raises(ValueError, match='needs chroma_denoise'):
        build(noise_model=model)
    assert 'noise_model' not in inspect.signature(ImageProcessor.from_camera_settings).parameters
    for settings in (ImageProcessingSettings, CameraSettings):
        assert not {'noise_model', 'noise_profile', 'noiseprofile'} & set(settings.model_fields), settings


def test_python_front_end_validates_without_a_device(td):
    import torch

    cuda, cpu = torch.device('cuda', 0), torch.device('cpu')   # a device object only: nothing below needs a GPU
    P = td.BayerPattern.GRBG
    with pytest.raises(ValueError, match='CUDA'):
        td.NoiseProfile(cpu, (64, 48), P)
    for size in ((0, 48), (64, 0), (65536, 48)):
        with pytest.raises(ValueError, match='dimensions'):
            td.NoiseProfile(cuda, size, P)
    for size in ((63, 48), (64, 47)):
        with pytest.raises(ValueError, match='even'):
            td.NoiseProfile(cuda, size, P)
    with pytest.raises(ValueError, match='bayer pattern'):
        td.NoiseProfile(cuda, (64, 48), 'RGGB')
    for bins in (1, 33, 2.5, 0):
        with pytest.raises(ValueError, match='bins'):
            td.NoiseProfile(cuda, (64, 48), P, bins=bins)
    for white in (0.0, -1.0, float('nan'), float('inf'), 1e-40):
        with pytest.raises(ValueError, match='white'):
            td.NoiseProfile(cuda, (64, 48), P, white=white)
    for clip in ((-1, 5), (5, 4), (0, 65536), (1, 2, 3), (1.5, 9)):
        with pytest.raises(ValueError, match='clip'):
            td.NoiseProfile(cuda, (64, 48), P, clip=clip)
    for min_count in (0, -3, 2.5):
        with pytest.raises(ValueError, match='min_count'):
            td.NoiseProfile(cuda, (64, 48), P, min_count=min_count)
    for max_frames in (0, 17, 1.5):
        with pytest.raises(ValueError, match='max_frames'):
            td.NoiseProfile(cuda, (64, 48), P, max_frames=max_frames)

    # what the object tells: the float32 numbers the kernel is given
    npf = td.NoiseProfile(cuda, (64, 48), P, bins=16, white=0.9, clip=(2, 60000), min_count=8, max_frames=3)
    assert npf.image_size == (64, 48) and npf.white == float(np.float32(0.9)) and npf.clip == (2, 60000)
    assert (npf.bins, npf.min_count, npf.max_frames, npf.bayer_pattern) == (16, 8, 3, P)
    assert npf.lds_bytes() == LDS and npf.workspace_bytes() == GRID * record(16) + 8
    assert repr(npf) == 'NoiseProfile(64x48, GRBG, bins=16, white=0.9, clip=(2, 60000), min_count=8, max_frames=3)'
    with pytest.raises(RuntimeError, match='shape'):
        npf.estimate(torch.zeros(48, 64, 1))
    with pytest.raises(ValueError, match='max_frames'):
        npf.estimate([torch.zeros(48, 64)] * 4)
    with pytest.raises(ValueError, match='max_frames'):
        npf.statistics([])
    with pytest.raises(RuntimeError, match='CUDA'):
        npf.estimate(torch.zeros(48, 64))   # no CPU fallback

    # the model: host-side construction and the dictionary of the settings files
    m = td.NoiseModel.from_values((2e-4, 5e-5, 1e-3), 1e-6, cpu)
    assert m.model.shape == (3, 4) and m.curve is None
    assert m.a.tolist() == [float(np.float32(v)) for v in (2e-4, 5e-5, 1e-3)] and m.b.tolist() == [float(np.float32(1e-6))] * 3 and m.valid.tolist() == [1.0] * 3
    assert m.a.data_ptr() == m.model.data_ptr()   # views
    d = m.to_dict()
    assert d == {'a': m.a.tolist(), 'b': m.b.tolist(), 'valid': [True] * 3, 'bins': [0] * 3}
    back = td.NoiseModel.from_dict(d, cpu)
    assert torch.equal(back.model, m.model)
    assert td.NoiseModel.from_dict({'a': [1e-4] * 3, 'b': [0, 0, 0], 'valid': [True, False, True], 'bins': [4, 0, 9]}, cpu).model[:, 2:].tolist() == [[1, 4], [0, 0], [1, 9]]
    for a, b in (((1, 2), 0), (-1e-4, 0), (1e-4, float('nan')), ((1, 2, 3, 4), 0)):
        with pytest.raises(ValueError, match='three finite values'):
            td.NoiseModel.from_values(a, b, cpu)
    with pytest.raises(ValueError, match=r'\(3, 4\)'):
        td.NoiseModel(torch.zeros(4, 3))
    x = torch.zeros(48, 64, 3)
    with pytest.raises(ValueError, match='C = 1 or 3'):
        m.stabilize(torch.zeros(48, 64, 2))
    with pytest.raises(ValueError, match='mosaic'):
        m.stabilize(x, bayer_pattern=P)
    with pytest.raises(ValueError, match='mosaic'):
        m.unstabilize(torch.zeros(47, 64), bayer_pattern=P)
    with pytest.raises(ValueError, match='bayer pattern'):
        m.stabilize(torch.zeros(48, 64), bayer_pattern=1)
    for sigma_out in (0.0, -1.0, float('nan')):
        with pytest.raises(ValueError, match='sigma_out'):
            m.stabilize(x, sigma_out=sigma_out)
    with pytest.raises(ValueError, match='inverse'):
        m.unstabilize(x, inverse='exact')
    with pytest.raises(ValueError, match='out_dtype'):
        m.stabilize(x, out_dtype=torch.uint8)
    with pytest.raises(ValueError, match='empty'):
        m.stabilize(torch.zeros(0, 3))
    with pytest.raises(RuntimeError, match='CUDA'):
        m.stabilize(x)   # no CPU fallback
