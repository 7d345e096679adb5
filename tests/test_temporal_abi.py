"""CPU-only: the header include/tdk_hip_temporal.h (temporal denoiser) -- it parses to exactly its five declarations (exports and the
ctypes table: tests/test_header_abi.py), every argument error of its two entry points is reported on the host before any HIP call,
the state and LDS queries give the documented sizes, and the Python front-end torch_darktable.TemporalDenoise and the pipeline hook
exist and validate their arguments without a device."""

import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import temporal_spec as spec
from abi_header import declarations

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / 'include' / 'tdk_hip_temporal.h'
EXPECTED = ['tdk_temporal_abi_version', 'tdk_temporal_denoise', 'tdk_temporal_lds_bytes', 'tdk_temporal_reset', 'tdk_temporal_state_bytes']
F32, F16, U8, U16 = 0, 1, 2, 3
RGGB = 0x94949494
TW, TH = 64, 32


def lds(r):   # two staged planes with four columns either side, two planes of row sums
    return 4 * (2 * (TH + 2 * r) * (TW + 8) + 2 * (TH + 2 * r) * TW)


def test_header_declares_the_temporal_surface(td):
    from torch_darktable import _native

    decls = declarations(HEADER)
    assert sorted(decls) == EXPECTED
    text = HEADER.read_text()
    for define in ('TDK_TEMPORAL_ABI_VERSION 1', f'TDK_TEMPORAL_TILE_W {TW}', f'TDK_TEMPORAL_TILE_H {TH}', 'TDK_TEMPORAL_HEAD_BYTES 16', 'TDK_TEMPORAL_MAX_FRAMES 64'):
        assert re.search(rf'#define {re.escape(define)}(?!\d)', text), define
    assert '#include "tdk_hip.h"' in text and '#include "tdk_hip_noise.h"' in text and 'extern "C"' in text
    assert decls['tdk_temporal_denoise'] == ('int', ['const void* src', 'int src_dtype', 'void* out', 'int out_dtype', 'void* state', 'int state_dtype', 'int width',
                                                     'int height', 'uint32_t pattern', 'const float* model', 'const float* gains', 'int radius', 'float t_lo',
                                                     'float t_hi', 'float pixel_c2', 'float n_max', 'float v_min', 'tdk_stream_t stream'])
    assert decls['tdk_temporal_reset'] == ('int', ['void* state', 'tdk_stream_t stream'])
    assert decls['tdk_temporal_state_bytes'] == ('size_t', ['int width', 'int height', 'int state_dtype'])
    assert decls['tdk_temporal_lds_bytes'] == ('size_t', ['int radius'])
    assert decls['tdk_temporal_abi_version'] == ('int', [])
    for formula in ("a' = g * a;   b' = (g * g) * b", 'p = 2*(i & 1) + (j & 1)', 'k = (pattern >> (2*p)) & 3', 'inv = fl32(1 / (t_hi - t_lo))',
                    'A = first ? 0 : (float)acc_src[q]        N = first ? 0 : (float)cnt_src[q]', 'd = x - A',
                    "var = fmaxf(a' * fmaxf(A, 0) + b', v_min);   v = var + var / fmaxf(N, 1);   e = d * d", 'invalid row:  v = 0;  e = 0', 't  = E / V',
                    's  = fminf(fmaxf((t_hi - t) * inv, 0), 1)', 'if (e > c2 * v) s = 0', 'n1 = fminf(s * N + 1, n_max);   invalid row: n1 = 1',
                    "y  = (n1 == 1) ? x : A + d / n1", 'reads the planes (idx + 1) & 1 and writes the planes idx & 1', '0xFFFFFFFF -> 2',
                    'tdk_temporal_state_bytes = 16 + 2*PA + 2*PC', 'A sliding sum that adds and subtracts has other bits', 'raw mosaics only',
                    'Decisions the issue left open'):
        assert formula in text, formula
    assert (_native.TDK_TEMPORAL_TILE_W, _native.TDK_TEMPORAL_TILE_H, _native.TDK_TEMPORAL_HEAD_BYTES, _native.TDK_TEMPORAL_MAX_FRAMES) == (TW, TH, 16, 64)
    assert _native.ABI_VERSIONS['tdk_temporal_abi_version'] == (1, 'temporal ABI')
    assert _native.lib.tdk_temporal_abi_version() == 1
    rows = [row for row in _native.HEADERS if row[0] == 'tdk_hip_temporal.h']
    assert rows == [('tdk_hip_temporal.h', _native.TEMPORAL_SIGNATURES, 'tdk_temporal_abi_version', 1, 'temporal ABI')]


def test_denoise_invalid_arguments_fail_on_the_host(td):
    from torch_darktable._native import lib

    fake = 1 << 30   # never dereferenced: every check below happens before anything touches device memory or a device
    w, h = 640, 480
    src, out, state, model, gains = fake, fake + (1 << 24), fake + (2 << 24), fake + (1 << 28), fake + (1 << 28) + 64
    names = ['src', 'src_dtype', 'out', 'out_dtype', 'state', 'state_dtype', 'width', 'height', 'pattern', 'model', 'gains', 'radius', 't_lo', 't_hi', 'pixel_c2',
             'n_max', 'v_min', 'stream']
    args = [src, F32, out, F16, state, F32, w, h, RGGB, model, gains, 2, 1.5, 3.0, 16.0, 8.0, 1e-12, None]

    def rejected(word, **change):
        a = list(args)
        for k, v in change.items():
            a[names.index(k)] = v
        return lib.tdk_temporal_denoise(*a) == 1 and word in lib.tdk_last_error() and b'tdk_temporal_denoise' in lib.tdk_last_error()

    for k in ('src', 'out', 'state', 'model'):
        assert rejected(b'null pointer', **{k: None}), k
    for k in ('src_dtype', 'out_dtype', 'state_dtype'):
        for v in (U8, U16, -1):
            assert rejected(b'dtype', **{k: v}), (k, v)
    for k in ('width', 'height'):
        for v in (0, -2, 65536):
            assert rejected(b'frame size', **{k: v}), (k, v)
        for v in (641, 65535):
            assert rejected(b'even', **{k: v}), (k, v)
    assert rejected(b'Bayer pattern', pattern=0x12345678) and rejected(b'Bayer pattern', pattern=0)
    for v in (1, 0, 4, -2):
        assert rejected(b'radius', radius=v), v
    nan, inf = float('nan'), float('inf')
    for lo, hi in ((0.0, 3.0), (-1.0, 3.0), (3.0, 3.0), (3.0, 1.5), (nan, 3.0), (1.5, nan), (1.5, inf), (1e-40, 2e-40)):   # the last: 1 / (t_hi - t_lo) is not finite
        assert rejected(b'thresholds', t_lo=lo, t_hi=hi), (lo, hi)
    for v in (0.0, -1.0, nan, -inf):
        assert rejected(b'pixel_c2', pixel_c2=v), v
    for v in (0.0, 0.999, 64.5, -3.0, nan, inf):
        assert rejected(b'n_max', n_max=v), v
    for v in (0.0, -1e-12, nan, inf):
        assert rejected(b'v_min', v_min=v), v
    for off in (4, 8, 1):
        assert rejected(b'aligned to 16', state=state + off), off
    state_bytes = lib.tdk_temporal_state_bytes(w, h, F32)
    assert rejected(b'src, out and state overlap', out=src + 64) and rejected(b'src, out and state overlap', out=src)
    assert rejected(b'src, out and state overlap', src=out + w * h * 2 - 4)
    assert rejected(b'src, out and state overlap', state=src + 16) and rejected(b'src, out and state overlap', out=state + state_bytes - 2)
    assert rejected(b'src, out and state overlap', src=state + state_bytes - 16)
    assert rejected(b'the model or the gains overlap', model=out + 16) and rejected(b'the model or the gains overlap', model=state + 32)
    assert rejected(b'the model or the gains overlap', gains=out + w * h * 2 - 4) and rejected(b'the model or the gains overlap', gains=state)
    assert rejected(b'null pointer', src=None, gains=None)   # gains may be NULL, src may not


def test_reset_invalid_arguments_fail_on_the_host(td):
    from torch_darktable._native import lib

    assert lib.tdk_temporal_reset(None, None) == 1 and b'tdk_temporal_reset: null pointer' in lib.tdk_last_error()
    for off in (1, 4, 8):
        assert lib.tdk_temporal_reset((1 << 30) + off, None) == 1 and b'tdk_temporal_reset: state must be aligned to 16' in lib.tdk_last_error()


def test_state_and_lds_queries(td):
    from torch_darktable._native import lib

    sb, lb = lib.tdk_temporal_state_bytes, lib.tdk_temporal_lds_bytes
    for w, h, dtype in ((0, 4, F32), (4, 0, F32), (3, 4, F32), (4, 5, F32), (65536, 4, F32), (4, 65536, F32), (4, 4, U8), (4, 4, -1), (-2, 4, F16)):
        assert sb(w, h, dtype) == 0, (w, h, dtype)
    for w, h in ((2, 2), (6, 4), (2, 6), (62, 34), (4096, 3072), (65534, 65534)):
        for dtype, np_dtype in ((F32, np.float32), (F16, np.float16)):
            pa, pc = spec.align16(w * h * np.dtype(np_dtype).itemsize), spec.align16(w * h * 2)
            assert sb(w, h, dtype) == 16 + 2 * pa + 2 * pc == spec.state_bytes(w, h, np_dtype), (w, h, dtype)
    assert sb(2, 2, F32) == 16 + 2 * 16 + 2 * 16 and sb(2, 2, F16) == 16 + 4 * 16   # 8 bytes of a plane take 16
    for bad in (0, 1, 4, -2):
        assert lb(bad) == 0, bad
    assert (lb(2), lb(3)) == (lds(2), lds(3)) == (39168, 41344)
    assert lb(3) <= 64 * 1024 and 4 * lb(2) <= 160 * 1024 and 3 * lb(3) <= 160 * 1024   # four and three workgroups share a compute unit


def test_package_exports_temporal(td):
    import torch
    import torch_darktable

    assert torch_darktable.TemporalDenoise is torch_darktable.temporal.TemporalDenoise
    assert {'TemporalDenoise', 'temporal'} <= set(torch_darktable.__all__)
    assert torch_darktable.temporal.__all__ == ['TemporalDenoise']
    assert torch_darktable.TemporalDenoise.TILE == (TW, TH)
    for name in ('process', 'prepare', 'reset', 'state', 'frames', 'state_bytes', 'lds_bytes'):
        assert callable(getattr(torch_darktable.TemporalDenoise, name)), name
    assert isinstance(torch_darktable.TemporalDenoise.noise_model, property) and torch_darktable.TemporalDenoise.noise_model.fset is not None
    params = inspect.signature(torch_darktable.TemporalDenoise.__init__).parameters
    assert list(params) == ['self', 'device', 'image_size', 'bayer_pattern', 'noise_model', 'radius', 'thresholds', 'pixel_threshold', 'max_frames',
                            'variance_floor', 'state_dtype']
    assert [params[k].default for k in list(params)[5:]] == [2, (1.5, 3.0), 4.0, 8.0, 1e-12, torch.float32]
    params = inspect.signature(torch_darktable.TemporalDenoise.process).parameters
    assert list(params) == ['self', 'mosaic', 'key', 'gains', 'out_dtype'] and [params[k].default for k in ('key', 'gains', 'out_dtype')] == [None, None, None]
    assert list(inspect.signature(torch_darktable.TemporalDenoise.prepare).parameters) == ['self', 'keys']
    assert inspect.signature(torch_darktable.TemporalDenoise.reset).parameters['key'].default is ...
    for name in ('state', 'frames'):
        assert list(inspect.signature(getattr(torch_darktable.TemporalDenoise, name)).parameters) == ['self', 'key']
    assert 'raw mosaics only' in torch_darktable.temporal.__doc__


def test_pipeline_takes_a_temporal_denoiser(td):
    import torch
    from torch_darktable.pipeline import CameraSettings, ImageProcessingSettings, ImageProcessor

    params = inspect.signature(ImageProcessor.__init__).parameters
    names = list(params)
    # directly behind storage_dtype and in front of exposure: the tests of the earlier stages pin the order from exposure on
    assert names[names.index('storage_dtype') + 1:names.index('exposure')] == ['temporal'] and params['temporal'].default is None
    dev = torch.device('cuda', 0)
    build = lambda **kw: ImageProcessor((64, 48), td.BayerPattern.RGGB, td.PackedFormat.Packed12, ImageProcessingSettings(), dev, None, **kw)
    model = td.NoiseModel.from_values(2e-4, 1e-6, torch.device('cpu'))
    for wrong in (object(), model, 'temporal'):
        with pytest.raises(TypeError, match='temporal must be a TemporalDenoise'):
            build(temporal=wrong)
    with pytest.raises(ValueError, match='temporal is for'):
        build(temporal=td.TemporalDenoise(dev, (64, 50), td.BayerPattern.RGGB, model))
    with pytest.raises(ValueError, match='temporal is for'):
        build(temporal=td.TemporalDenoise(dev, (64, 48), td.BayerPattern.BGGR, model))
    assert 'temporal' not in inspect.signature(ImageProcessor.from_camera_settings).parameters
    for settings in (ImageProcessingSettings, CameraSettings):
        assert not {'temporal', 'temporal_denoise', 'max_frames'} & set(settings.model_fields), settings
    assert inspect.signature(ImageProcessor.load_image).parameters['image_name'].default is None


def test_python_front_end_validates_without_a_device(td):
    import torch

    cuda, cpu = torch.device('cuda', 0), torch.device('cpu')   # a device object only: nothing below needs a GPU
    P = td.BayerPattern.GRBG
    model = td.NoiseModel.from_values((2e-4, 5e-5, 1e-3), 1e-6, cpu)
    with pytest.raises(ValueError, match='CUDA'):
        td.TemporalDenoise(cpu, (64, 48), P, model)
    for size in ((0, 48), (64, 0), (65536, 48)):
        with pytest.raises(ValueError, match='dimensions'):
            td.TemporalDenoise(cuda, size, P, model)
    for size in ((63, 48), (64, 47)):
        with pytest.raises(ValueError, match='even'):
            td.TemporalDenoise(cuda, size, P, model)
    with pytest.raises(ValueError, match='bayer pattern'):
        td.TemporalDenoise(cuda, (64, 48), 'RGGB', model)
    for wrong in (None, (2e-4, 1e-6), model.model):
        with pytest.raises(TypeError, match='noise_model must be a NoiseModel'):
            td.TemporalDenoise(cuda, (64, 48), P, wrong)
    for radius in (1, 4, 0, 2.5, True):
        with pytest.raises(ValueError, match='radius'):
            td.TemporalDenoise(cuda, (64, 48), P, model, radius=radius)
    for thresholds in ((0.0, 3.0), (3.0, 3.0), (3.0, 1.5), (1.5,), (1.5, 2.0, 3.0), (float('nan'), 3.0), (1.5, float('inf')), (-1.0, 2.0)):
        with pytest.raises(ValueError, match='thresholds'):
            td.TemporalDenoise(cuda, (64, 48), P, model, thresholds=thresholds)
    for pixel_threshold in (0.0, -4.0, float('nan'), float('inf'), 1e-30):
        with pytest.raises(ValueError, match='pixel_threshold'):
            td.TemporalDenoise(cuda, (64, 48), P, model, pixel_threshold=pixel_threshold)
    for max_frames in (0, 0.5, 65, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='max_frames'):
            td.TemporalDenoise(cuda, (64, 48), P, model, max_frames=max_frames)
    for variance_floor in (0.0, -1e-12, float('nan'), float('inf'), 1e-60):
        with pytest.raises(ValueError, match='variance_floor'):
            td.TemporalDenoise(cuda, (64, 48), P, model, variance_floor=variance_floor)
    for state_dtype in (torch.float64, torch.uint16, torch.bfloat16):
        with pytest.raises(ValueError, match='state_dtype'):
            td.TemporalDenoise(cuda, (64, 48), P, model, state_dtype=state_dtype)

    # what the object tells: the float32 numbers the kernel is given
    t = td.TemporalDenoise(cuda, (64, 48), P, model, radius=3, thresholds=(1.2, 2.7), pixel_threshold=3.3, max_frames=12, variance_floor=1e-10,
                           state_dtype=torch.float16)
    assert t.image_size == (64, 48) and t.bayer_pattern == P and t.radius == 3 and t.state_dtype == torch.float16
    assert t.thresholds == (float(np.float32(1.2)), float(np.float32(2.7))) and t.pixel_threshold == float(np.float32(3.3))
    assert t.max_frames == 12.0 and t.variance_floor == float(np.float32(1e-10))
    assert t._c2 == float(np.float32(3.3) * np.float32(3.3))
    assert t.lds_bytes() == lds(3) and t.state_bytes() == 16 + 4 * 64 * 48 * 2
    assert td.TemporalDenoise(cuda, (62, 34), P, model).state_bytes() == spec.state_bytes(62, 34)
    assert td.TemporalDenoise(cuda, (64, 48), P, model, pixel_threshold=None)._c2 == float('inf')
    assert repr(t) == 'TemporalDenoise(64x48, GRBG, radius=3, thresholds=(1.2, 2.7), pixel_threshold=3.3, max_frames=12, state_dtype=torch.float16)'
    assert t.noise_model is model
    other = td.NoiseModel.from_values(1e-4, 0.0, cpu)
    t.noise_model = other
    assert t.noise_model is other
    with pytest.raises(TypeError, match='noise_model must be a NoiseModel'):
        t.noise_model = other.model
    with pytest.raises(RuntimeError, match='shape'):
        t.process(torch.zeros(48, 64, 1))
    with pytest.raises(RuntimeError, match='shape'):
        t.process(torch.zeros(64, 48))
    with pytest.raises(ValueError, match='out_dtype'):
        t.process(torch.zeros(48, 64), out_dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='CUDA'):
        t.process(torch.zeros(48, 64))   # no CPU fallback
    with pytest.raises(KeyError, match='no state for key'):
        t.reset(key='never seen')
