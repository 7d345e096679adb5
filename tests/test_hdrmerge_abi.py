"""CPU-only: the header include/tdk_hip_hdr.h (exposure-bracket merge) -- it parses to exactly its three declarations (exports and the
ctypes table: tests/test_header_abi.py), every argument error of tdk_hdr_merge is reported on the host before any HIP call, the LDS
query gives the documented size, and the Python front-end torch_darktable.HdrMerge and the pipeline hook exist and validate their
arguments without a device."""

import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import hdrmerge_spec as spec
from abi_header import declarations

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / 'include' / 'tdk_hip_hdr.h'
EXPECTED = ['tdk_hdr_abi_version', 'tdk_hdr_lds_bytes', 'tdk_hdr_merge']
F32, F16, U8, U16 = 0, 1, 2, 3
RGGB = 0x94949494
TW, TH = spec.TILE


def test_header_declares_the_hdr_surface(td):
    from torch_darktable import _native

    decls = declarations(HEADER)
    assert sorted(decls) == EXPECTED
    text = HEADER.read_text()
    for define in ('TDK_HDR_ABI_VERSION 1', f'TDK_HDR_TILE_W {TW}', f'TDK_HDR_TILE_H {TH}', 'TDK_HDR_MAX_FRAMES 8'):
        assert re.search(rf'#define {re.escape(define)}(?!\d)', text), define
    assert '#include "tdk_hip.h"' in text and '#include "tdk_hip_noise.h"' in text and 'extern "C"' in text
    assert decls['tdk_hdr_merge'] == ('int', ['const void* const* frames', 'int num_frames', 'int src_dtype', 'void* out', 'int out_dtype', 'unsigned char* mask',
                                              'int width', 'int height', 'uint32_t pattern', 'const float* exposures', 'int ref', 'const float* model', 'int radius',
                                              'float clip', 'float t_lo', 'float t_hi', 'float pixel_c2', 'float v_min', 'tdk_stream_t stream'])
    assert decls['tdk_hdr_lds_bytes'] == ('size_t', ['int radius'])
    assert decls['tdk_hdr_abi_version'] == ('int', [])
    for formula in ('e_min = exposures[lo];   k_f = exposures[f] / e_min', 'ref == -1 selects ref = hi', 'c_f(q)   = !(x_f < clip)', 'the 3 x 3 around q',
                    'g = ref if !sat_ref(q)', 'else blown(q): g = lo', 'R = x_g / k_g',
                    'm_f = fmaxf(R, 0) * k_f;   var_f = fmaxf(a * m_f + b, v_min);   u_f = var_f / (k_f * k_f)', 'd = r_f - R;   eps = d * d;   v = u_f + u_g',
                    'a site with sat_f(q), blown(q) or g(q) == f contributes eps = 0, v = 0', 't   = E / V', 's_f = fminf(fmaxf((t_hi - t) * inv, 0), 1)',
                    'if (eps > c2 * v) s_f = 0', 'invalid row: s_f = 1;     s_g = 1', 'w_f = sat_f(q) ? 0 : s_f / u_f', 'out = (den > 0) ? num / den : R',
                    'g | (blown ? 8 : 0) | (count of f with w_f > 0) << 4', 'an invalid row uses a = 1, b = 0', 'a sliding sum has other bits',
                    'raw mosaics only', 'Decisions the issue left open', 'HOST array'):
        assert formula in text, formula
    assert (_native.TDK_HDR_TILE_W, _native.TDK_HDR_TILE_H, _native.TDK_HDR_MAX_FRAMES) == (TW, TH, 8) == (*spec.TILE, spec.MAX_FRAMES)
    assert _native.ABI_VERSIONS['tdk_hdr_abi_version'] == (1, 'hdr ABI')
    assert _native.lib.tdk_hdr_abi_version() == 1
    rows = [row for row in _native.HEADERS if row[0] == 'tdk_hip_hdr.h']
    assert rows == [('tdk_hip_hdr.h', _native.HDR_SIGNATURES, 'tdk_hdr_abi_version', 1, 'hdr ABI')]


def test_merge_invalid_arguments_fail_on_the_host(td):
    from torch_darktable._native import lib

    fake = 1 << 30   # never dereferenced: every check below happens before anything touches device memory or a device
    w, h, nf = 640, 480, 3
    step = 1 << 24   # more than a float32 frame
    out, mask, exposures, model = fake + 8 * step, fake + 9 * step, fake + 10 * step, fake + 10 * step + 64
    frame_at = [fake + f * step for f in range(8)]
    names = ['frames', 'num_frames', 'src_dtype', 'out', 'out_dtype', 'mask', 'width', 'height', 'pattern', 'exposures', 'ref', 'model', 'radius', 'clip', 't_lo',
             't_hi', 'pixel_c2', 'v_min', 'stream']

    def call(frames=frame_at, **change):
        args = [(ctypes.c_void_p * len(frames))(*frames) if frames is not None else None, nf, F32, out, F16, mask, w, h, RGGB, exposures, -1, model, 2, 0.95, 1.5, 3.0, 16.0, 1e-12, None]
        for k, v in change.items():
            args[names.index(k)] = v
        return lib.tdk_hdr_merge(*args)

    def rejected(word, frames=frame_at, **change):
        return call(frames, **change) == 1 and word in lib.tdk_last_error() and b'tdk_hdr_merge' in lib.tdk_last_error()

    assert rejected(b'null pointer', frames=None)
    for k in ('out', 'exposures', 'model'):
        assert rejected(b'null pointer', **{k: None}), k
    for f in range(nf):
        assert rejected(b'null pointer (frame', frames=[None if i == f else p for i, p in enumerate(frame_at)]), f
    for v in (1, 0, 9, -1):
        assert rejected(b'num_frames', num_frames=v), v
    for k in ('src_dtype', 'out_dtype'):
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
    for v in (-2, 3, 8):
        assert rejected(b'ref', ref=v), v
    nan, inf = float('nan'), float('inf')
    for v in (0.0, -1.0, nan, inf):
        assert rejected(b'clip', clip=v), v
    for lo, hi in ((0.0, 3.0), (-1.0, 3.0), (3.0, 3.0), (3.0, 1.5), (nan, 3.0), (1.5, nan), (1.5, inf), (1e-40, 2e-40)):   # the last: 1 / (t_hi - t_lo) is not finite
        assert rejected(b'thresholds', t_lo=lo, t_hi=hi), (lo, hi)
    for v in (0.0, -1.0, nan, -inf):
        assert rejected(b'pixel_c2', pixel_c2=v), v
    for v in (0.0, -1e-12, nan, inf):
        assert rejected(b'v_min', v_min=v), v
    for f in range(nf):
        assert rejected(b'overlaps frame', out=frame_at[f] + 64) and rejected(b'overlaps frame', mask=frame_at[f] + w * h * 4 - 1), f
        assert rejected(b'overlaps frame', frames=[out + w * h * 2 - 2 if i == f else p for i, p in enumerate(frame_at)]), f
    assert rejected(b'the exposures or the model overlap', exposures=out + 16) and rejected(b'the exposures or the model overlap', model=mask + w * h - 1)
    assert rejected(b'the exposures or the model overlap', exposures=mask - 4 * nf + 1) and rejected(b'the exposures or the model overlap', model=out + w * h * 2 - 4)
    assert rejected(b'out and mask overlap', mask=out + w * h * 2 - 1) and rejected(b'out and mask overlap', mask=out)
    assert rejected(b'null pointer', out=None, mask=None)   # mask may be NULL, out may not


def test_lds_query(td):
    from torch_darktable._native import lib

    for bad in (0, 1, 4, -2):
        assert lib.tdk_hdr_lds_bytes(bad) == 0, bad
    assert (lib.tdk_hdr_lds_bytes(2), lib.tdk_hdr_lds_bytes(3)) == (spec.lds_bytes(2), spec.lds_bytes(3)) == (22352, 23584)
    assert 2 * lib.tdk_hdr_lds_bytes(3) <= 160 * 1024 and lib.tdk_hdr_lds_bytes(3) <= 64 * 1024


def test_package_exports_hdrmerge(td):
    import torch_darktable

    assert torch_darktable.HdrMerge is torch_darktable.hdrmerge.HdrMerge
    assert {'HdrMerge', 'hdrmerge'} <= set(torch_darktable.__all__)
    assert torch_darktable.hdrmerge.__all__ == ['HdrMerge']
    assert torch_darktable.HdrMerge.TILE == (TW, TH) and torch_darktable.HdrMerge.MAX_FRAMES == 8
    params = inspect.signature(torch_darktable.HdrMerge.__init__).parameters
    assert list(params) == ['self', 'device', 'image_size', 'bayer_pattern', 'noise_model', 'radius', 'clip', 'thresholds', 'pixel_threshold', 'variance_floor']
    assert [params[k].default for k in list(params)[5:]] == [2, 0.95, (1.5, 3.0), 4.0, 1e-12]
    temporal = inspect.signature(torch_darktable.TemporalDenoise.__init__).parameters   # the same statistic, the same defaults
    assert all(params[k].default == temporal[k].default for k in ('radius', 'thresholds', 'pixel_threshold', 'variance_floor'))
    params = inspect.signature(torch_darktable.HdrMerge.process).parameters
    assert list(params) == ['self', 'frames', 'exposures', 'ref', 'out_dtype', 'return_mask']
    assert [params[k].default for k in ('ref', 'out_dtype', 'return_mask')] == [None, None, False]
    assert isinstance(torch_darktable.HdrMerge.noise_model, property) and torch_darktable.HdrMerge.noise_model.fset is not None
    assert 'raw mosaics only' in torch_darktable.hdrmerge.__doc__


def test_pipeline_takes_a_bracket_merge(td):
    import torch
    from torch_darktable.pipeline import CameraSettings, ImageProcessingSettings, ImageProcessor

    params = inspect.signature(ImageProcessor.__init__).parameters
    names = list(params)
    # directly behind padding and in front of storage_dtype: the tests of the earlier stages pin the order from storage_dtype on
    assert names[names.index('padding') + 1:names.index('storage_dtype')] == ['hdr'] and params['hdr'].default is None
    assert list(inspect.signature(ImageProcessor.process_bracket).parameters) == ['self', 'payloads', 'exposures', 'image_name', 'ref']
    dev = torch.device('cuda', 0)
    build = lambda **kw: ImageProcessor((64, 48), td.BayerPattern.RGGB, td.PackedFormat.Packed12, ImageProcessingSettings(), dev, None, **kw)
    model = td.NoiseModel.from_values(2e-4, 1e-6, torch.device('cpu'))
    for wrong in (object(), model, torch.float16):
        with pytest.raises(TypeError, match='hdr must be an HdrMerge'):
            build(hdr=wrong)
    with pytest.raises(ValueError, match='hdr is for'):
        build(hdr=td.HdrMerge(dev, (64, 50), td.BayerPattern.RGGB, model))
    with pytest.raises(ValueError, match='hdr is for'):
        build(hdr=td.HdrMerge(dev, (64, 48), td.BayerPattern.BGGR, model))
    payload = torch.zeros(64 * 48 * 3 // 2, dtype=torch.uint8)
    with pytest.raises(ValueError, match='process_bracket needs hdr'):
        build().process_bracket([payload, payload], (1.0, 0.25), 'cam')
    both = build(hdr=td.HdrMerge(dev, (64, 48), td.BayerPattern.RGGB, model), temporal=td.TemporalDenoise(dev, (64, 48), td.BayerPattern.RGGB, model))
    with pytest.raises(ValueError, match='temporal'):
        both.process_bracket([payload, payload], (1.0, 0.25), 'cam')
    assert 'hdr' not in inspect.signature(ImageProcessor.from_camera_settings).parameters
    for settings in (ImageProcessingSettings, CameraSettings):
        assert not {'hdr', 'hdr_merge', 'exposures'} & set(settings.model_fields), settings


def test_python_front_end_validates_without_a_device(td):
    import torch

    cuda, cpu = torch.device('cuda', 0), torch.device('cpu')   # a device object only: nothing below needs a GPU
    P = td.BayerPattern.GRBG
    model = td.NoiseModel.from_values((2e-4, 5e-5, 1e-3), 1e-6, cpu)
    with pytest.raises(ValueError, match='CUDA'):
        td.HdrMerge(cpu, (64, 48), P, model)
    for size in ((0, 48), (64, 0), (65536, 48)):
        with pytest.raises(ValueError, match='dimensions'):
            td.HdrMerge(cuda, size, P, model)
    for size in ((63, 48), (64, 47)):
        with pytest.raises(ValueError, match='even'):
            td.HdrMerge(cuda, size, P, model)
    with pytest.raises(ValueError, match='bayer pattern'):
        td.HdrMerge(cuda, (64, 48), 'RGGB', model)
    for wrong in (None, (2e-4, 1e-6), model.model):
        with pytest.raises(TypeError, match='noise_model must be a NoiseModel'):
            td.HdrMerge(cuda, (64, 48), P, wrong)
    for radius in (1, 4, 0, 2.5, True):
        with pytest.raises(ValueError, match='radius'):
            td.HdrMerge(cuda, (64, 48), P, model, radius=radius)
    for clip in (0.0, -0.5, float('nan'), float('inf'), 1e-60):
        with pytest.raises(ValueError, match='clip'):
            td.HdrMerge(cuda, (64, 48), P, model, clip=clip)
    for thresholds in ((0.0, 3.0), (3.0, 3.0), (3.0, 1.5), (1.5,), (1.5, 2.0, 3.0), (float('nan'), 3.0), (1.5, float('inf')), (-1.0, 2.0)):
        with pytest.raises(ValueError, match='thresholds'):
            td.HdrMerge(cuda, (64, 48), P, model, thresholds=thresholds)
    for pixel_threshold in (0.0, -4.0, float('nan'), float('inf'), 1e-30):
        with pytest.raises(ValueError, match='pixel_threshold'):
            td.HdrMerge(cuda, (64, 48), P, model, pixel_threshold=pixel_threshold)
    for variance_floor in (0.0, -1e-12, float('nan'), float('inf'), 1e-60):
        with pytest.raises(ValueError, match='variance_floor'):
            td.HdrMerge(cuda, (64, 48), P, model, variance_floor=variance_floor)

    # what the object tells: the float32 numbers the kernel is given
    t = td.HdrMerge(cuda, (64, 48), P, model, radius=3, clip=0.9, thresholds=(1.2, 2.7), pixel_threshold=3.3, variance_floor=1e-10)
    assert t.image_size == (64, 48) and t.bayer_pattern == P and t.radius == 3 and t.clip == float(np.float32(0.9))
    assert t.thresholds == (float(np.float32(1.2)), float(np.float32(2.7))) and t.pixel_threshold == float(np.float32(3.3))
    assert t.variance_floor == float(np.float32(1e-10)) and t._c2 == float(np.float32(3.3) * np.float32(3.3))
    assert t.lds_bytes() == spec.lds_bytes(3)
    assert td.HdrMerge(cuda, (64, 48), P, model, pixel_threshold=None)._c2 == float('inf')
    assert repr(t) == 'HdrMerge(64x48, GRBG, radius=3, clip=0.9, thresholds=(1.2, 2.7), pixel_threshold=3.3)'
    assert t.noise_model is model
    with pytest.raises(TypeError, match='noise_model must be a NoiseModel'):
        t.noise_model = model.model
    frame = torch.zeros(48, 64)
    with pytest.raises(ValueError, match='2..8 frames'):
        t.process([frame], (1.0,))
    with pytest.raises(ValueError, match='2..8 frames'):
        t.process([frame] * 9, (1.0,) * 9)
    with pytest.raises(RuntimeError, match='shape'):
        t.process([frame, torch.zeros(64, 48)], (1.0, 0.5))
    with pytest.raises(RuntimeError, match='stacked'):
        t.process(torch.zeros(48, 64), (1.0, 0.5))
    with pytest.raises(ValueError, match='out_dtype'):
        t.process([frame, frame], (1.0, 0.5), out_dtype=torch.uint8)
    for ref in (-1, 2, 0.5, True):
        with pytest.raises(ValueError, match='ref'):
            t.process([frame, frame], (1.0, 0.5), ref=ref)
    for exposures in ((1.0, 0.0), (1.0, -0.5), (float('nan'), 1.0), (1.0, float('inf')), (1.0, 1e-60), (1.0,), (1.0, 0.5, 0.25)):
        with pytest.raises(ValueError, match='exposures'):
            t.process([frame, frame], exposures)
    with pytest.raises(RuntimeError, match='exposures must be a contiguous'):
        t.process([frame, frame], torch.ones(3))
    with pytest.raises(RuntimeError, match='CUDA'):
        t.process([frame, frame], (1.0, 0.5))   # no CPU fallback
    with pytest.raises(RuntimeError, match='CUDA'):
        t.process(torch.zeros(2, 48, 64), (1.0, 0.5))
