"""CPU-only: the header include/tdk_hip_motion.h (motion estimation and the compensated temporal denoiser) -- it parses to exactly its
five declarations (exports and the ctypes table: tests/test_header_abi.py), every argument error of its three entry points is reported
on the host before any HIP call, the pyramid query gives the documented size, and the Python front-end torch_darktable.MotionEstimate
and torch_darktable.MotionTemporalDenoise exist and validate their arguments without a device."""

import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import motion_spec as spec
from abi_header import declarations

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / 'include' / 'tdk_hip_motion.h'
EXPECTED = ['tdk_motion_abi_version', 'tdk_motion_match', 'tdk_motion_pyramid', 'tdk_motion_pyramid_bytes', 'tdk_motion_temporal_denoise']
F32, F16, U8, U16 = 0, 1, 2, 3
RGGB = 0x94949494
FAKE = 1 << 30   # never dereferenced: every check happens before anything touches device memory or a device


def test_header_declares_the_motion_surface(td):
    from torch_darktable import _native

    decls = declarations(HEADER)
    assert sorted(decls) == EXPECTED
    text = HEADER.read_text()
    for define in ('TDK_MOTION_ABI_VERSION 1', 'TDK_MOTION_TILE_W 64', 'TDK_MOTION_TILE_H 32', 'TDK_MOTION_MAX_LEVELS 4', 'TDK_MOTION_MAX_SEARCH 4',
                   'TDK_MOTION_MAX_DISPLACEMENT 78', 'TDK_MOTION_MAX_ZERO_BIAS 65535'):
        assert re.search(rf'#define {re.escape(define)}(?!\d)', text), define
    assert '#include "tdk_hip.h"' in text and '#include "tdk_hip_temporal.h"' in text and 'extern "C"' in text
    assert decls['tdk_motion_abi_version'] == ('int', [])
    assert decls['tdk_motion_pyramid_bytes'] == ('size_t', ['int width', 'int height', 'int levels'])
    assert decls['tdk_motion_pyramid'] == ('int', ['const void* src', 'int src_dtype', 'int width', 'int height', 'float scale', 'int levels', 'void* pyramid',
                                                   'const uint32_t* index', 'int which', 'tdk_stream_t stream'])
    assert decls['tdk_motion_match'] == ('int', ['const void* pyramid_cur', 'int which_cur', 'const void* pyramid_ref', 'int which_ref', 'int width', 'int height',
                                                 'int levels', 'int search', 'uint32_t zero_bias', 'const uint32_t* index', 'int16_t* field', 'uint32_t* costs',
                                                 'tdk_stream_t stream'])
    temporal = declarations(ROOT / 'include' / 'tdk_hip_temporal.h')['tdk_temporal_denoise'][1]
    assert decls['tdk_motion_temporal_denoise'] == ('int', temporal[:-1] + ['const int16_t* field', 'tdk_stream_t stream'])   # every argument of the plain filter
    for formula in ('q = (x00 + x01) + (x10 + x11)', 'u = fminf(fmaxf(q * scale, 0), 1)', 'g = (uint8)(sqrtf(u) * 255 + 0.5f)', '(a + b + c + d + 2) >> 2',
                    'SLOT = P(0) + ... + P(K-1)', 'tdk_motion_pyramid_bytes = 2 * SLOT', 'c = ((16 ty + 8) >> k, (32 tx + 16) >> k)',
                    'key = cost << 14 | (oy*oy + ox*ox) << 8 | (oy + 4) << 4 | (ox + 4)', 'base = 2 * d(k + 1)', 'if (cost(w) + zero_bias >= cost(0)) the result is 0',
                    '(dy, dx) = field[i / 32][j / 64] & ~1', 'h = q + (dy, dx)', 'With a zero field the function is tdk_temporal_denoise bit for bit',
                    '(idx + which) & 1', 'Decisions the issue left open'):
        assert formula in text, formula
    assert (_native.TDK_MOTION_TILE_W, _native.TDK_MOTION_TILE_H) == (_native.TDK_TEMPORAL_TILE_W, _native.TDK_TEMPORAL_TILE_H) == (64, 32)
    assert (_native.TDK_MOTION_MAX_LEVELS, _native.TDK_MOTION_MAX_SEARCH, _native.TDK_MOTION_MAX_DISPLACEMENT, _native.TDK_MOTION_MAX_ZERO_BIAS) == (4, 4, 78, 65535)
    assert _native.ABI_VERSIONS['tdk_motion_abi_version'] == (1, 'motion ABI') and _native.lib.tdk_motion_abi_version() == 1
    rows = [row for row in _native.HEADERS if row[0] == 'tdk_hip_motion.h']
    assert rows == [('tdk_hip_motion.h', _native.MOTION_SIGNATURES, 'tdk_motion_abi_version', 1, 'motion ABI')]


def rejecter(fn, who, names, args):
    from torch_darktable._native import lib

    def rejected(word, **change):
        a = list(args)
        for k, v in change.items():
            a[names.index(k)] = v
        return fn(*a) == 1 and word in lib.tdk_last_error() and who in lib.tdk_last_error()
    return rejected


def test_pyramid_invalid_arguments_fail_on_the_host(td):
    from torch_darktable._native import lib

    w, h = 640, 480
    names = ['src', 'src_dtype', 'width', 'height', 'scale', 'levels', 'pyramid', 'index', 'which', 'stream']
    rejected = rejecter(lib.tdk_motion_pyramid, b'tdk_motion_pyramid', names, [FAKE, F32, w, h, 0.25, 3, FAKE + (1 << 24), FAKE + (2 << 24), 0, None])
    for k in ('src', 'pyramid'):
        assert rejected(b'null pointer', **{k: None}), k
    for v in (U8, U16, -1):
        assert rejected(b'dtype', src_dtype=v), v
    for k in ('width', 'height'):
        for v in (0, -2, 65536):
            assert rejected(b'frame size', **{k: v}), (k, v)
        for v in (641, 65535):
            assert rejected(b'even', **{k: v}), (k, v)
    for v in (0.0, -0.25, float('nan'), float('inf')):
        assert rejected(b'scale', scale=v), v
    for v in (0, 5, -1):
        assert rejected(b'levels', levels=v), v
    for v in (2, -1):
        assert rejected(b'which', which=v), v
    for off in (1, 4, 8):
        assert rejected(b'pyramid must be aligned to 16', pyramid=FAKE + (1 << 24) + off), off
    for off in (1, 2):
        assert rejected(b'index must be aligned to 4', index=FAKE + (2 << 24) + off), off
    bytes_ = lib.tdk_motion_pyramid_bytes(w, h, 3)
    assert rejected(b'src and pyramid overlap', pyramid=FAKE + 16) and rejected(b'src and pyramid overlap', src=FAKE + (1 << 24) + bytes_ - 4)
    assert rejected(b'null pointer', src=None, index=None)   # index may be NULL, src may not


def test_match_invalid_arguments_fail_on_the_host(td):
    from torch_darktable._native import lib

    w, h = 640, 480
    names = ['pyramid_cur', 'which_cur', 'pyramid_ref', 'which_ref', 'width', 'height', 'levels', 'search', 'zero_bias', 'index', 'field', 'costs', 'stream']
    cur, ref, field, costs = FAKE, FAKE + (1 << 24), FAKE + (2 << 24), FAKE + (3 << 24)
    rejected = rejecter(lib.tdk_motion_match, b'tdk_motion_match', names, [cur, 0, ref, 1, w, h, 3, 4, 300, FAKE + (4 << 24), field, costs, None])
    for k in ('pyramid_cur', 'pyramid_ref', 'field'):
        assert rejected(b'null pointer', **{k: None}), k
    for k in ('width', 'height'):
        for v in (0, -2, 65536):
            assert rejected(b'frame size', **{k: v}), (k, v)
        assert rejected(b'even', **{k: 641}), k
    for v in (0, 5, -1):
        assert rejected(b'levels', levels=v) and rejected(b'search', search=v), v
    for v in (65536, 0xFFFFFFFF):
        assert rejected(b'zero_bias', zero_bias=v), v
    for k in ('which_cur', 'which_ref'):
        for v in (2, -1):
            assert rejected(b'which_cur and which_ref', **{k: v}), (k, v)
    for k, base in (('pyramid_cur', cur), ('pyramid_ref', ref)):
        assert rejected(b'pyramids must be aligned to 16', **{k: base + 8}), k
    assert rejected(b'index must be aligned to 4', index=FAKE + (4 << 24) + 2)
    assert rejected(b'field must be aligned to 4', field=field + 2) and rejected(b'costs must be aligned to 8', costs=costs + 4)
    tiles = 10 * 15
    assert rejected(b'overlap', field=cur + 16) and rejected(b'overlap', field=ref + 32) and rejected(b'overlap', costs=cur + 64) and rejected(b'overlap', costs=ref)
    assert rejected(b'overlap', costs=field + 8) and rejected(b'overlap', costs=field + tiles * 4 - 4 - (tiles * 4 - 4) % 8)
    assert rejected(b'null pointer', field=None, costs=None, index=None)   # costs and index may be NULL, field may not
    # one buffer for both pyramids is the normal case
    assert not rejected(b'overlap', pyramid_ref=cur, levels=0) and rejected(b'levels', pyramid_ref=cur, levels=0)


def test_compensated_filter_invalid_arguments_fail_on_the_host(td):
    from torch_darktable._native import lib

    w, h = 640, 480
    src, out, state, model, gains, field = FAKE, FAKE + (1 << 24), FAKE + (2 << 24), FAKE + (1 << 28), FAKE + (1 << 28) + 64, FAKE + (1 << 27)
    names = ['src', 'src_dtype', 'out', 'out_dtype', 'state', 'state_dtype', 'width', 'height', 'pattern', 'model', 'gains', 'radius', 't_lo', 't_hi', 'pixel_c2',
             'n_max', 'v_min', 'field', 'stream']
    rejected = rejecter(lib.tdk_motion_temporal_denoise, b'tdk_motion_temporal_denoise', names,
                        [src, F32, out, F16, state, F32, w, h, RGGB, model, gains, 2, 1.5, 3.0, 16.0, 8.0, 1e-12, field, None])
    for k in ('src', 'out', 'state', 'model', 'field'):
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
    for lo, hi in ((0.0, 3.0), (-1.0, 3.0), (3.0, 3.0), (3.0, 1.5), (nan, 3.0), (1.5, nan), (1.5, inf), (1e-40, 2e-40)):
        assert rejected(b'thresholds', t_lo=lo, t_hi=hi), (lo, hi)
    for v in (0.0, -1.0, nan, -inf):
        assert rejected(b'pixel_c2', pixel_c2=v), v
    for v in (0.0, 0.999, 64.5, -3.0, nan, inf):
        assert rejected(b'n_max', n_max=v), v
    for v in (0.0, -1e-12, nan, inf):
        assert rejected(b'v_min', v_min=v), v
    for off in (4, 8, 1):
        assert rejected(b'state must be aligned to 16', state=state + off), off
    for off in (1, 2):
        assert rejected(b'field must be aligned to 4', field=field + off), off
    state_bytes = lib.tdk_temporal_state_bytes(w, h, F32)
    assert rejected(b'src, out and state overlap', out=src + 64) and rejected(b'src, out and state overlap', state=src + 16)
    assert rejected(b'src, out and state overlap', src=state + state_bytes - 16)
    assert rejected(b'the model or the gains overlap', model=out + 16) and rejected(b'the model or the gains overlap', gains=state)
    assert rejected(b'the field overlaps', field=out + 16) and rejected(b'the field overlaps', field=state + state_bytes - 4) and rejected(b'the field overlaps', field=state)
    assert rejected(b'null pointer', src=None, gains=None)   # gains may be NULL, src may not


def test_pyramid_bytes_query(td):
    from torch_darktable._native import lib

    pb = lib.tdk_motion_pyramid_bytes
    for w, h, levels in ((0, 4, 3), (4, 0, 3), (3, 4, 3), (4, 5, 3), (65536, 4, 3), (4, 65536, 3), (4, 4, 0), (4, 4, 5), (-2, 4, 1)):
        assert pb(w, h, levels) == 0, (w, h, levels)
    for w, h in ((2, 2), (6, 4), (66, 34), (130, 70), (198, 150), (4096, 3072), (65534, 65534)):
        for levels in (1, 2, 3, 4):
            assert pb(w, h, levels) == spec.pyramid_bytes(w, h, levels), (w, h, levels)
    assert pb(2, 2, 4) == 128 and pb(66, 34, 4) == 1600 and pb(64, 32, 1) == 2 * 512
    assert pb(4096, 3072, 3) == 2 * (2048 * 1536 + 1024 * 768 + 512 * 384)


def test_package_exports_motion(td):
    import torch
    import torch_darktable as t

    assert t.MotionEstimate is t.motion.MotionEstimate and t.MotionTemporalDenoise is t.motion.MotionTemporalDenoise
    assert {'MotionEstimate', 'MotionTemporalDenoise', 'motion'} <= set(t.__all__)
    assert t.motion.__all__ == ['MotionEstimate', 'MotionTemporalDenoise']
    assert issubclass(t.MotionTemporalDenoise, t.TemporalDenoise) and t.MotionEstimate.TILE == t.TemporalDenoise.TILE == (64, 32)
    assert t.motion.DEFAULT_ZERO_BIAS == spec.DEFAULT_ZERO_BIAS == 300
    params = inspect.signature(t.MotionEstimate.__init__).parameters
    assert list(params) == ['self', 'device', 'image_size', 'levels', 'search', 'zero_bias', 'white_level']
    assert [params[k].default for k in list(params)[3:]] == [3, 4, 300, 1.0]
    params = inspect.signature(t.MotionEstimate.estimate).parameters
    assert list(params) == ['self', 'cur', 'ref', 'return_costs'] and params['return_costs'].default is False
    params = inspect.signature(t.MotionTemporalDenoise.__init__).parameters
    assert list(params)[:6] == ['self', 'device', 'image_size', 'bayer_pattern', 'noise_model', 'motion'] and params['motion'].default is None
    assert inspect.signature(t.MotionTemporalDenoise.process) == inspect.signature(t.TemporalDenoise.process)   # the same signature
    assert inspect.signature(t.MotionTemporalDenoise.prepare) == inspect.signature(t.TemporalDenoise.prepare)
    for name in ('field', 'costs'):
        assert list(inspect.signature(getattr(t.MotionTemporalDenoise, name)).parameters) == ['self', 'key']
    for name in ('reset', 'state', 'frames', 'state_bytes', 'lds_bytes'):
        assert getattr(t.MotionTemporalDenoise, name) is getattr(t.TemporalDenoise, name), name
    assert 'raw mosaics only' in t.motion.__doc__
    assert torch.uint32 is not None


def test_python_front_end_validates_without_a_device(td):
    import torch

    cuda, cpu = torch.device('cuda', 0), torch.device('cpu')   # a device object only: nothing below needs a GPU
    with pytest.raises(ValueError, match='CUDA'):
        td.MotionEstimate(cpu, (64, 48))
    for size in ((0, 48), (64, 0), (65536, 48)):
        with pytest.raises(ValueError, match='dimensions'):
            td.MotionEstimate(cuda, size)
    for size in ((63, 48), (64, 47)):
        with pytest.raises(ValueError, match='even'):
            td.MotionEstimate(cuda, size)
    for levels in (0, 5, 2.5, True, None):
        with pytest.raises(ValueError, match='levels'):
            td.MotionEstimate(cuda, (64, 48), levels=levels)
    for search in (0, 5, 1.5, True):
        with pytest.raises(ValueError, match='search'):
            td.MotionEstimate(cuda, (64, 48), search=search)
    for zero_bias in (-1, 65536, 2.0, True):
        with pytest.raises(ValueError, match='zero_bias'):
            td.MotionEstimate(cuda, (64, 48), zero_bias=zero_bias)
    for white in (0.0, -1.0, float('nan'), float('inf'), 1e-40):
        with pytest.raises(ValueError, match='white_level'):
            td.MotionEstimate(cuda, (64, 48), white_level=white)

    me = td.MotionEstimate(cuda, (198, 150), levels=4, search=2, zero_bias=17, white_level=4095.0)
    assert me.image_size == (198, 150) and me.tiles == (5, 4) and (me.levels, me.search, me.zero_bias) == (4, 2, 17)
    assert me.max_displacement == 2 * (3 * 8 - 1) == spec.max_displacement(4, 2) and td.MotionEstimate(cuda, (64, 48)).max_displacement == 38
    assert td.MotionEstimate(cuda, (64, 48), levels=4).max_displacement == 78
    assert me.scale == float(spec.scale_of(4095.0)) and td.MotionEstimate(cuda, (64, 48)).scale == 0.25
    assert me.pyramid_bytes() == spec.pyramid_bytes(198, 150, 4) and me.level_sizes() == spec.level_sizes(198, 150, 4)
    assert me.level_offsets() == spec.level_offsets(198, 150, 4)
    assert repr(me) == 'MotionEstimate(198x150, levels=4, search=2, zero_bias=17, white_level=4095)'
    with pytest.raises(RuntimeError, match='shape'):
        me.estimate(torch.zeros(198, 150), torch.zeros(150, 198))
    with pytest.raises(RuntimeError, match='CUDA'):
        me.estimate(torch.zeros(150, 198), torch.zeros(150, 198))   # no CPU fallback

    P = td.BayerPattern.GRBG
    model = td.NoiseModel.from_values((2e-4, 5e-5, 1e-3), 1e-6, cpu)
    for wrong in (object(), 'motion', model):
        with pytest.raises(TypeError, match='motion must be a MotionEstimate'):
            td.MotionTemporalDenoise(cuda, (198, 150), P, model, motion=wrong)
    with pytest.raises(ValueError, match='motion is for'):
        td.MotionTemporalDenoise(cuda, (64, 48), P, model, motion=me)
    with pytest.raises(ValueError, match='radius'):   # every check of TemporalDenoise
        td.MotionTemporalDenoise(cuda, (198, 150), P, model, motion=me, radius=4)
    with pytest.raises(TypeError, match='noise_model must be a NoiseModel'):
        td.MotionTemporalDenoise(cuda, (198, 150), P, None, motion=me)
    mt = td.MotionTemporalDenoise(cuda, (198, 150), P, model, motion=me, radius=3, max_frames=12, state_dtype=torch.float16)
    assert isinstance(mt, td.TemporalDenoise) and mt.motion is me and mt.radius == 3 and mt.max_frames == 12.0 and mt.state_dtype == torch.float16
    assert mt.state_bytes() == 16 + 4 * ((198 * 150 * 2 + 15) // 16 * 16)
    assert td.MotionTemporalDenoise(cuda, (64, 48), P, model).motion.max_displacement == 38   # a default estimator
    assert repr(mt).startswith('MotionTemporalDenoise(198x150, GRBG, radius=3') and repr(mt).endswith(f'motion={me!r})')
    with pytest.raises(RuntimeError, match='shape'):
        mt.process(torch.zeros(198, 150))
    with pytest.raises(ValueError, match='out_dtype'):
        mt.process(torch.zeros(150, 198), out_dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='CUDA'):
        mt.process(torch.zeros(150, 198))
    with pytest.raises(KeyError, match='no state for key'):
        mt.reset(key='never seen')


def test_pipeline_takes_a_compensated_denoiser(td):
    import torch
    from torch_darktable.pipeline import ImageProcessingSettings, ImageProcessor

    dev = torch.device('cuda', 0)
    model = td.NoiseModel.from_values(2e-4, 1e-6, torch.device('cpu'))
    build = lambda **kw: ImageProcessor((64, 48), td.BayerPattern.RGGB, td.PackedFormat.Packed12, ImageProcessingSettings(), dev, None, **kw)
    with pytest.raises(ValueError, match='temporal is for'):
        build(temporal=td.MotionTemporalDenoise(dev, (64, 50), td.BayerPattern.RGGB, model))
