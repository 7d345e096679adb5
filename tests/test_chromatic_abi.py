"""CPU-only: the header include/tdk_hip_ca.h (lateral chromatic aberration) -- it parses to exactly its five declarations (exports and
the ctypes table: tests/test_header_abi.py), every argument error of tdk_ca_correct and tdk_ca_estimate is reported on the host before
any HIP call, the queries give the documented sizes, and the Python front-end torch_darktable.ChromaticAberration and the pipeline hook
exist and validate their arguments without a device."""

import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import chromatic_spec as spec
from abi_header import declarations

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / 'include' / 'tdk_hip_ca.h'
EXPECTED = ['tdk_ca_abi_version', 'tdk_ca_correct', 'tdk_ca_estimate', 'tdk_ca_lds_bytes', 'tdk_ca_workspace_bytes']
F32, F16, U8, U16 = 0, 1, 2, 3
RGGB = 0x94949494


def test_header_declares_the_ca_surface(td):
    from torch_darktable import _native

    decls = declarations(HEADER)
    assert sorted(decls) == EXPECTED
    text = HEADER.read_text()
    for define in ('TDK_CA_ABI_VERSION 1', 'TDK_CA_MAX_SHIFT 8', 'TDK_CA_TILE_W 64', 'TDK_CA_TILE_H 32', 'TDK_CA_MAX_FRAMES 16', 'TDK_CA_QMAX 65535', 'TDK_CA_SUMS 17',
                   'TDK_CA_MIN_SITES 16', 'TDK_CA_BILINEAR 0', 'TDK_CA_BICUBIC 1', 'TDK_CA_LINEAR 0', 'TDK_CA_POLY3 1'):
        assert re.search(rf'#define {re.escape(define)}(?!\d)', text), define
    assert '#define TDK_CA_QSCALE 65535.0f' in text
    assert '#include "tdk_hip.h"' in text and '#include "tdk_hip_noise.h"' in text and 'extern "C"' in text
    assert decls['tdk_ca_correct'] == ('int', ['const void* src', 'int src_dtype', 'void* out', 'int out_dtype', 'int width', 'int height', 'uint32_t pattern',
                                               'const float* model', 'float x0', 'float y0', 'float rn', 'int interp', 'tdk_stream_t stream'])
    assert decls['tdk_ca_estimate'] == ('int', ['const void* const* frames', 'int num_frames', 'int src_dtype', 'int width', 'int height', 'uint32_t pattern',
                                                'const float* noise_model', 'int fit', 'float clip', 'int block', 'float max_shift', 'float x0', 'float y0', 'float rn',
                                                'void* workspace', 'float* model', 'tdk_stream_t stream'])
    assert decls['tdk_ca_lds_bytes'] == ('size_t', ['int interp', 'int src_dtype'])
    assert decls['tdk_ca_workspace_bytes'] == ('size_t', ['int width', 'int height', 'int block'])
    for formula in ('q = c0 + (p - c0) * s_k(rho),   rho = |p - c0| / rn,   s_k = v + c*rho + b*rho^2', 's = (b*rho + c)*rho + v;   t = s - 1.0f',
                    'dx = px*t;   dy = py*t', 'if dx or dy is not finite: dx = dy = 0', 'u = (float)(j >> 1) + dx*0.5f', 'Why D is fixed', 'Tile shape',
                    'G4 = gl + gr + gu + gd;   gx2 = gr - gl;   gy2 = gd - gu', 'N00 = c11/16  N01 = c12/8  N02 = c13/8  N11 = c22/4  N12 = c23/4  N22 = c33/4',
                    'N00 -= nv/4, N11 -= nv/2, N22 -= nv/2', 'det = (N00*C00 + N01*C01) + N02*C02', 'dx = mx / kappa;   dy = my / kappa;   wx = det / C11;   wy = det / C22',
                    'g = (wx*cx)*cx + (wy*cy)*cy;   h = -((wx*cx)*dx + (wy*cy)*dy)', 'exact to first order in s - 1', 'Decisions the issue left open', 'HOST',
                    'more than twice what a poor lens shows at 50 MP'):
        assert formula in text, formula
    assert (_native.TDK_CA_MAX_SHIFT, _native.TDK_CA_TILE_W, _native.TDK_CA_TILE_H, _native.TDK_CA_MAX_FRAMES) == (spec.MAX_SHIFT, *spec.TILE, spec.MAX_FRAMES) == (8, 64, 32, 16)
    assert (_native.TDK_CA_QSCALE, _native.TDK_CA_QMAX, _native.TDK_CA_SUMS, _native.TDK_CA_MIN_SITES) == (float(spec.QSCALE), spec.QMAX, spec.SUMS, spec.MIN_SITES)
    assert _native.ABI_VERSIONS['tdk_ca_abi_version'] == (1, 'chromatic aberration ABI')
    assert _native.lib.tdk_ca_abi_version() == 1
    rows = [row for row in _native.HEADERS if row[0] == 'tdk_hip_ca.h']
    assert rows == [('tdk_hip_ca.h', _native.CA_SIGNATURES, 'tdk_ca_abi_version', 1, 'chromatic aberration ABI')]


def test_correct_invalid_arguments_fail_on_the_host(td):
    from torch_darktable._native import lib

    fake = 1 << 30   # never dereferenced: every check below happens before anything touches device memory or a device
    w, h = 640, 480
    src, out, model = fake, fake + (1 << 24), fake + (1 << 25)
    names = ['src', 'src_dtype', 'out', 'out_dtype', 'width', 'height', 'pattern', 'model', 'x0', 'y0', 'rn', 'interp', 'stream']

    def rejected(word, **change):
        args = [src, F32, out, F16, w, h, RGGB, model, 319.5, 239.5, 400.0, 1, None]
        for k, v in change.items():
            args[names.index(k)] = v
        return lib.tdk_ca_correct(*args) == 1 and word in lib.tdk_last_error() and b'tdk_ca_correct' in lib.tdk_last_error()

    for k in ('src', 'out', 'model'):
        assert rejected(b'null pointer', **{k: None}), k
    for k in ('src_dtype', 'out_dtype'):
        for v in (U8, U16, -1):
            assert rejected(b'dtype', **{k: v}), (k, v)
    for k in ('width', 'height'):
        for v in (0, -2, 65536):
            assert rejected(b'frame size', **{k: v}), (k, v)
        for v in (641, 65535):
            assert rejected(b'even', **{k: v}), (k, v)
    assert rejected(b'Bayer pattern', pattern=0x12345678) and rejected(b'Bayer pattern', pattern=0)
    for v in (2, -1):
        assert rejected(b'interp', interp=v), v
    nan, inf = float('nan'), float('inf')
    for k in ('x0', 'y0'):
        for v in (nan, inf, -inf):
            assert rejected(b'centre', **{k: v}), (k, v)
    for v in (0.0, -1.0, nan, inf):
        assert rejected(b'rn', rn=v), v
    assert rejected(b'out overlaps src', out=src + 64) and rejected(b'out overlaps src', src=out + w * h * 2 - 2)
    assert rejected(b'out overlaps the model', model=out + 16) and rejected(b'out overlaps the model', model=out - 31)


def test_estimate_invalid_arguments_fail_on_the_host(td):
    from torch_darktable._native import lib

    fake = 1 << 30
    w, h, nf = 640, 480, 3
    step = 1 << 24
    frame_at = [fake + f * step for f in range(16)]
    workspace, model, noise = fake + 16 * step, fake + 17 * step, fake + 17 * step + 64
    names = ['frames', 'num_frames', 'src_dtype', 'width', 'height', 'pattern', 'noise_model', 'fit', 'clip', 'block', 'max_shift', 'x0', 'y0', 'rn', 'workspace',
             'model', 'stream']

    def rejected(word, frames=frame_at, **change):
        args = [(ctypes.c_void_p * len(frames))(*frames) if frames is not None else None, nf, F32, w, h, RGGB, noise, 0, 0.95, 64, 2.0, 319.5, 239.5, 400.0, workspace,
                model, None]
        for k, v in change.items():
            args[names.index(k)] = v
        return lib.tdk_ca_estimate(*args) == 1 and word in lib.tdk_last_error() and b'tdk_ca_estimate' in lib.tdk_last_error()

    assert rejected(b'null pointer', frames=None)
    for k in ('workspace', 'model'):
        assert rejected(b'null pointer', **{k: None}), k
    for f in range(nf):
        assert rejected(b'null pointer (frame', frames=[None if i == f else p for i, p in enumerate(frame_at)]), f
    for v in (0, 17, -1):
        assert rejected(b'num_frames', num_frames=v), v
    for v in (U8, U16, -1):
        assert rejected(b'dtype', src_dtype=v), v
    for k in ('width', 'height'):
        for v in (0, -2, 65536):
            assert rejected(b'frame size', **{k: v}), (k, v)
        for v in (641, 65535):
            assert rejected(b'even', **{k: v}), (k, v)
    assert rejected(b'Bayer pattern', pattern=0x12345678)
    for v in (2, -1):
        assert rejected(b'fit', fit=v), v
    nan, inf = float('nan'), float('inf')
    for v in (0.0, -1.0, nan, inf):
        assert rejected(b'clip', clip=v), v
    for v in (14, 15, 33, 258, 0, -64):
        assert rejected(b'block', block=v), v
    for v in (0.0, -1.0, nan, inf, 8.5):
        assert rejected(b'max_shift', max_shift=v), v
    for k in ('x0', 'y0'):
        assert rejected(b'centre', **{k: nan}), k
    for v in (0.0, -1.0, nan, inf):
        assert rejected(b'rn', rn=v), v
    ws_bytes = lib.tdk_ca_workspace_bytes(w, h, 64)
    for f in range(nf):
        assert rejected(b'overlaps frame', workspace=frame_at[f] + w * h * 4 - 1) and rejected(b'overlaps frame', model=frame_at[f] + 64), f
    assert rejected(b'workspace and model overlap', model=workspace + ws_bytes - 1) and rejected(b'workspace and model overlap', model=workspace)
    assert rejected(b'the noise model overlaps', noise_model=model + 16) and rejected(b'the noise model overlaps', noise_model=workspace + ws_bytes - 4)


def test_queries(td):
    from torch_darktable._native import lib

    for interp, dtype in ((2, F32), (-1, F32), (0, U8), (1, -1)):
        assert lib.tdk_ca_lds_bytes(interp, dtype) == 0, (interp, dtype)
    for dtype in (F32, F16):
        assert (lib.tdk_ca_lds_bytes(0, dtype), lib.tdk_ca_lds_bytes(1, dtype)) == (spec.lds_bytes(0), spec.lds_bytes(1)) == (17472, 19712)
    assert 5 * lib.tdk_ca_lds_bytes(1, F32) <= 160 * 1024
    for w, h, block in ((641, 480, 64), (640, 0, 64), (640, 480, 15), (640, 480, 258), (640, 480, 8)):
        assert lib.tdk_ca_workspace_bytes(w, h, block) == 0, (w, h, block)
    assert lib.tdk_ca_workspace_bytes(640, 480, 64) == 10 * 7 * 2 * 17 * 8
    assert lib.tdk_ca_workspace_bytes(60, 40, 64) == 16


def test_package_exports_chromatic(td):
    import torch_darktable

    CA = torch_darktable.ChromaticAberration
    assert CA is torch_darktable.chromatic.ChromaticAberration
    assert {'ChromaticAberration', 'chromatic'} <= set(torch_darktable.__all__)
    assert torch_darktable.chromatic.__all__ == ['ChromaticAberration']
    assert CA.TILE == spec.TILE and CA.MAX_SHIFT == 8 and CA.MAX_FRAMES == 16
    params = inspect.signature(CA.__init__).parameters
    assert list(params) == ['self', 'device', 'image_size', 'bayer_pattern', 'model', 'center', 'rn', 'interp']
    assert [params[k].default for k in list(params)[4:]] == [None, None, None, 'bilinear']
    params = inspect.signature(CA.correct).parameters
    assert list(params) == ['self', 'mosaic', 'model', 'out_dtype'] and [params[k].default for k in ('model', 'out_dtype')] == [None, None]
    params = inspect.signature(CA.estimate).parameters
    assert list(params) == ['self', 'mosaics', 'noise_model', 'fit', 'clip', 'block', 'max_shift']
    assert [params[k].default for k in list(params)[2:]] == [None, 'linear', 0.95, 64, 2.0]
    assert list(inspect.signature(CA.refine).parameters) == ['self', 'mosaics', 'model', 'kwargs']
    assert 'raw mosaics only' in torch_darktable.chromatic.__doc__


def test_pipeline_takes_a_chromatic_aberration(td):
    import torch
    from torch_darktable.pipeline import CameraSettings, ImageProcessingSettings, ImageProcessor

    params = inspect.signature(ImageProcessor.__init__).parameters
    names = list(params)
    # in front of padding: every slot behind it is pinned by the test of an earlier stage
    assert names[names.index('transforms') + 1:names.index('padding')] == ['chromatic'] and params['chromatic'].default is None
    dev = torch.device('cuda', 0)
    build = lambda **kw: ImageProcessor((64, 48), td.BayerPattern.RGGB, td.PackedFormat.Packed12, ImageProcessingSettings(), dev, None, **kw)
    for wrong in (object(), 16, torch.zeros(2, 4)):
        with pytest.raises(TypeError, match='chromatic must be a ChromaticAberration'):
            build(chromatic=wrong)
    with pytest.raises(ValueError, match='chromatic is for'):
        build(chromatic=td.ChromaticAberration(dev, (64, 50), td.BayerPattern.RGGB))
    with pytest.raises(ValueError, match='chromatic is for'):
        build(chromatic=td.ChromaticAberration(dev, (64, 48), td.BayerPattern.BGGR))
    assert build().chromatic is None and build(padding=16).padding == 16
    assert 'chromatic' not in inspect.signature(ImageProcessor.from_camera_settings).parameters
    for settings in (ImageProcessingSettings, CameraSettings):
        assert not {'chromatic', 'chromatic_aberration', 'ca'} & set(settings.model_fields), settings


def test_python_front_end_validates_without_a_device(td):
    import torch

    cuda, cpu = torch.device('cuda', 0), torch.device('cpu')   # a device object only: nothing below needs a GPU
    P = td.BayerPattern.GRBG
    CA = td.ChromaticAberration
    with pytest.raises(ValueError, match='CUDA'):
        CA(cpu, (64, 48), P)
    for size in ((0, 48), (64, 0), (65536, 48)):
        with pytest.raises(ValueError, match='dimensions'):
            CA(cuda, size, P)
    for size in ((63, 48), (64, 47)):
        with pytest.raises(ValueError, match='even'):
            CA(cuda, size, P)
    with pytest.raises(ValueError, match='bayer pattern'):
        CA(cuda, (64, 48), 'RGGB')
    for interp in ('cubic', 1, None):
        with pytest.raises(ValueError, match='interp'):
            CA(cuda, (64, 48), P, interp=interp)
    for center in ((1.0,), (1.0, 2.0, 3.0), (float('nan'), 1.0), (1.0, float('inf'))):
        with pytest.raises(ValueError, match='center'):
            CA(cuda, (64, 48), P, center=center)
    for rn in (0.0, -1.0, float('nan'), float('inf'), 1e-60):
        with pytest.raises(ValueError, match='rn'):
            CA(cuda, (64, 48), P, rn=rn)
    for model in (torch.zeros(3, 4), torch.zeros(2, 4, dtype=torch.float64), torch.zeros(4, 2).t(), [[1, 0, 0, 1]] * 2):
        with pytest.raises(ValueError, match='model must be'):
            CA(cuda, (64, 48), P, model=model)
    for red in ((1.0, 0.0), (1.0, 0.0, float('nan'))):
        with pytest.raises(ValueError, match='red must be'):
            CA.from_coefficients(cuda, (64, 48), P, red=red)

    # what the object tells: the float32 numbers the kernels are given
    ca = CA(cuda, (64, 48), P)
    x0, y0, rn = spec.default_geometry(64, 48)
    assert ca.image_size == (64, 48) and ca.bayer_pattern == P and ca.center == (float(x0), float(y0)) == (31.5, 23.5) and ca.rn == float(rn) and ca.model is None
    ca = CA(cuda, (64, 48), P, center=(10.1, 40.0), rn=77.7, interp='bicubic')
    assert ca.center == (float(np.float32(10.1)), 40.0) and ca.rn == float(np.float32(77.7))
    assert ca.lds_bytes() == spec.lds_bytes(spec.BICUBIC) and ca.lds_bytes(torch.uint8) == 0 and CA(cuda, (64, 48), P).lds_bytes(torch.float16) == spec.lds_bytes(spec.BILINEAR)
    assert ca.workspace_bytes(16) == 4 * 3 * 2 * 17 * 8 and ca.workspace_bytes() == 16
    assert repr(ca) == 'ChromaticAberration(64x48, GRBG, center=(10.1, 40), rn=77.7, interp=bicubic)'
    model = torch.tensor([[1.001, 0.0, 0.0, 1.0], [0.999, 0.0, 0.0, 1.0]])
    other = ca.with_model(model)
    assert other.model is model and other.center == ca.center and other.rn == ca.rn and other.interp == 'bicubic' and ca.model is None
    with pytest.raises(ValueError, match='model must be'):
        ca.model = torch.zeros(4)
    frame = torch.zeros(48, 64)
    with pytest.raises(RuntimeError, match='shape'):
        ca.correct(torch.zeros(64, 48))
    with pytest.raises(ValueError, match='out_dtype'):
        ca.correct(frame, out_dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='CUDA'):
        ca.correct(frame)   # no CPU fallback
    with pytest.raises(ValueError, match='1..16 frames'):
        ca.estimate([])
    with pytest.raises(ValueError, match='1..16 frames'):
        ca.estimate([frame] * 17)
    with pytest.raises(RuntimeError, match='shape'):
        ca.estimate([frame, torch.zeros(64, 48)])
    with pytest.raises(TypeError, match='noise_model must be a NoiseModel'):
        ca.estimate(frame, noise_model=torch.zeros(3, 4))
    with pytest.raises(ValueError, match='fit'):
        ca.estimate(frame, fit='quadratic')
    for clip in (0.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='clip'):
            ca.estimate(frame, clip=clip)
    for block in (15, 14, 258, 32.5, True):
        with pytest.raises(ValueError, match='block'):
            ca.estimate(frame, block=block)
    for max_shift in (0.0, 8.5, float('nan')):
        with pytest.raises(ValueError, match='max_shift'):
            ca.estimate(frame, max_shift=max_shift)
    with pytest.raises(RuntimeError, match='CUDA'):
        ca.estimate(frame)
