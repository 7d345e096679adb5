"""CPU-only: the seventh header include/tdk_hip_sharpen.h (unsharp mask) -- it parses to exactly its four declarations
(exports and the ctypes table: tests/test_header_abi.py), every argument error of tdk_sharpen is
reported on the host before any HIP call, the LDS query stays within (0, 64 KB] over every legal (channels, dtype, radius, flags),
and the Python front-end torch_darktable.Sharpen and the pipeline hook exist and raise the error types of Resize."""

import ctypes
import re
from pathlib import Path

import pytest

from abi_header import declarations

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / 'include' / 'tdk_hip_sharpen.h'
EXPECTED = ['tdk_sharpen', 'tdk_sharpen_abi_version', 'tdk_sharpen_lds_bytes', 'tdk_sharpen_weights']
F32, F16, U8 = 0, 1, 2
LUMA, LIMIT = 1, 2


def test_header_declares_the_sharpen_surface(td):
    from torch_darktable import _native

    decls = declarations(HEADER)
    assert sorted(decls) == EXPECTED
    text = HEADER.read_text()
    assert re.search(r'#define TDK_SHARPEN_ABI_VERSION 1\b', text)
    assert re.search(r'#define TDK_SHARPEN_LUMA 1\b', text) and re.search(r'#define TDK_SHARPEN_LIMIT 2\b', text)
    assert re.search(r'#define TDK_SHARPEN_MAX_RADIUS 12\b', text)
    assert '#include "tdk_hip.h"' in text and 'extern "C"' in text
    assert decls['tdk_sharpen'] == ('int', ['const void* src', 'void* dst', 'int width', 'int height', 'int channels', 'int dtype', 'const float* weights',
                                            'int radius', 'float amount', 'float threshold', 'float overshoot', 'int flags', 'tdk_stream_t stream'])
    assert decls['tdk_sharpen_weights'] == ('int', ['float sigma', 'float* weights', 'int* radius'])
    assert decls['tdk_sharpen_lds_bytes'] == ('size_t', ['int channels', 'int dtype', 'int radius', 'int flags'])
    for formula in ('s = (0.2126729f*r + 0.7151522f*g) + 0.0721750f*b', 'h = w[0]*s[0]', 'h = h + w[k]*(s[-k] + s[+k])', 'd  = s - b',
                    "d' = |d| > t ? copysignf(|d| - t, d) : 0", "y[c] = x[c] + amount * d'", 'y[c] = fminf(fmaxf(y[c], lo[c] - o), hi[c] + o)'):
        assert formula in text, formula
    assert (_native.TDK_SHARPEN_LUMA, _native.TDK_SHARPEN_LIMIT, _native.TDK_SHARPEN_MAX_RADIUS) == (LUMA, LIMIT, 12)
    assert _native.ABI_VERSIONS['tdk_sharpen_abi_version'] == (1, 'sharpen ABI')


def test_sharpen_invalid_arguments_fail_on_the_host(td):
    from torch_darktable._native import lib

    fake = 1 << 20   # never dereferenced: every check below happens before anything touches device memory or a device
    good = (ctypes.c_float * 13)(0.4, 0.2, 0.1, *([0.0] * 10))
    names = ['src', 'dst', 'w', 'h', 'c', 'dtype', 'weights', 'radius', 'amount', 'threshold', 'overshoot', 'flags', 'stream']
    args = [fake, fake + (1 << 24), 64, 48, 3, F32, good, 2, 0.5, 0.0, 0.0, 0, None]

    def call(**change):
        a = list(args)
        for k, v in change.items():
            a[names.index(k)] = v
        return lib.tdk_sharpen(*a)

    for k in ('src', 'dst', 'weights'):
        assert call(**{k: None}) == 1 and b'null pointer' in lib.tdk_last_error(), k
    for k in ('w', 'h'):
        for v in (0, -3, 65536):
            assert call(**{k: v}) == 1 and b'frame size' in lib.tdk_last_error(), (k, v)
    for c in (0, 2, 4):
        assert call(c=c) == 1 and b'channels' in lib.tdk_last_error(), c
    for d in (3, -1):
        assert call(dtype=d) == 1 and b'dtype' in lib.tdk_last_error(), d
    for r in (0, -1, 13):
        assert call(radius=r) == 1 and b'radius' in lib.tdk_last_error(), r
    for bad in (-0.1, float('nan'), float('inf')):
        for k in range(3):
            w = (ctypes.c_float * 13)(*good)
            w[k] = bad
            assert call(weights=w) == 1 and b'weights[%d]' % k in lib.tdk_last_error(), (k, bad)
    beyond = (ctypes.c_float * 13)(*good)
    beyond[3] = float('nan')                       # past radius: never read
    assert call(weights=beyond, dtype=7) == 1 and b'dtype' in lib.tdk_last_error()
    for v in (-0.001, 16.001, float('nan'), float('inf')):
        assert call(amount=v) == 1 and b'amount' in lib.tdk_last_error(), v
    for v in (-0.001, float('nan'), float('inf')):
        assert call(threshold=v) == 1 and b'threshold' in lib.tdk_last_error(), v
        assert call(overshoot=v, flags=LIMIT) == 1 and b'overshoot' in lib.tdk_last_error(), v
    for f in (4, 8, -1, 7):
        assert call(flags=f) == 1 and b'flags' in lib.tdk_last_error(), f
    for f in (LUMA, LUMA | LIMIT):
        assert call(c=1, flags=f) == 1 and b'TDK_SHARPEN_LUMA needs three channels' in lib.tdk_last_error(), f
    # overlap, in bytes of the dtype: the same pointer, dst inside src, src inside dst, and the last byte
    nbytes = 64 * 48 * 3 * 4
    for dst in (fake, fake + 64, fake - nbytes + 4, fake + nbytes - 4):
        assert call(dst=dst) == 1 and b'overlap' in lib.tdk_last_error(), dst
    assert call(dst=fake + nbytes // 4 - 1, dtype=U8) == 1 and b'overlap' in lib.tdk_last_error()


def test_lds_query_stays_within_64_kb(td):
    from torch_darktable._native import lib

    q = lib.tdk_sharpen_lds_bytes
    for bad in ((0, F32, 3, 0), (2, F32, 3, 0), (4, F32, 3, 0), (3, 3, 3, 0), (3, -1, 3, 0), (3, F32, 0, 0), (3, F32, 13, 0), (3, F32, -2, 0),
                (3, F32, 3, 4), (3, F32, 3, -1), (1, F32, 3, LUMA), (1, U8, 3, LUMA | LIMIT)):
        assert q(*bad) == 0, bad
    worst = 0
    for c in (1, 3):
        for dtype in (F32, F16, U8):
            for r in range(1, 13):
                for flags in (0, LIMIT) + ((LUMA, LUMA | LIMIT) if c == 3 else ()):
                    b = q(c, dtype, r, flags)
                    signals = 1 if (flags & LUMA) or c == 1 else 3
                    assert b == 4 * signals * (32 + 2 * r) * ((32 + 2 * r) + 32), (c, dtype, r, flags, b)   # the two planes of DESIGN.md 3.8
                    assert 0 < b <= 65536, (c, dtype, r, flags, b)
                    worst = max(worst, b)
    print(f'tdk_sharpen_lds_bytes: at most {worst} bytes')
    assert worst == 59136
    assert 4 * q(3, U8, 3, LUMA) <= 160 * 1024     # the pipeline's call (sigma 1, uint8, luminance): four workgroups per CU and more


def test_package_exports_sharpen(td):
    import torch_darktable

    assert torch_darktable.Sharpen is torch_darktable.sharpen.Sharpen
    assert 'Sharpen' in torch_darktable.__all__ and 'sharpen' in torch_darktable.__all__
    assert torch_darktable.sharpen.__all__ == ['Sharpen']
    assert callable(torch_darktable.Sharpen.process) and callable(torch_darktable.Sharpen.from_weights)
    from torch_darktable import torch_darktable_extension as ext   # its extra exports are a closed list: nothing of the sharpener
    assert not any('sharpen' in n.lower() for n in dir(ext))


def test_pipeline_takes_a_sharpener_and_the_settings_stay_pinned(td):
    import inspect

    from torch_darktable.pipeline import ImageProcessingSettings, ImageProcessor

    p = inspect.signature(ImageProcessor.__init__).parameters['sharpen']
    assert p.default is None
    import torch
    from torch_darktable.pipeline import ImageProcessingSettings as S
    with pytest.raises(TypeError, match='sharpen must be a Sharpen'):
        ImageProcessor((64, 48), td.BayerPattern.RGGB, td.PackedFormat.Packed12, S(), torch.device('cuda', 0), None, sharpen=object())
    assert 'sharpen' not in inspect.signature(ImageProcessor.from_camera_settings).parameters
    assert not any('sharpen' in name for name in ImageProcessingSettings.model_fields)


def test_python_front_end_raises_the_error_types_of_resize(td):
    import torch

    cuda = torch.device('cuda', 0)   # a device object only: nothing below reaches the GPU
    with pytest.raises(ValueError, match='CUDA'):
        td.Sharpen(torch.device('cpu'))
    with pytest.raises(ValueError, match='CUDA'):
        td.Sharpen.from_weights(torch.device('cpu'), (0.5, 0.25))
    for sigma in (0.2, 4.5, 0.0, -1.0, float('nan')):
        with pytest.raises(ValueError, match='sigma'):
            td.Sharpen(cuda, sigma=sigma)
    for amount in (-0.5, 16.5, float('nan')):
        with pytest.raises(ValueError, match='amount'):
            td.Sharpen(cuda, amount=amount)
    for v in (-0.01, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='threshold'):
            td.Sharpen(cuda, threshold=v)
        with pytest.raises(ValueError, match='overshoot'):
            td.Sharpen(cuda, overshoot=v)
    for weights in ((1.0,), (), tuple([0.01] * 14)):
        with pytest.raises(ValueError, match='weights must hold'):
            td.Sharpen.from_weights(cuda, weights)
    for weights in ((0.5, -0.25), (0.5, float('nan')), (float('inf'), 0.1)):
        with pytest.raises(ValueError, match='finite'):
            td.Sharpen.from_weights(cuda, weights)

    s = td.Sharpen(cuda)
    assert (s.sigma, s.radius, s.amount, s.threshold, s.luma, s.overshoot) == (1.0, 3, 0.5, 0.0, True, None)
    assert len(s.weights) == 4 and isinstance(s.weights, tuple) and td.Sharpen.TILE == (32, 32)
    assert repr(s) == 'Sharpen(sigma=1, radius=3, amount=0.5, threshold=0, luma=True, overshoot=None)'
    c = td.Sharpen.from_weights(cuda, (0.5, 0.25), amount=2.0, luma=False, overshoot=0.0)
    assert (c.sigma, c.radius, c.weights, c.amount, c.luma, c.overshoot) == (None, 1, (0.5, 0.25), 2.0, False, 0.0)
    # luminance is dropped for one channel; the LDS query follows the flags process would pass
    assert s.lds_bytes(3, torch.uint8) == 4 * 38 * 70 and s.lds_bytes(1, torch.uint8) == 4 * 38 * 70
    assert td.Sharpen(cuda, luma=False).lds_bytes(3, torch.float16) == 3 * 4 * 38 * 70
    assert s.lds_bytes(2, torch.uint8) == 0 and s.lds_bytes(3, torch.int32) == 0
    assert td.Sharpen(cuda, sigma=4.0, luma=False, overshoot=0.1).lds_bytes(3, torch.float32) == 59136

    with pytest.raises(AssertionError, match='3 dimensions'):
        s.process(torch.zeros(48, 64))
    with pytest.raises(ValueError, match='channels'):
        s.process(torch.zeros(48, 64, 2))
    with pytest.raises(ValueError, match='channels'):
        s.process(torch.zeros(48, 64, 4))
    with pytest.raises(ValueError, match='dimensions'):
        s.process(torch.zeros(0, 64, 3))
    with pytest.raises(RuntimeError, match='CUDA'):
        s.process(torch.zeros(48, 64, 3))   # no CPU fallback
    with pytest.raises(RuntimeError, match='CUDA'):
        s.process(torch.zeros(48, 64, 1, dtype=torch.uint8))
