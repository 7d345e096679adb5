"""CPU-only: the fifth header include/tdk_hip_warp.h (parametric warp) -- it parses to exactly its four declarations
(exports and the ctypes table: tests/test_header_abi.py), every argument error of tdk_warp is
reported on the host before any HIP call and names its argument, the LDS query stays within 64 KB, and the Python front-end
torch_darktable.Warp builds the maps the issue describes and raises the error types of Resize."""

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from abi_header import declarations

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / 'include' / 'tdk_hip_warp.h'
EXPECTED = ['tdk_warp', 'tdk_warp_abi_version', 'tdk_warp_coordinates', 'tdk_warp_lds_bytes']
F32, F16, U8 = 0, 1, 2
IDENTITY = [1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]


def test_header_declares_the_warp_surface(td):
    from torch_darktable import _native

    decls = declarations(HEADER)
    assert sorted(decls) == EXPECTED
    text = HEADER.read_text()
    assert re.search(r'#define TDK_WARP_ABI_VERSION 1\b', text) and re.search(r'#define TDK_WARP_DIRECT 1\b', text)
    assert '#include "tdk_hip_resample.h"' in text and 'extern "C"' in text and '#define TDK_U8' not in text   # TDK_U8 is the scaler's
    assert decls['tdk_warp'] == ('int', ['const void* src', 'void* dst', 'int src_width', 'int src_height', 'int dst_width', 'int dst_height',
                                         'int channels', 'int dtype', 'const float* map', 'int interp', 'int border', 'float fill', 'int flags',
                                         'tdk_stream_t stream'])
    assert decls['tdk_warp_coordinates'] == ('int', ['float* xy', 'int dst_width', 'int dst_height', 'const float* map', 'tdk_stream_t stream'])
    assert decls['tdk_warp_lds_bytes'] == ('size_t', ['int channels', 'int dtype', 'int interp'])
    for formula in ('X = (h0*u + h1*v) + h2', 'iz = 1.0f / Z', 'rad = ((k3*r2 + k2)*r2 + k1)*r2 + 1.0f', 'tx = p1*(xy + xy) + p2*(r2 + (x2 + x2))',
                    'ty = p1*(r2 + (y2 + y2)) + p2*(xy + xy)', 'xd = x*rad + tx', 'sx = fx*xd + cx', 'sx = min(max(sx, -4), sw + 3)',
                    'c1(t) = ((1.25f*t - 2.25f)*t)*t + 1.0f', 'c2(t) = ((-0.75f*t + 3.75f)*t - 6.0f)*t + 3.0f', '((s0*w0 + s1*w1) + s2*w2) + s3*w3'):
        assert formula in text, formula
    assert _native.TDK_WARP_DIRECT == 1 and _native.TDK_U8 == U8
    assert _native.ABI_VERSIONS['tdk_warp_abi_version'] == (1, 'warp ABI')


def test_warp_invalid_arguments_fail_on_the_host(td):
    from torch_darktable._native import lib

    fake = 1 << 20   # never dereferenced: every check below happens before anything touches device memory or a device
    good = (ctypes.c_float * 18)(*IDENTITY)
    names = ['src', 'dst', 'sw', 'sh', 'dw', 'dh', 'c', 'dtype', 'map', 'interp', 'border', 'fill', 'flags', 'stream']
    args = [fake, fake + (1 << 24), 64, 48, 16, 12, 3, F32, ctypes.addressof(good), 1, 0, 0.0, 0, None]

    def call(**change):
        a = list(args)
        for k, v in change.items():
            a[names.index(k)] = v
        return lib.tdk_warp(*a)

    def failed(word):
        return word in lib.tdk_last_error()

    for k in ('src', 'dst', 'map'):
        assert call(**{k: None}) == 1 and failed(b'null pointer') and failed(k.encode()), k
    for k in ('sw', 'sh'):
        for v in (0, -3, 65536):
            assert call(**{k: v}) == 1 and failed(b'source size'), (k, v)
    for k in ('dw', 'dh'):
        for v in (0, -3, 65536):
            assert call(**{k: v}) == 1 and failed(b'destination size'), (k, v)
    for c in (0, 2, 4):
        assert call(c=c) == 1 and failed(b'channels'), c
    for d in (3, -1):
        assert call(dtype=d) == 1 and failed(b'dtype'), d
    for v in (2, -1):
        assert call(interp=v) == 1 and failed(b'interp'), v
        assert call(border=v) == 1 and failed(b'border'), v
    for v in (2, -1, 3):
        assert call(flags=v) == 1 and failed(b'flags'), v
    for k in range(18):
        for bad in (float('nan'), float('inf'), -float('inf')):
            m = (ctypes.c_float * 18)(*IDENTITY)
            m[k] = bad
            assert call(map=ctypes.addressof(m)) == 1 and failed(f'map[{k}]'.encode()), (k, bad)
    for bad in (float('nan'), float('inf')):
        assert call(fill=bad) == 1 and failed(b'fill'), bad
    # overlap, in bytes of the dtype: the same pointer, dst inside src, src inside dst, and the last byte
    src_bytes = 64 * 48 * 3 * 4
    for dst in (fake, fake + 64, fake - 16 * 12 * 3 * 4 + 4, fake + src_bytes - 4):
        assert call(dst=dst) == 1 and failed(b'overlap'), dst
    assert call(dst=fake + src_bytes // 4, dtype=U8, sw=640, sh=480) == 1 and failed(b'overlap')

    cnames = ['xy', 'dw', 'dh', 'map', 'stream']
    cargs = [fake, 16, 12, ctypes.addressof(good), None]

    def coords(**change):
        a = list(cargs)
        for k, v in change.items():
            a[cnames.index(k)] = v
        return lib.tdk_warp_coordinates(*a)

    for k in ('xy', 'map'):
        assert coords(**{k: None}) == 1 and failed(b'null pointer') and failed(k.encode()), k
    for k in ('dw', 'dh'):
        for v in (0, 65536):
            assert coords(**{k: v}) == 1 and failed(b'destination size'), (k, v)
    m = (ctypes.c_float * 18)(*IDENTITY)
    m[13] = float('nan')
    assert coords(map=ctypes.addressof(m)) == 1 and failed(b'map[13]')


def test_lds_query_stays_within_64_kb(td):
    from torch_darktable._native import lib

    q = lib.tdk_warp_lds_bytes
    for c in (1, 3):
        for dtype in (F32, F16, U8):
            for interp in (0, 1):
                assert 0 < q(c, dtype, interp) <= 65536, (c, dtype, interp)
    for bad in ((0, F32, 0), (2, F32, 0), (4, F16, 1), (3, 3, 0), (3, -1, 1), (3, U8, 2), (1, F32, -1)):
        assert q(*bad) == 0, bad


def test_package_exports_warp(td):
    import torch_darktable

    assert torch_darktable.Warp is torch_darktable.warp.Warp
    assert 'Warp' in torch_darktable.__all__ and 'warp' in torch_darktable.__all__
    assert torch_darktable.warp.__all__ == ['Warp']
    for name in ('process', 'coordinates', 'undistort', 'homography', 'from_transform'):
        assert callable(getattr(torch_darktable.Warp, name)), name


def test_undistort_builds_the_inverse_of_knew_r(td):
    import torch

    cuda = torch.device('cuda', 0)   # a device object only: nothing below reaches the GPU
    K = np.array([[2950.0, 0, 2040.3], [0, 2946.0, 1507.7], [0, 0, 1]])
    Knew = np.array([[2400.0, 0, 1999.5], [0, 2400.0, 1499.5], [0, 0, 1]])
    a = np.deg2rad(3.0)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    dist = [-0.12, 0.09, 8e-4, -5e-4, -0.02]
    wp = td.Warp.undistort(cuda, (4096, 3000), K, dist, new_camera_matrix=Knew, rectify=R, output_size=(4000, 2900), interpolation='bilinear',
                           border='replicate')
    m = wp.map
    assert m.dtype == np.float32 and m.shape == (18,)
    assert np.array_equal(m[:9], np.linalg.inv(Knew @ R).reshape(-1).astype(np.float32))   # float64 on the host, rounded once
    assert np.array_equal(m[9:13], np.array([2950.0, 2946.0, 2040.3, 1507.7], dtype=np.float32))
    assert np.array_equal(m[13:], np.array(dist, dtype=np.float32))
    assert (wp.input_size, wp.output_size) == ((4096, 3000), (4000, 2900))
    assert repr(wp) == 'Warp(4096x3000 -> 4000x2900, bilinear, replicate)'
    # the defaults: new_camera_matrix = camera_matrix, R = I, output_size = size, k3 = 0 with four coefficients
    wp = td.Warp.undistort(cuda, (4096, 3000), K, dist[:4])
    assert np.array_equal(wp.map[:9], np.linalg.inv(K).reshape(-1).astype(np.float32)) and wp.map[17] == 0 and wp.output_size == (4096, 3000)
    assert repr(wp) == 'Warp(4096x3000 -> 4096x3000, bicubic, constant, fill=0)'
    for n in (3, 6, 8, 14):
        with pytest.raises(ValueError, match='dist_coeffs'):
            td.Warp.undistort(cuda, (4096, 3000), K, [0.0] * n)
    hm = td.Warp.homography(cuda, (64, 48), (32, 24), np.eye(3)).map
    assert np.array_equal(hm, np.array(IDENTITY, dtype=np.float32))
    wp.map[0] = 5.0   # a copy: the object keeps its values
    assert wp.map[0] != 5.0


def test_python_front_end_raises_the_error_types_of_resize(td):
    import torch

    cuda = torch.device('cuda', 0)
    with pytest.raises(ValueError, match='CUDA'):
        td.Warp(torch.device('cpu'), (64, 48), (16, 12), IDENTITY)
    for size in ((0, 48), (64, -1), (65536, 48)):
        with pytest.raises(ValueError, match='Input dimensions'):
            td.Warp(cuda, size, (16, 12), IDENTITY)
        with pytest.raises(ValueError, match='Output dimensions'):
            td.Warp(cuda, (64, 48), size, IDENTITY)
    with pytest.raises(ValueError, match='18'):
        td.Warp(cuda, (64, 48), (16, 12), IDENTITY[:17])
    with pytest.raises(ValueError, match='finite'):
        td.Warp(cuda, (64, 48), (16, 12), [float('nan')] + IDENTITY[1:])
    with pytest.raises(ValueError, match='finite'):
        td.Warp(cuda, (64, 48), (16, 12), [1e39] + IDENTITY[1:])   # finite in float64, not in float32
    with pytest.raises(ValueError, match='fill'):
        td.Warp(cuda, (64, 48), (16, 12), IDENTITY, fill=float('inf'))
    with pytest.raises(ValueError, match='interpolation'):
        td.Warp(cuda, (64, 48), (16, 12), IDENTITY, interpolation='nearest')
    with pytest.raises(ValueError, match='border'):
        td.Warp(cuda, (64, 48), (16, 12), IDENTITY, border='reflect')
    wp = td.Warp(cuda, (64, 48), (16, 12), IDENTITY)
    assert 0 < wp.lds_bytes(3, torch.uint8) <= 65536 and wp.lds_bytes(2, torch.uint8) == 0 and wp.lds_bytes(3, torch.int32) == 0
    with pytest.raises(RuntimeError, match='shape'):
        wp.process(torch.zeros(48, 60, 3))
    with pytest.raises(RuntimeError, match='shape'):
        wp.process(torch.zeros(64, 48, 3))
    with pytest.raises(ValueError, match='channels'):
        wp.process(torch.zeros(48, 64, 2))
    with pytest.raises(ValueError, match='channels'):
        wp.process(torch.zeros(48, 64, 4))
    with pytest.raises(RuntimeError, match='CUDA'):
        wp.process(torch.zeros(48, 64, 3))   # no CPU fallback
    with pytest.raises(RuntimeError, match='CUDA'):
        wp.process(torch.zeros(48, 64, 3, dtype=torch.uint8))
