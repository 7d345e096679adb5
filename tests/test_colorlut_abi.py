"""CPU-only: the header include/tdk_hip_lut.h (colour matrix, shaper curves, 3D LUT) -- it parses to exactly its three declarations
(exports and the ctypes table: tests/test_header_abi.py), every argument error of tdk_color_lut is reported on the host before any
HIP call, the LDS query gives the bytes of the tables that are staged, and the Python front-end torch_darktable.ColorLUT and the two
pipeline hooks exist and validate their arguments without a device."""

import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

from abi_header import declarations

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / 'include' / 'tdk_hip_lut.h'
EXPECTED = ['tdk_color_lut', 'tdk_lut_abi_version', 'tdk_lut_lds_bytes']
F32, F16, U8 = 0, 1, 2
TETRA, TRILINEAR, GLOBAL = 0, 1, 1
BUDGET = 80 * 1024


def test_header_declares_the_lut_surface(td):
    from torch_darktable import _native

    decls = declarations(HEADER)
    assert sorted(decls) == EXPECTED
    text = HEADER.read_text()
    for define in ('TDK_LUT_ABI_VERSION 1', 'TDK_LUT_TETRAHEDRAL 0', 'TDK_LUT_TRILINEAR 1', 'TDK_LUT_GLOBAL 1', 'TDK_LUT_MAX_SHAPER 1024', 'TDK_LUT_MAX_SIZE 65',
                   f'TDK_LUT_LDS_BUDGET {BUDGET}'):
        assert re.search(rf'#define {define}\b', text), define
    assert '#include "tdk_hip.h"' in text and 'extern "C"' in text
    assert decls['tdk_color_lut'] == ('int', ['const void* src', 'int src_dtype', 'void* dst', 'int dst_dtype', 'int64_t npix', 'const float* matrix',
                                              'const float* shaper', 'int shaper_size', 'int shaper_tables', 'float shaper_lo', 'float shaper_scale',
                                              'const float* lut', 'int lut_size', 'const float* lut_lo', 'const float* lut_scale', 'int interp', 'int flags',
                                              'tdk_stream_t stream'])
    assert decls['tdk_lut_lds_bytes'] == ('size_t', ['int shaper_size', 'int shaper_tables', 'int lut_size', 'int flags'])
    assert decls['tdk_lut_abi_version'] == ('int', [])
    for formula in ('0x3B808081', "r' = (m0*r + m1*g) + m2*b", "g' = (m3*r + m4*g) + m5*b", "b' = (m6*r + m7*g) + m8*b",
                    't = fminf(fmaxf((x - lo) * scale, 0.0f), (float)(S-1))', 'k = min((int)t, S-2)', 'f = t - (float)k', 'y = T[k] + f*(T[k+1] - T[k])',
                    't_c = fminf(fmaxf((y_c - lo_c) * scale_c, 0.0f), (float)(N-1))', 'k_c = min((int)t_c, N-2)', 'f_c = t_c - (float)k_c',
                    '((kb*N + kg)*N + kr)*3', "out = ((L[P0] + f_a*(L[P1] - L[P0])) + f_b'*(L[P2] - L[P1])) + f_c'*(L[P3] - L[P2])",
                    'lerp(p, q, f) = p + f*(q - p)', 'out = lerp(lerp(c00, c10, f_g), lerp(c01, c11, f_g), f_b)',
                    'rintf(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f)', 'ties go in the order r, g, b'):
        assert formula in text, formula
    assert (_native.TDK_LUT_TETRAHEDRAL, _native.TDK_LUT_TRILINEAR, _native.TDK_LUT_GLOBAL) == (TETRA, TRILINEAR, GLOBAL)
    assert (_native.TDK_LUT_MAX_SHAPER, _native.TDK_LUT_MAX_SIZE) == (1024, 65)
    assert _native.ABI_VERSIONS['tdk_lut_abi_version'] == (1, 'lut ABI')
    assert _native.HEADERS[-1][0] == 'tdk_hip_lut.h'


def test_color_lut_invalid_arguments_fail_on_the_host(td):
    from torch_darktable._native import lib

    fake = 1 << 30   # never dereferenced: every check below happens before anything touches device memory or a device
    npix = 1000
    matrix = (ctypes.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    lo, scale = (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(16, 16, 16)
    shaper, lut = fake + (1 << 26), fake + (2 << 26)
    names = ['src', 'src_dtype', 'dst', 'dst_dtype', 'npix', 'matrix', 'shaper', 'shaper_size', 'shaper_tables', 'shaper_lo', 'shaper_scale', 'lut', 'lut_size',
             'lut_lo', 'lut_scale', 'interp', 'flags', 'stream']
    args = [fake, F32, fake + (1 << 24), F32, npix, matrix, shaper, 256, 3, 0.0, 255.0, lut, 17, lo, scale, TETRA, 0, None]

    def call(**change):
        a = list(args)
        for k, v in change.items():
            a[names.index(k)] = v
        return lib.tdk_color_lut(*a)

    def rejected(word, **change):
        return call(**change) == 1 and word in lib.tdk_last_error()

    for k in ('src', 'dst'):
        assert rejected(b'null pointer', **{k: None}), k
    for v in (-1, -(1 << 40)):
        assert rejected(b'npix', npix=v), v
    for k in ('src_dtype', 'dst_dtype'):
        for v in (3, -1, 7):
            assert rejected(b'dtype', **{k: v}), (k, v)
    for v in (0, 1, -4, 1025):
        assert rejected(b'shaper_size', shaper_size=v), v
    for v in (0, 2, 4, -1):
        assert rejected(b'shaper_tables', shaper_tables=v), v
    for v in (0, 1, -2, 66):
        assert rejected(b'lut_size', lut_size=v), v
    for bad in (float('nan'), float('inf'), -float('inf')):
        for k in range(9):
            m = (ctypes.c_float * 9)(*matrix)
            m[k] = bad
            assert rejected(b'matrix[%d]' % k, matrix=m), (k, bad)
        assert rejected(b'shaper_lo', shaper_lo=bad) and rejected(b'shaper_scale', shaper_scale=bad), bad
        for c in range(3):
            for name, good in (('lut_lo', lo), ('lut_scale', scale)):
                v = (ctypes.c_float * 3)(*good)
                v[c] = bad
                assert rejected(b'lut_lo[%d]' % c, **{name: v}), (name, c, bad)
    assert rejected(b'null pointer', lut_lo=None) and rejected(b'null pointer', lut_scale=None)
    for v in (2, -1, 5):
        assert rejected(b'interp', interp=v), v
    for v in (2, 3, -1, 4):
        assert rejected(b'flags', flags=v), v
    # overlap of dst with src, in bytes of each side's dtype: the same pointer (in place), dst inside src, src inside dst, the last byte
    nbytes = npix * 3 * 4
    for dst in (fake, fake + 64, fake - nbytes + 4, fake + nbytes - 4):
        assert rejected(b'src and dst overlap', dst=dst), dst
    assert rejected(b'src and dst overlap', dst=fake + npix * 3 - 1, src_dtype=U8, dst_dtype=F32)
    assert rejected(b'src and dst overlap', dst=fake - npix * 3 * 2 + 1, src_dtype=F32, dst_dtype=F16)
    # ... with the shaper (3 * 256 floats) and the LUT (17^3 * 3 floats)
    for dst in (shaper, shaper + 3 * 256 * 4 - 4, shaper - nbytes + 4):
        assert rejected(b'shaper and dst overlap', dst=dst), dst
    for dst in (lut, lut + 17 ** 3 * 12 - 4, lut - nbytes + 4):
        assert rejected(b'lut and dst overlap', dst=dst), dst
    # a stage that is left out is not checked: its other parameters are not read
    assert rejected(b'lut_size', shaper=None, shaper_size=-7, shaper_tables=9, shaper_lo=float('nan'), lut_size=1)
    assert rejected(b'shaper_size', lut=None, lut_size=900, lut_lo=None, lut_scale=None, shaper_size=1)
    assert rejected(b'flags', matrix=None, shaper=None, lut=None, flags=8)
    # npix == 0 is not an error and launches nothing (no device here: a launch would fail); the other checks still run
    assert call(npix=0) == 0
    assert call(npix=0, matrix=None, shaper=None, lut=None, dst=fake) == 0     # no bytes: nothing overlaps
    assert rejected(b'interp', npix=0, interp=9)


def test_lds_query_gives_the_staged_tables(td):
    from torch_darktable._native import lib

    q = lib.tdk_lut_lds_bytes
    for bad in ((1, 1, 0, 0), (1025, 1, 0, 0), (-3, 1, 17, 0), (16, 2, 0, 0), (16, 0, 0, 0), (0, 2, 17, 0), (0, 1, 1, 0), (0, 1, 66, 0), (0, 1, -5, 0),
                (0, 1, 17, 2), (0, 1, 17, -1), (16, 3, 17, 3)):
        assert q(*bad) == 0, bad
    assert q(0, 1, 0, 0) == 0 and q(0, 3, 0, GLOBAL) == 0                    # no table at all
    assert q(0, 1, 17, 0) == 12 * 17 ** 3 == 58956                           # the staged nodes, 12 bytes each
    assert q(0, 1, 17, GLOBAL) == 0 and q(0, 1, 33, 0) == 0 and q(0, 1, 65, 0) == 0 and q(0, 1, 19, 0) == 0   # the global path
    assert q(1024, 3, 0, 0) == 12288 and q(2, 1, 0, 0) == 8 and q(5, 3, 0, GLOBAL) == 60
    assert q(1024, 3, 17, 0) == 58956 + 12288 and q(1024, 3, 17, GLOBAL) == 12288 and q(1024, 3, 33, 0) == 12288
    assert q(0, 1, 18, 0) == 12 * 18 ** 3 == 69984                           # N = 18 fits the budget alone ...
    assert q(1024, 3, 18, 0) == 12288 and q(1024, 1, 18, 0) == 69984 + 4096  # ... not beside the largest shaper: then its nodes stay global
    worst = 0
    for n in [0] + list(range(2, 66)):
        for s, tables in ((0, 1), (2, 1), (2, 3), (1024, 1), (1024, 3), (333, 3)):
            for flags in (0, GLOBAL):
                b = q(s, tables, n, flags)
                staged = n and not flags and 12 * n ** 3 + 4 * s * tables <= BUDGET
                assert b == 4 * s * tables + (12 * n ** 3 if staged else 0), (s, tables, n, flags, b)
                assert b <= BUDGET
                worst = max(worst, b)
                assert not (n and n <= 17 and not flags) or staged                # N <= 17 is staged beside any shaper
    print(f'tdk_lut_lds_bytes: at most {worst} bytes')
    assert worst == 69984 + 4096                                                 # N = 18 beside one table of 1024
    assert 2 * worst <= 160 * 1024                                               # two workgroups share a CU


def test_package_exports_colorlut(td):
    import torch_darktable

    assert torch_darktable.ColorLUT is torch_darktable.colorlut.ColorLUT
    assert 'ColorLUT' in torch_darktable.__all__ and 'colorlut' in torch_darktable.__all__
    assert torch_darktable.colorlut.__all__ == ['ColorLUT']
    for name in ('process', 'from_cube', 'identity', 'from_matrix', 'lds_bytes'):
        assert callable(getattr(torch_darktable.ColorLUT, name)), name
    params = list(inspect.signature(torch_darktable.ColorLUT.__init__).parameters)
    assert params == ['self', 'device', 'matrix', 'shaper', 'shaper_domain', 'lut', 'lut_domain', 'interpolation']
    defaults = {k: p.default for k, p in inspect.signature(torch_darktable.ColorLUT.__init__).parameters.items()}
    assert (defaults['matrix'], defaults['shaper'], defaults['lut'], defaults['interpolation']) == (None, None, None, 'tetrahedral')
    assert defaults['shaper_domain'] == (0.0, 1.0) and defaults['lut_domain'] == ((0, 0, 0), (1, 1, 1))
    assert list(inspect.signature(torch_darktable.ColorLUT.process).parameters) == ['self', 'frame', 'out_dtype']
    from torch_darktable import torch_darktable_extension as ext   # its extra exports are a closed list: nothing of the colour transform
    assert not any('lut' in n.lower() for n in dir(ext))


def test_pipeline_takes_color_and_look_and_the_settings_stay_pinned(td):
    import torch
    from torch_darktable.pipeline import CameraSettings, ImageProcessingSettings, ImageProcessor

    params = list(inspect.signature(ImageProcessor.__init__).parameters)
    assert params[-3:] == ['sharpen', 'chroma_denoise', 'raw_correction']
    assert params[params.index('highlights') + 1:params.index('sharpen')] == ['color', 'look']
    for name in ('color', 'look'):
        assert inspect.signature(ImageProcessor.__init__).parameters[name].default is None
    dev = torch.device('cuda', 0)
    build = lambda **kw: ImageProcessor((64, 48), td.BayerPattern.RGGB, td.PackedFormat.Packed12, ImageProcessingSettings(), dev, None, **kw)
    for name in ('color', 'look'):
        for wrong in (object(), np.eye(3), 'film.cube', td.Sharpen(dev)):
            with pytest.raises(TypeError, match=f'{name} must be a ColorLUT'):
                build(**{name: wrong})
    from_settings = inspect.signature(ImageProcessor.from_camera_settings).parameters
    assert list(from_settings) == ['camera_settings', 'device', 'storage_dtype']
    for model in (ImageProcessingSettings, CameraSettings):
        assert not {'color', 'colour', 'look', 'lut', 'color_lut', 'colorlut', 'cube'} & set(model.model_fields), model
        assert not any('lut' in name or 'look' in name for name in model.model_fields), model


def test_python_front_end_validates_without_a_device(td):
    import torch

    cuda = torch.device('cuda', 0)   # a device object only: nothing below needs a GPU
    with pytest.raises(ValueError, match='CUDA'):
        td.ColorLUT(torch.device('cpu'))
    with pytest.raises(ValueError, match='CUDA'):
        td.ColorLUT.from_matrix(torch.device('cpu'), np.eye(3))
    with pytest.raises(ValueError, match='interpolation'):
        td.ColorLUT(cuda, interpolation='cubic')
    for m in (np.eye(4), np.ones(8), np.ones((9, 1)), np.ones((1, 3, 3))):
        with pytest.raises(ValueError, match='matrix must be 3x3'):
            td.ColorLUT(cuda, matrix=m)
    for bad in (float('nan'), float('inf')):
        m = np.eye(3)
        m[1, 2] = bad
        with pytest.raises(ValueError, match='matrix must be finite'):
            td.ColorLUT(cuda, matrix=m)
    for shaper in (np.zeros(1), np.zeros(1025), np.zeros((2, 16)), np.zeros((3, 1)), np.zeros((3, 4, 4)), np.zeros(())):
        with pytest.raises(ValueError, match='shaper must be'):
            td.ColorLUT(cuda, shaper=shaper)
    with pytest.raises(ValueError, match='shaper must be finite'):
        td.ColorLUT(cuda, shaper=[0.0, float('nan'), 1.0])
    for domain in ((0.0, 0.0), (0.0, float('inf')), (float('nan'), 1.0), (1.0, 1.0 + 1e-12)):
        with pytest.raises(ValueError, match='shaper_domain'):
            td.ColorLUT(cuda, shaper=[0.0, 1.0], shaper_domain=domain)
    for lut in (np.zeros((1, 1, 1, 3)), np.zeros((66, 66, 66, 3), np.float32), np.zeros((4, 4, 4)), np.zeros((4, 4, 5, 3)), np.zeros((4, 4, 4, 4)), np.zeros(12)):
        with pytest.raises(ValueError, match='lut must be'):
            td.ColorLUT(cuda, lut=lut)
    bad = np.zeros((2, 2, 2, 3))
    bad[1, 0, 1, 2] = float('inf')
    with pytest.raises(ValueError, match='lut must be finite'):
        td.ColorLUT(cuda, lut=bad)
    for domain in (((0, 0, 0), (1, 0, 1)), ((0, 0), (1, 1)), ((0, 0, 0),), ((0, 0, 0), (1, float('nan'), 1))):
        with pytest.raises(ValueError, match='lut_domain'):
            td.ColorLUT(cuda, lut=np.zeros((2, 2, 2, 3)), lut_domain=domain)
    for size in (1, 66, 2.5, 0):
        with pytest.raises(ValueError, match='size'):
            td.ColorLUT.identity(cuda, size)

    # what the object tells: the float32 numbers the kernel is given
    empty = td.ColorLUT(cuda)
    assert (empty.matrix, empty.shaper, empty.lut, empty.shaper_size, empty.lut_size, empty.lds_bytes()) == (None, None, None, 0, 0, 0)
    assert repr(empty) == 'ColorLUT(no stage, lds=0)'
    c = td.ColorLUT(cuda, matrix=np.arange(9) / 10, shaper=np.linspace(0, 1, 5) ** 2, shaper_domain=(-0.5, 1.5), lut=np.zeros((17, 17, 17, 3)),
                    lut_domain=((0, 0.1, -1), (1, 0.9, 3)), interpolation='trilinear')
    f = np.float32
    assert c.matrix == tuple(float(f(v / 10)) for v in range(9)) and c.interpolation == 'trilinear'
    assert (c.shaper_size, c.shaper_tables, c.lut_size) == (5, 1, 17)
    assert c.shaper_lo == -0.5 and c.shaper_scale == float(f(4) / (f(1.5) - f(-0.5))) == 2.0
    assert c.lut_lo == (0.0, float(f(0.1)), -1.0)
    assert c.lut_scale == (16.0, float(f(16) / (f(0.9) - f(0.1))), 4.0)
    assert c.shaper.dtype == torch.float32 and c.lut.dtype == torch.float32 and not c.lut.is_cuda
    assert c.lds_bytes() == 58956 + 20 and repr(c) == 'ColorLUT(matrix, shaper=1x5, lut=17^3 trilinear, lds=58976)'
    c.global_nodes = True
    assert c.lds_bytes() == 20
    three = td.ColorLUT(cuda, shaper=np.zeros((3, 1024)), lut=np.zeros((33, 33, 33, 3)))
    assert (three.shaper_tables, three.shaper_size, three.lds_bytes()) == (3, 1024, 12288)
    ident = td.ColorLUT.identity(cuda, 3)
    assert ident.lut[2, 1, 0].tolist() == [0.0, 0.5, 1.0] and ident.lut_scale == (2.0, 2.0, 2.0) and ident.matrix is None and ident.shaper is None
    assert td.ColorLUT.from_matrix(cuda, [[2, 0, 0], [0, 1, 0], [0, 0, 0.5]]).matrix == (2.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.5)

    with pytest.raises(ValueError, match='three channels'):
        empty.process(torch.zeros(48, 64))
    with pytest.raises(ValueError, match='three channels'):
        empty.process(torch.zeros(48, 64, 4))
    with pytest.raises(ValueError, match='out_dtype'):
        empty.process(torch.zeros(48, 64, 3), out_dtype=torch.int32)
    with pytest.raises(RuntimeError, match='CUDA'):
        empty.process(torch.zeros(48, 64, 3))   # no CPU fallback
    with pytest.raises(RuntimeError, match='CUDA'):
        empty.process(torch.zeros(7, 3, dtype=torch.uint8), out_dtype=torch.float16)
