"""CPU-only: the sixth header include/tdk_hip_raw.h (sensor correction) -- it parses to exactly its three declarations
(exports and the ctypes table: tests/test_header_abi.py), every argument error of tdk_raw_prepare is
reported on the host before any HIP call and names its argument, the LDS query stays within 64 KB, and the Python front end
torch_darktable.RawPrepare forms black and scale as the header says and raises the error types of Warp and Resize."""

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from abi_header import declarations

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / 'include' / 'tdk_hip_raw.h'
EXPECTED = ['tdk_raw_abi_version', 'tdk_raw_prepare', 'tdk_raw_prepare_lds_bytes']
F32, F16 = 0, 1
PACKED12, PACKED12_IDS, U16, RAW_F32, RAW_F16 = range(5)
RGGB = 0x94949494


def test_header_declares_the_raw_surface(td):
    from torch_darktable import _native

    decls = declarations(HEADER)
    assert sorted(decls) == EXPECTED
    text = HEADER.read_text()
    assert re.search(r'#define TDK_RAW_ABI_VERSION 1\b', text)
    for name, value in (('PACKED12', 0), ('PACKED12_IDS', 1), ('U16', 2), ('F32', 3), ('F16', 4), ('HOT', 1), ('DEAD', 2)):
        assert re.search(rf'#define TDK_RAW_{name} {value}\b', text), name
    assert '#include "tdk_hip.h"' in text and 'extern "C"' in text
    assert decls['tdk_raw_prepare'] == ('int', ['const void* src', 'int src_format', 'void* dst', 'int dst_dtype', 'unsigned char* mask', 'int width',
                                                'int height', 'uint32_t pattern', 'const float* black', 'const float* scale', 'int defects',
                                                'float threshold', 'float ratio', 'int min_count', 'const float* shading', 'int grid_width',
                                                'int grid_height', 'const float* gains', 'int clip', 'tdk_stream_t stream'])
    assert decls['tdk_raw_prepare_lds_bytes'] == ('size_t', ['int defects', 'int shading'])
    for formula in ('p = 2*(i & 1) + (j & 1)', 'L = (raw - black[p]) * scale[p]', 'S = { n : n < L*ratio }', 'S = { n : n > threshold and L < n*ratio }',
                    '(i-2, j), (i+2, j), (i, j-2), (i, j+2)', 't = j*(gw - 1);  qx = t / (W - 1);  rx = t % (W - 1);  ax = (float)rx / (float)(W - 1)',
                    'qx1 = min(qx + 1, gw - 1)', 'g0 = G[qy][qx][p]*(1.0f - ax) + G[qy][qx1][p]*ax', 'g  = g0*(1.0f - ay) + g1*ay',
                    'v = min(max(v*gains[colour], 0.0f), 1.0f)', '4*(gw - 1) <= W - 1'):
        assert formula in text, formula
    assert (_native.TDK_RAW_PACKED12, _native.TDK_RAW_PACKED12_IDS, _native.TDK_RAW_U16, _native.TDK_RAW_F32, _native.TDK_RAW_F16) == (0, 1, 2, 3, 4)
    assert (_native.TDK_RAW_HOT, _native.TDK_RAW_DEAD) == (1, 2)
    assert _native.ABI_VERSIONS['tdk_raw_abi_version'] == (1, 'raw ABI')


def test_raw_prepare_invalid_arguments_fail_on_the_host(td):
    from torch_darktable._native import lib

    fake = 1 << 20   # never dereferenced: every check below happens before anything touches device memory or a device
    black, scale = (ctypes.c_float * 4)(0, 0, 0, 0), (ctypes.c_float * 4)(*([1 / 4095] * 4))
    names = ['src', 'fmt', 'dst', 'dtype', 'mask', 'w', 'h', 'pattern', 'black', 'scale', 'defects', 'threshold', 'ratio', 'min_count', 'shading', 'gw',
             'gh', 'gains', 'clip', 'stream']
    w, h = 64, 48
    args = [fake, PACKED12, fake + (1 << 24), F32, fake + (2 << 24), w, h, RGGB, ctypes.addressof(black), ctypes.addressof(scale), 3, 0.02, 0.5, 3,
            fake + (3 << 24), 9, 7, fake + (4 << 24), 1, None]

    def call(**change):
        a = list(args)
        for k, v in change.items():
            a[names.index(k)] = v
        return lib.tdk_raw_prepare(*a)

    def failed(word):
        return word in lib.tdk_last_error()

    for k in ('src', 'dst', 'black', 'scale'):
        assert call(**{k: None}) == 1 and failed(b'null pointer') and failed(k.encode()), k
    for k in ('w', 'h'):
        for v in (0, 1, -4, 65536, 65537):
            assert call(**{k: v}) == 1 and failed(b'frame size'), (k, v)
        for v in (3, 63, 65535):
            assert call(**{k: v}) == 1 and failed(b'even'), (k, v)
    for v in (-1, 5):
        assert call(fmt=v) == 1 and failed(b'src_format'), v
    for v in (2, -1):
        assert call(dtype=v) == 1 and failed(b'dtype'), v
    for v in (0, 1, 0x94949495):
        assert call(pattern=v) == 1 and failed(b'pattern'), v
    for which in ('black', 'scale'):
        for p in range(4):
            for bad in (float('nan'), float('inf'), -float('inf')):
                arr = (ctypes.c_float * 4)(*(black if which == 'black' else scale))
                arr[p] = bad
                assert call(**{which: ctypes.addressof(arr)}) == 1 and failed(f'{which}[{p}]'.encode()), (which, p, bad)
    for v in (-1, 4, 8):
        assert call(defects=v) == 1 and failed(b'defects'), v
    for v in (-0.001, float('nan'), float('inf')):
        assert call(threshold=v) == 1 and failed(b'threshold'), v
    for v in (0.0, -0.5, 1.0001, float('nan')):
        assert call(ratio=v) == 1 and failed(b'ratio'), v
    for v in (0, 5, -1):
        assert call(min_count=v) == 1 and failed(b'min_count'), v
    for v in (2, -1):
        assert call(clip=v) == 1 and failed(b'clip'), v
    # the grid: 2..257 nodes per axis, at least four pixels apart, and none without a pointer
    for k in ('gw', 'gh'):
        for v in (0, 1, 258):
            assert call(**{k: v}) == 1 and failed(b'shading grid'), (k, v)
    assert call(gw=17) == 1 and failed(b'too dense')          # 4 * 16 > 63
    assert call(gh=13) == 1 and failed(b'too dense')          # 4 * 12 > 47
    assert call(shading=None) == 1 and failed(b'without shading')
    # overlap, in bytes: dst against src, shading, gains and mask; mask against src, shading and gains
    src_bytes, dst_bytes, grid_bytes = w * h * 3 // 2, w * h * 4, 9 * 7 * 16
    for dst in (fake, fake + src_bytes - 1, fake - dst_bytes + 1):
        assert call(dst=dst) == 1 and failed(b'src and dst overlap'), dst
    assert call(dst=fake + (3 << 24) + grid_bytes - 4) == 1 and failed(b'shading and dst overlap')
    assert call(dst=fake + (4 << 24) + 8) == 1 and failed(b'gains and dst overlap')
    assert call(mask=fake + (1 << 24) + dst_bytes - 1) == 1 and failed(b'mask and dst overlap')
    assert call(mask=fake + 16) == 1 and failed(b'mask and src overlap')
    assert call(mask=fake + (3 << 24)) == 1 and failed(b'mask and shading overlap')
    assert call(mask=fake + (4 << 24) - w * h + 1) == 1 and failed(b'mask and gains overlap')
    # the sizes of the other forms: a uint16 frame is longer than a packed one
    assert call(fmt=U16, dst=fake + w * h * 2 - 2) == 1 and failed(b'src and dst overlap')
    assert call(fmt=RAW_F32, dst=fake + w * h * 4 - 4) == 1 and failed(b'src and dst overlap')
    assert call(fmt=RAW_F16, dtype=F16, dst=fake - w * h * 2 + 2) == 1 and failed(b'src and dst overlap')


def test_lds_query_stays_within_64_kb(td):
    from torch_darktable._native import lib

    q = lib.tdk_raw_prepare_lds_bytes
    assert q(0, 0) == 0                                    # the plain streaming form: no LDS, no barrier
    tile, shade = q(1, 0), q(0, 1)
    assert tile == (128 + 4) * (16 + 4) * 4                # the tile with its two-pixel apron as float32
    assert 0 < shade <= 8 * 1024                           # records and nodes: a few KB
    assert q(3, 1) == tile + shade <= 65536 and q(2, 5) == tile + shade
    assert tile % 16 == 0 and shade % 16 == 0              # every carve offset stays 16-byte aligned


def test_package_exports_raw_prepare(td):
    import torch_darktable

    assert torch_darktable.RawPrepare is torch_darktable.rawprepare.RawPrepare
    assert 'RawPrepare' in torch_darktable.__all__ and 'rawprepare' in torch_darktable.__all__
    assert torch_darktable.rawprepare.__all__ == ['RawPrepare']
    for name in ('process', 'process_packed', 'shading_from_rgb', 'lds_bytes'):
        assert callable(getattr(torch_darktable.RawPrepare, name)), name


def test_front_end_forms_black_and_scale_in_float64(td):
    import torch

    cuda = torch.device('cuda', 0)   # a device object only: nothing below reaches the GPU
    rp = td.RawPrepare(cuda, (4096, 3072), td.BayerPattern.GRBG, black=[240.0, 256.5, 250.0, 260.0], white=4000.0, hot=True, threshold=0.03)
    assert rp.black.dtype == np.float32 and np.array_equal(rp.black, np.array([240.0, 256.5, 250.0, 260.0], dtype=np.float32))
    assert np.array_equal(rp.scale, (1.0 / (4000.0 - np.array([240.0, 256.5, 250.0, 260.0]))).astype(np.float32))
    assert rp.image_size == (4096, 3072) and rp.lds_bytes() > 0
    assert repr(rp) == ('RawPrepare(4096x3072, GRBG, black=[240.0, 256.5, 250.0, 260.0], white=4000, defects=hot(threshold=0.03, ratio=0.5, min_count=3), '
                        'clip=True)')
    ident = td.RawPrepare(cuda, (64, 48), td.BayerPattern.RGGB)
    assert np.all(ident.black == 0) and np.all(ident.scale == np.float32(1.0) / np.float32(4095.0)) and ident.lds_bytes() == 0
    assert ident.lds_bytes(mask=True) > 0
    rp.black[0] = 5.0   # a copy: the object keeps its values
    assert rp.black[0] == 240.0
    g = td.RawPrepare.shading_from_rgb(torch.arange(24, dtype=torch.float32).view(2, 4, 3), td.BayerPattern.GRBG)
    assert tuple(g.shape) == (2, 4, 4) and torch.equal(g[0, 0], torch.tensor([1.0, 0.0, 2.0, 1.0]))   # G R / B G


def test_python_front_end_raises_the_error_types_of_warp(td):
    import torch

    cuda = torch.device('cuda', 0)
    P = td.BayerPattern.RGGB
    with pytest.raises(ValueError, match='CUDA'):
        td.RawPrepare(torch.device('cpu'), (64, 48), P)
    for size in ((0, 48), (64, -2), (65536, 48)):
        with pytest.raises(ValueError, match='dimensions'):
            td.RawPrepare(cuda, size, P)
    for size in ((63, 48), (64, 47)):
        with pytest.raises(ValueError, match='even'):
            td.RawPrepare(cuda, size, P)
    with pytest.raises(ValueError, match='bayer pattern'):
        td.RawPrepare(cuda, (64, 48), 'RGGB')
    with pytest.raises(ValueError, match='one level or four'):
        td.RawPrepare(cuda, (64, 48), P, black=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match='finite'):
        td.RawPrepare(cuda, (64, 48), P, black=float('nan'))
    with pytest.raises(ValueError, match='above every black'):
        td.RawPrepare(cuda, (64, 48), P, black=[0, 0, 4095, 0])
    with pytest.raises(ValueError, match='finite in float32'):
        td.RawPrepare(cuda, (64, 48), P, black=0.0, white=1e-60)   # 1 / white overflows float32
    with pytest.raises(ValueError, match='threshold'):
        td.RawPrepare(cuda, (64, 48), P, threshold=-1.0)
    for ratio in (0.0, 1.5, float('nan')):
        with pytest.raises(ValueError, match='ratio'):
            td.RawPrepare(cuda, (64, 48), P, ratio=ratio)
    for n in (0, 5, 2.5):
        with pytest.raises(ValueError, match='min_count'):
            td.RawPrepare(cuda, (64, 48), P, min_count=n)
    with pytest.raises(ValueError, match='grid_height, grid_width, 4'):
        td.RawPrepare(cuda, (64, 48), P, shading=torch.ones(7, 9, 3))
    with pytest.raises(ValueError, match='2..257'):
        td.RawPrepare(cuda, (64, 48), P, shading=torch.ones(1, 9, 4))
    with pytest.raises(ValueError, match='too dense'):
        td.RawPrepare(cuda, (64, 48), P, shading=torch.ones(7, 17, 4))
    with pytest.raises(ValueError, match='gains must be'):
        td.RawPrepare.shading_from_rgb(torch.ones(7, 9, 4), P)
    rp = td.RawPrepare(cuda, (64, 48), P)
    with pytest.raises(RuntimeError, match='shape'):
        rp.process(torch.zeros(48, 60))
    with pytest.raises(RuntimeError, match='shape'):
        rp.process(torch.zeros(64, 48))
    with pytest.raises(RuntimeError, match='CUDA'):
        rp.process(torch.zeros(48, 64))   # no CPU fallback
    with pytest.raises(RuntimeError, match='CUDA'):
        rp.process_packed(torch.zeros(64 * 48 * 3 // 2, dtype=torch.uint8))
    with pytest.raises(ValueError, match='packed format'):
        rp.process_packed(torch.zeros(64 * 48 * 3 // 2, dtype=torch.uint8), format_type=2)


def test_image_processor_takes_raw_correction_and_settings_are_unchanged(td):
    """The keyword exists, defaults to None, and the settings models gained no field (the reference's JSON keeps loading)."""
    import inspect

    from torch_darktable.pipeline.camera_settings import CameraSettings
    from torch_darktable.pipeline.config import ImageProcessingSettings
    from torch_darktable.pipeline.image_processor import ImageProcessor

    p = inspect.signature(ImageProcessor.__init__).parameters
    assert list(p)[-1] == 'raw_correction' and p['raw_correction'].default is None and p['storage_dtype'].default is not inspect.Parameter.empty
    for model in (CameraSettings, ImageProcessingSettings):
        assert not [f for f in model.model_fields if 'raw' in f or 'black' in f or 'shading' in f or 'defect' in f], model
