"""CPU-only: the fourth header include/tdk_hip_resample.h (antialiased scaling) -- it parses to exactly its three declarations
(exports and the ctypes table: tests/test_header_abi.py), every argument error of
tdk_resample is reported on the host before any HIP call, the LDS query stays within (0, 80 KB], and the Python front-end
torch_darktable.Resize and the pipeline entry points exist and raise the error types of NLMeans."""

import re
from pathlib import Path

import pytest

from abi_header import declarations

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / 'include' / 'tdk_hip_resample.h'
EXPECTED = ['tdk_resample', 'tdk_resample_abi_version', 'tdk_resample_lds_bytes']
F32, F16, U8 = 0, 1, 2


def test_header_declares_the_resample_surface(td):
    from torch_darktable import _native

    decls = declarations(HEADER)
    assert sorted(decls) == EXPECTED
    text = HEADER.read_text()
    assert re.search(r'#define TDK_RESAMPLE_ABI_VERSION 1\b', text)
    assert re.search(r'#define TDK_U8 2\b', text)   # beside TDK_F32 = 0 and TDK_F16 = 1 of tdk_hip.h
    assert '#include "tdk_hip.h"' in text and 'extern "C"' in text
    assert decls['tdk_resample'] == ('int', ['const void* src', 'void* dst', 'int src_width', 'int src_height', 'int dst_width', 'int dst_height',
                                             'int channels', 'int dtype', 'tdk_stream_t stream'])
    assert decls['tdk_resample_lds_bytes'] == ('size_t', ['int src_width', 'int src_height', 'int dst_width', 'int dst_height', 'int channels', 'int dtype'])
    for formula in ('s = n_in / n_out', 'r = max(s, 1)', 'c = s (i + 1/2)', 'w_j = max(0, 1 - |j + 1/2 - c| / r)', 'y_i = sum_j w_j x_j / sum_j w_j'):
        assert formula in text, formula
    assert (_native.TDK_F32, _native.TDK_F16, _native.TDK_U8) == (F32, F16, U8)
    assert _native.ABI_VERSIONS['tdk_resample_abi_version'] == (1, 'resample ABI')


def test_resample_invalid_arguments_fail_on_the_host(td):
    from torch_darktable._native import lib

    fake = 1 << 20   # never dereferenced: every check below happens before anything touches memory or a device
    names = ['src', 'dst', 'sw', 'sh', 'dw', 'dh', 'c', 'dtype', 'stream']
    args = [fake, fake + (1 << 24), 64, 48, 16, 12, 3, F32, None]

    def call(**change):
        a = list(args)
        for k, v in change.items():
            a[names.index(k)] = v
        return lib.tdk_resample(*a)

    for k in ('src', 'dst'):
        assert call(**{k: None}) == 1 and b'null pointer' in lib.tdk_last_error(), k
    for k in ('sw', 'sh'):
        for v in (0, -3, 65536):
            assert call(**{k: v}) == 1 and b'source size' in lib.tdk_last_error(), (k, v)
    for k in ('dw', 'dh'):
        for v in (0, -3, 65536):
            assert call(**{k: v}) == 1 and b'destination size' in lib.tdk_last_error(), (k, v)
    for c in (0, 2, 4):
        assert call(c=c) == 1 and b'channels' in lib.tdk_last_error(), c
    for d in (3, -1):
        assert call(dtype=d) == 1 and b'dtype' in lib.tdk_last_error(), d
    # the ratio: 16 is the last legal one on either axis
    assert call(sw=257, dw=16) == 1 and b'ratio' in lib.tdk_last_error()
    assert call(sh=193, dh=12) == 1 and b'ratio' in lib.tdk_last_error()
    assert call(sw=65535, dw=4095) == 1 and b'ratio' in lib.tdk_last_error()
    assert call(sw=17, sh=1, dw=1, dh=1) == 1 and b'ratio' in lib.tdk_last_error()
    # overlap, in bytes of the dtype: the same pointer, dst inside src, src inside dst, and the last byte
    src_bytes = 64 * 48 * 3 * 4
    for dst in (fake, fake + 64, fake - 16 * 12 * 3 * 4 + 4, fake + src_bytes - 4):
        assert call(dst=dst) == 1 and b'overlap' in lib.tdk_last_error(), dst
    assert call(dst=fake + src_bytes // 4, dtype=F32) == 1 and b'overlap' in lib.tdk_last_error()


def test_ratio_16_and_touching_buffers_pass_the_host_checks(td):
    """What the checks must let through is told apart from what they refuse by the LDS query, which applies the same size, ratio,
    channel and dtype checks and runs on the host (a launch needs a device)."""
    from torch_darktable._native import lib

    assert lib.tdk_resample_lds_bytes(256, 192, 16, 12, 3, F32) > 0          # exactly 16 on both axes
    assert lib.tdk_resample_lds_bytes(257, 192, 16, 12, 3, F32) == 0
    assert lib.tdk_resample_lds_bytes(256, 193, 16, 12, 3, F32) == 0
    assert lib.tdk_resample_lds_bytes(65520, 16, 4095, 1, 1, U8) > 0
    assert lib.tdk_resample_lds_bytes(65521, 16, 4095, 1, 1, U8) == 0
    assert lib.tdk_resample_lds_bytes(1, 1, 65535, 65535, 3, F16) > 0         # up-scaling is not limited by a ratio


def test_lds_query_stays_within_80_kb(td):
    from torch_darktable._native import lib

    q = lib.tdk_resample_lds_bytes
    for bad in ((0, 48, 16, 12, 3, F32), (64, 0, 16, 12, 3, F32), (64, 48, 0, 12, 3, F32), (64, 48, 16, 0, 3, F32), (65536, 48, 16384, 12, 3, F32),
                (64, 65536, 16, 16384, 3, F32), (64, 48, 65536, 12, 3, F32), (64, 48, 16, 65536, 3, F32), (64, 48, 16, 12, 2, F32),
                (64, 48, 16, 12, 4, F32), (64, 48, 16, 12, 0, F32), (64, 48, 16, 12, 3, 3), (64, 48, 16, 12, 3, -1), (64, 48, 3, 12, 3, F32),
                (64, 48, 16, 2, 3, F32)):
        assert q(*bad) == 0, bad
    sizes = [1, 2, 3, 17, 64, 100, 255, 256, 1000, 1024, 3072, 4096, 40000, 65535]
    worst, n = 0, 0
    for sw in sizes:
        for dw in sizes:
            if sw > 16 * dw:
                continue
            for sh, dh in ((sw, dw), (dw, sw), (3072, 192), (3072, 768), (1, 1), (65535, 4096), (7, 65535)):
                if sh > 16 * dh:
                    continue
                for c in (1, 3):
                    for dtype in (F32, F16, U8):
                        b = q(sw, sh, dw, dh, c, dtype)
                        assert 0 < b <= 80 * 1024, (sw, sh, dw, dh, c, dtype, b)
                        worst, n = max(worst, b), n + 1
    print(f'tdk_resample_lds_bytes over {n} legal geometries: at most {worst} bytes')
    # the benchmarked shapes leave room for at least four workgroups per CU
    for dst in ((1024, 768), (256, 192)):
        for dtype in (F32, F16, U8):
            assert 4 * q(4096, 3072, *dst, 3, dtype) <= 160 * 1024, (dst, dtype)


def test_package_exports_resize(td):
    import torch_darktable

    assert torch_darktable.Resize is torch_darktable.resample.Resize
    assert 'Resize' in torch_darktable.__all__ and 'resample' in torch_darktable.__all__
    assert torch_darktable.resample.__all__ == ['Resize']
    assert callable(torch_darktable.Resize.process) and callable(torch_darktable.Resize.longest_edge)
    from torch_darktable import torch_darktable_extension as ext   # its extra exports are a closed list: nothing of the scaler
    assert not any('resample' in n.lower() or 'resize' in n.lower() for n in dir(ext))


def test_pipeline_has_the_resized_entry_points(td):
    from torch_darktable.pipeline import ImageProcessor
    from torch_darktable.pipeline import util

    for name in ('process_resized', 'process_image_set_resized', 'process', 'process_image_set'):
        assert callable(getattr(ImageProcessor, name)), name
    # the reference's helper stays plain bilinear
    import inspect
    assert "mode='bilinear', align_corners=False" in inspect.getsource(util.resize) and 'antialias' not in inspect.getsource(util.resize)


def test_python_front_end_raises_the_error_types_of_nlmeans(td):
    import torch

    cuda = torch.device('cuda', 0)   # a device object only: nothing below reaches the GPU
    with pytest.raises(ValueError, match='CUDA'):
        td.Resize(torch.device('cpu'), (64, 48), (16, 12))
    for size in ((0, 48), (64, -1), (65536, 48)):
        with pytest.raises(ValueError, match='Input dimensions'):
            td.Resize(cuda, size, (16, 12))
        with pytest.raises(ValueError, match='Output dimensions'):
            td.Resize(cuda, (64, 48), size)
    for src, dst in (((257, 48), (16, 12)), ((64, 193), (16, 12)), ((17, 1), (1, 1))):
        with pytest.raises(ValueError, match='ratio'):
            td.Resize(cuda, src, dst)
    rs = td.Resize(cuda, (64, 48), (16, 12))
    assert (rs.input_size, rs.output_size) == ((64, 48), (16, 12)) and repr(rs) == 'Resize(64x48 -> 16x12)'
    assert td.Resize(cuda, (256, 192), (16, 12)).output_size == (16, 12)   # exactly 16:1
    assert 0 < rs.lds_bytes(3, torch.uint8) <= 80 * 1024 and rs.lds_bytes(2, torch.uint8) == 0 and rs.lds_bytes(3, torch.int32) == 0
    # longest_edge goes through pipeline.util.resize_longest_edge
    from torch_darktable.pipeline.util import resize_longest_edge
    for size, longest in (((4096, 3072), 1024), ((3072, 4096), 256), ((4112, 3008), 1000), ((64, 48), 0)):
        assert td.Resize.longest_edge(cuda, size, longest).output_size == resize_longest_edge(size, longest)
    with pytest.raises(RuntimeError, match='shape'):
        rs.process(torch.zeros(48, 60, 3))
    with pytest.raises(RuntimeError, match='shape'):
        rs.process(torch.zeros(64, 48, 3))
    with pytest.raises(ValueError, match='channels'):
        rs.process(torch.zeros(48, 64, 2))
    with pytest.raises(ValueError, match='channels'):
        rs.process(torch.zeros(48, 64, 4))
    with pytest.raises(RuntimeError, match='CUDA'):
        rs.process(torch.zeros(48, 64, 3))   # no CPU fallback
    with pytest.raises(RuntimeError, match='CUDA'):
        rs.process(torch.zeros(48, 64, 3, dtype=torch.uint8))
