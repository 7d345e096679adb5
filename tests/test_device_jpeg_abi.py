"""CPU-only: the companion header include/tdk_hip_ext.h (entry points beyond the reference's surface) -- it parses to exactly its
five declarations (exports and the ctypes table: tests/test_header_abi.py), the size queries and the argument checks of
the device-resident JPEG encode answer on the host, and the new kernels of that path keep everything in registers and LDS."""

import re
from pathlib import Path

import pytest

from abi_header import declarations
from kernel_isa import device_asm, metadata

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / 'include' / 'tdk_hip_ext.h'
EXPECTED = ['tdk_ext_abi_version', 'tdk_jpeg_device_max_stream_bytes', 'tdk_jpeg_device_workspace_bytes', 'tdk_jpeg_encode_device',
            'tdk_jpeg_huffman_tables']


def test_header_declares_the_device_jpeg_surface(td):
    from torch_darktable import _native

    assert sorted(declarations(HEADER)) == EXPECTED
    assert re.search(r'#define TDK_EXT_ABI_VERSION 1\b', HEADER.read_text())
    assert _native.ABI_VERSIONS['tdk_ext_abi_version'] == (1, 'extension ABI')


def test_device_jpeg_size_queries_run_on_the_host(td):
    from torch_darktable._native import lib

    for bad in ((0, 8, 1), (8, 0, 1), (65536, 8, 1), (8, 65536, 1), (8, 8, 3), (8, 8, -1)):
        assert lib.tdk_jpeg_device_workspace_bytes(*bad) == 0, bad
        assert lib.tdk_jpeg_device_max_stream_bytes(*bad, 0) == 0, bad
    assert lib.tdk_jpeg_device_max_stream_bytes(64, 64, 1, 2) == 0
    for w, h, sub, blocks in ((4096, 3072, 1, 4096 // 16 * 3072 // 8 * 4), (4096, 3072, 0, 4096 // 8 * 3072 // 8 * 3),
                              (4096, 3072, 2, 4096 // 8 * 3072 // 8), (1, 1, 1, 4), (17, 9, 0, 3 * 3 * 2)):
        for progressive in (0, 1):
            cap = lib.tdk_jpeg_device_max_stream_bytes(w, h, sub, progressive)
            assert cap >= 1024 + 212 * blocks, (w, h, sub, cap)
        # the device path keeps no stream region of its own: the workspace of Jpeg.encode less at least that much
        ws = lib.tdk_jpeg_device_workspace_bytes(w, h, sub)
        assert 0 < ws and ws + cap <= lib.tdk_jpeg_workspace_bytes(w, h, sub), (w, h, sub)


def test_device_jpeg_invalid_arguments_fail_on_the_host(td):
    from torch_darktable._native import lib

    fake = 1 << 20   # never dereferenced: every check below happens before anything touches memory or a device
    args = [fake, 64, 48, 3, 90, 1, 0, fake, fake, 1 << 16, fake, None]

    def call(**change):
        a = list(args)
        for k, v in change.items():
            a[['image', 'w', 'h', 'fmt', 'quality', 'sub', 'prog', 'ws', 'out', 'cap', 'length', 'stream'].index(k)] = v
        return lib.tdk_jpeg_encode_device(*a)

    for k in ('image', 'ws', 'out', 'length'):
        assert call(**{k: None}) == 1 and b'null pointer' in lib.tdk_last_error(), k
    for q in (0, 101, -5):
        assert call(quality=q) == 1 and b'quality' in lib.tdk_last_error(), q
    assert call(w=0) == 1 and b'outside' in lib.tdk_last_error()
    assert call(fmt=4) == 1 and b'input format' in lib.tdk_last_error()
    assert call(sub=3) == 1 and b'subsampling' in lib.tdk_last_error()
    assert call(prog=2) == 1 and b'progressive' in lib.tdk_last_error()
    assert call(ws=fake + 16) == 1 and b'aligned' in lib.tdk_last_error()
    assert call(length=fake + 4) == 1 and b'aligned' in lib.tdk_last_error()
    assert lib.tdk_jpeg_huffman_tables(None, 4, fake, fake, None) == 1 and b'null pointer' in lib.tdk_last_error()
    assert lib.tdk_jpeg_huffman_tables(fake, 0, fake, fake, None) == 1 and b'ntables' in lib.tdk_last_error()


def test_device_path_kernels_use_no_scratch():
    """gfx950 ISA of csrc/jpeg.hip: the table / marker kernel (both forms) and the device-position stuffing kernel keep their state in
    registers and LDS (.private_segment_fixed_size: 0) -- the K.2 loop's per-lane arrays are indexed by unrolled constants only."""
    private = {name: m['private_segment_fixed_size'] for name, m in metadata(device_asm('jpeg')).items()}
    wanted = {n: v for n, v in private.items() if re.search(r'jpeg_tables_kernelILb[01]E|jpeg_stuff_kernelILb1ELb1E|jpeg_scan_kernelILb1E', n)}
    assert len(wanted) == 4, sorted(private)
    assert all(v == 0 for v in wanted.values()), wanted
