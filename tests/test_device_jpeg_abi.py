"""CPU-only: the companion header include/tdk_hip_ext.h (entry points beyond the reference's surface) -- the library exports every
declaration, the ctypes table _native.EXT_SIGNATURES mirrors it parameter for parameter, the size queries and the argument checks of
the device-resident JPEG encode answer on the host, and the new kernels of that path keep everything in registers and LDS."""

import ctypes
import re
import subprocess
from pathlib import Path

import pytest

from abi_header import ctype_of, declarations, signature_tables_except

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / 'include' / 'tdk_hip_ext.h'
EXPECTED = ['tdk_ext_abi_version', 'tdk_jpeg_device_max_stream_bytes', 'tdk_jpeg_device_workspace_bytes', 'tdk_jpeg_encode_device',
            'tdk_jpeg_huffman_tables']


def test_header_declares_the_device_jpeg_surface():
    assert sorted(declarations(HEADER)) == EXPECTED
    assert re.search(r'#define TDK_EXT_ABI_VERSION 1\b', HEADER.read_text())


def test_library_exports_every_ext_symbol(td):
    lib = ctypes.CDLL(str(ROOT / 'torch-darktable_amd' / 'torch_darktable' / 'libtdk_hip.so'))
    for name in EXPECTED:
        assert hasattr(lib, name), f'{name} declared in tdk_hip_ext.h but not exported'
    lib.tdk_ext_abi_version.restype = ctypes.c_int
    assert lib.tdk_ext_abi_version() == 1


def test_ext_ctypes_table_matches_header(td):
    from torch_darktable import _native

    decls = declarations(HEADER)
    assert sorted(_native.EXT_SIGNATURES) == sorted(decls)
    assert not set(_native.EXT_SIGNATURES) & signature_tables_except('EXT_SIGNATURES')
    for name, (restype, argtypes) in _native.EXT_SIGNATURES.items():
        ret, params = decls[name]
        assert restype is (ctypes.c_int if ret == 'int' else ctypes.c_size_t), name
        assert [ctype_of(p) for p in params] == list(argtypes), f'{name}: header {params}, ctypes {argtypes}'


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
    flags = ['-O3', '-std=c++17', '--offload-arch=gfx950', '-ffp-contract=off', '-fno-slp-vectorize', '--cuda-device-only', '-S', '-o', '-']
    r = subprocess.run(['/opt/rocm/bin/hipcc', *flags, str(ROOT / 'torch-darktable_amd' / 'csrc' / 'jpeg.hip')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    private, name = {}, None
    for line in r.stdout.split('\n'):   # the code-object metadata: .name precedes .private_segment_fixed_size in every kernel's map
        m = re.match(r'\s+\.name:\s+(\S+)', line)
        if m:
            name = m.group(1)
        m = re.match(r'\s+\.private_segment_fixed_size:\s+(\d+)', line)
        if m and name:
            private[name] = int(m.group(1))
    wanted = {n: v for n, v in private.items() if re.search(r'jpeg_tables_kernelILb[01]E|jpeg_stuff_kernelILb1ELb1E|jpeg_scan_kernelILb1E', n)}
    assert len(wanted) == 4, sorted(private)
    assert all(v == 0 for v in wanted.values()), wanted
