"""CPU-only: the header include/tdk_hip_wiener.h (the Wiener entry points with flags, the strip kernel's interior rule as host
queries) -- it parses to exactly its five declarations (exports and the ctypes table: tests/test_header_abi.py), its constants are
the package's, its row stands in the registry and the build list, unknown flags are refused on the host before any HIP call, and
verification_paths carries the switch."""

import inspect
import re
from pathlib import Path

from abi_header import declarations, load_build_module

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / 'include' / 'tdk_hip_wiener.h'
EXPECTED = ['tdk_wiener_abi_version', 'tdk_wiener_ex', 'tdk_wiener_log_luminance_lab_ex', 'tdk_wiener_strip_interior', 'tdk_wiener_strip_order']
F32 = 0


def test_header_declares_the_wiener_flags_surface(td):
    from torch_darktable import _native

    decls = declarations(HEADER)
    assert sorted(decls) == EXPECTED
    text = HEADER.read_text()
    assert re.search(r'#define TDK_WIENER_ABI_VERSION 1\b', text) and re.search(r'#define TDK_WIENER_GENERAL_BODY 1u\b', text)
    assert '#include "tdk_hip.h"' in text and 'extern "C"' in text
    base = declarations(ROOT / 'include' / 'tdk_hip.h')
    # the two entry points are their tdk_hip.h forms with `uint32_t flags` in front of the stream
    for name, plain in (('tdk_wiener_ex', 'tdk_wiener'), ('tdk_wiener_log_luminance_lab_ex', 'tdk_wiener_log_luminance_lab')):
        ret, params = decls[name]
        assert ret == 'int' and params[-2:] == ['uint32_t flags', 'tdk_stream_t stream']
        assert (ret, params[:-2] + params[-1:]) == base[plain], name
    assert decls['tdk_wiener_strip_interior'] == ('int', ['int width', 'int height', 'int segment_rows', 'int strip', 'int segment'])
    assert decls['tdk_wiener_strip_order'] == ('int', ['int width', 'int height', 'int segment_rows', 'int workgroup'])
    assert decls['tdk_wiener_abi_version'] == ('int', [])
    assert 'interior <=> 1 <= strip < width / 128  &&  1 <= segment < height / (8 segment_rows)  &&  width % 4 == 0' in text
    assert _native.TDK_WIENER_GENERAL_BODY == 1
    rows = [row for row in _native.HEADERS if row[0] == 'tdk_hip_wiener.h']
    assert rows == [('tdk_hip_wiener.h', _native.WIENER_SIGNATURES, 'tdk_wiener_abi_version', 1, 'wiener ABI')]
    assert _native.ABI_VERSIONS['tdk_wiener_abi_version'] == (1, 'wiener ABI')
    assert sorted(_native.WIENER_SIGNATURES) == EXPECTED and _native.lib.tdk_wiener_abi_version() == 1
    build = load_build_module()
    assert HEADER in build.HEADERS and (ROOT / 'torch-darktable_amd' / 'csrc' / 'tdk_wiener_ystream.h') in build._inputs()


def test_unknown_flags_fail_on_the_host(td):
    from torch_darktable._native import lib

    fake = 1 << 30   # never dereferenced: the flags are checked before anything touches device memory or a device
    for flags in (2, 4, 3, 0x80000000):
        assert lib.tdk_wiener_ex(fake, fake + (1 << 24), fake + (2 << 24), 256, 128, 1, 32, 4, fake + (3 << 24), F32, flags, None) == 1
        assert b'tdk_wiener: unknown flags' in lib.tdk_last_error()
        assert lib.tdk_wiener_log_luminance_lab_ex(fake, fake + (2 << 24), 256, 128, 32, 4, fake + (3 << 24), 1e-4, None, F32, fake + (4 << 24), fake + (5 << 24),
                                                   flags, None) == 1
        assert b'tdk_wiener_log_luminance_lab: unknown flags' in lib.tdk_last_error()
    # the other argument checks are those of the plain entry points, flag or not
    for flags in (0, 1):
        assert lib.tdk_wiener_ex(fake, fake, fake, 256, 128, 2, 32, 4, fake, F32, flags, None) == 1 and b'channels must be 1 or 3' in lib.tdk_last_error()
        assert lib.tdk_wiener_ex(None, fake, fake, 256, 128, 1, 32, 4, fake, F32, flags, None) == 1 and b'null pointer' in lib.tdk_last_error()
        assert lib.tdk_wiener_log_luminance_lab_ex(fake, fake, 256, 128, 32, 4, fake, 0.0, None, F32, fake, fake, flags, None) == 1
        assert b'Epsilon must be positive' in lib.tdk_last_error()


def test_verification_paths_carries_the_switch(td):
    from torch_darktable import torch_darktable_extension as ext

    params = inspect.signature(ext.verification_paths).parameters
    assert list(params)[-1] == 'wiener_general_body' and params['wiener_general_body'].default is False
    assert getattr(ext._verify, 'wiener', 0) == 0
    with ext.verification_paths(wiener_general_body=True):
        assert ext._verify.wiener == 1 and ext._verify.rcd == 0 and ext._verify.bil == 0 and ext._verify.bil_lab == 0
        with ext.verification_paths(rcd_tiles=True):
            assert ext._verify.wiener == 0
        assert ext._verify.wiener == 1
    assert ext._verify.wiener == 0
