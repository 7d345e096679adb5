"""CPU-only (hipcc cross-compiles): the resource and instruction contract of the tone mapper's table form (csrc/tonemap.hip:
tonemap_table, tonemap_apply_table), read from the gfx950 assembly, and the header include/tdk_hip_tables.h.

  * both kernels keep their state in registers: no private segment, no SGPR or VGPR spills, no LDS (the table lives in global
    memory so that these kernels keep sharing a compute unit with the tile kernels of other frames);
  * the apply kernel holds no transcendental and no reciprocal -- the per-pixel arithmetic is gone, not moved;
  * its twelve samples per thread are twelve byte gathers, each a scalar base plus the lane's 32-bit offset, the loads and the store
    stay wide;
  * argument errors of tdk_tonemap_ex are reported on the host."""
import re
from pathlib import Path

import pytest

import kernel_isa
from abi_header import declarations

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / 'include' / 'tdk_hip_tables.h'


@pytest.fixture(scope='module')
def asm():
    return kernel_isa.device_asm('tonemap')


def only(found):
    assert len(found) == 1, sorted(found)
    return next(iter(found.values()))


def instructions(body):
    return [line.split()[0] for line in body if line and not line.startswith(('.', ';')) and not line.endswith(':')]


def test_both_kernels_live_in_registers(asm):
    meta = kernel_isa.metadata(asm)
    for kernel, vgprs in (('13tonemap_table', 32), ('19tonemap_apply_table', 32)):
        m = only({k: v for k, v in meta.items() if kernel in k})
        print(kernel, {k: m[k] for k in ('vgpr_count', 'sgpr_count', 'private_segment_fixed_size', 'group_segment_fixed_size')},
              len(instructions(only(kernel_isa.kernel_bodies(asm, kernel)))), 'instructions')
        assert m['private_segment_fixed_size'] == 0 and m['sgpr_spill_count'] == 0 and m['vgpr_spill_count'] == 0, (kernel, m)
        assert m['group_segment_fixed_size'] == 0, (kernel, m)
        assert m['vgpr_count'] <= vgprs and m['wavefront_size'] == 64, (kernel, m)


def test_the_apply_kernel_computes_nothing_per_pixel(asm):
    ops = instructions(only(kernel_isa.kernel_bodies(asm, '19tonemap_apply_table')))
    for word in ('v_exp', 'v_log', 'v_rcp', 'v_div', 'v_cvt_f32', 'v_sqrt', 'v_mul_f32', 'v_fma'):
        assert not [op for op in ops if op.startswith(word)], word
    valu = [op for op in ops if op.startswith('v_')]
    print(len(valu), 'VALU instructions in the kernel:', sorted(set(valu)))
    assert len(valu) <= 48   # twelve unpacks, nine packs and the loop's addresses: the per-pixel kernel has about 290 in its loop


def test_the_gathers_take_a_scalar_base_and_a_lane_offset(asm):
    body = only(kernel_isa.kernel_bodies(asm, '19tonemap_apply_table'))
    gathers = [line for line in body if line.startswith('global_load_ubyte')]
    assert len(gathers) == 12, gathers
    bases = set()
    for line in gathers:
        m = re.match(r'global_load_ubyte(?:_d16(?:_hi)?)? v\d+, v\d+, (s\[\d+:\d+\])(?: offset:\d+)?$', line)   # one 32-bit VGPR of offset
        assert m, line
        bases.add(m.group(1))
    assert len(bases) == 3, bases   # one base per channel
    loads = [line.split()[0] for line in body if line.startswith('global_load_dword')]
    stores = [line.split()[0] for line in body if line.startswith('global_store')]
    assert sorted(loads) in (['global_load_dwordx2'] * 3, ['global_load_dwordx2', 'global_load_dwordx4']), loads   # 24 bytes in
    assert stores == ['global_store_dwordx3'], stores                                                                # 12 bytes out


def test_header_and_argument_errors(td):
    from torch_darktable import _native
    from torch_darktable._native import lib

    decls = declarations(HEADER)
    assert sorted(decls) == ['tdk_tables_abi_version', 'tdk_tonemap_ex']
    assert decls['tdk_tonemap_ex'] == ('int', ['const void* rgb', 'uint8_t* out', 'int64_t npix', 'int mode', 'const float* metrics', 'float gamma', 'float intensity',
                                               'float light_adapt', 'float vibrance', 'int dtype', 'uint8_t* table', 'uint32_t flags', 'tdk_stream_t stream'])
    text = HEADER.read_text()
    for define in ('TDK_TABLES_ABI_VERSION 1', r'TDK_TONEMAP_TABLE_BYTES \(3 \* 65536\)', 'TDK_TONEMAP_DIRECT 1u'):
        assert re.search(rf'#define {define}', text), define
    assert (_native.TDK_TONEMAP_TABLE_BYTES, _native.TDK_TONEMAP_DIRECT) == (3 * 65536, 1)
    assert _native.ABI_VERSIONS['tdk_tables_abi_version'] == (1, 'tables ABI')
    fake = 1 << 30   # never dereferenced: every check below happens before a launch
    call = lambda **kw: lib.tdk_tonemap_ex(*[kw.get(k, v) for k, v in (('rgb', fake), ('out', fake + (1 << 28)), ('npix', 16), ('mode', 0), ('metrics', fake + (1 << 29)),  # noqa: E731
                                                                    ('gamma', 0.75), ('intensity', 2.0), ('light_adapt', 1.0), ('vibrance', 0.0), ('dtype', 1),
                                                                    ('table', fake + (1 << 27)), ('flags', 0), ('stream', None))])
    for flags in (2, 3, 0x80000000):
        assert call(flags=flags) == 1 and b'unknown flags' in lib.tdk_last_error(), flags
    assert call(npix=-1) == 1 and b'negative pixel count' in lib.tdk_last_error()
    assert call(npix=0) == 0 and call(npix=0, rgb=None, out=None, table=None) == 0   # nothing to do: no launch
    assert call(rgb=None) == 1 and b'null pointer' in lib.tdk_last_error()
    assert call(out=None) == 1 and b'null pointer' in lib.tdk_last_error()
    assert call(metrics=None) == 1 and b'metrics required' in lib.tdk_last_error()
    assert call(dtype=7) == 1 and b'unsupported dtype' in lib.tdk_last_error()
    assert call(mode=9) == 1 and b'unknown mode' in lib.tdk_last_error()


def test_verification_paths_carries_the_switch(td):
    from torch_darktable import torch_darktable_extension as ext

    assert getattr(ext._verify, 'tonemap', 0) == 0
    with ext.verification_paths(tonemap_direct=True):
        assert ext._verify.tonemap == 1 and ext._verify.wiener == 0
        with ext.verification_paths(wiener_general_body=True):
            assert ext._verify.tonemap == 0
        assert ext._verify.tonemap == 1
    assert ext._verify.tonemap == 0
