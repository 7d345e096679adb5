"""CPU-only (hipcc cross-compiles): the resource contract of the LMMSE demosaic's kernel (csrc/lmmse.hip), read from the gfx950
code-object metadata and the source alone.

  * every instantiation -- source type x destination type x domain -- keeps its state in registers and LDS: no private segment, no
    SGPR or VGPR spills;
  * the LDS is static, the six planes of the header's dependency chain in at most 40 KB (four workgroups per CU), and
    tdk_lmmse_lds_bytes answers the metadata;
  * they are wave64 kernels of 256 threads;
  * no atomics of any kind;
  * the source launches through one TDK_LAUNCH and holds no allocation, copy, memset or synchronisation."""
import re
from pathlib import Path

import pytest

import kernel_isa

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'torch-darktable_amd' / 'csrc' / 'lmmse.hip'
TYPES = {'f': 0, '6__half': 1}   # mangled storage type -> dtype tag
TILE_W, TILE_H = 32, 32


@pytest.fixture(scope='module')
def metadata():
    return kernel_isa.metadata(kernel_isa.device_asm('lmmse'))


def kernels(metadata):
    """{(source dtype tag, destination dtype tag, square-root domain): metadata}"""
    out = {}
    for name, m in metadata.items():
        found = re.search(r'\d+lmmse_kernelI(f|6__half)(f|6__half|S\d?_)Lb([01])EE', name)
        if found:
            dst = found.group(1) if found.group(2).startswith('S') else found.group(2)   # (a repeated type is mangled as a substitution)
            out[(TYPES[found.group(1)], TYPES[dst], int(found.group(3)))] = m
    return out


def planes_bytes():
    """t over the tile and its apron of 11, dh and dv (the tile +- 1 across, +- 9 along), ph and pv (+- 1, +- 5), D (+- 1, every other site)"""
    w, h = TILE_W, TILE_H
    return 4 * ((h + 22) * (w + 22) + (h + 2) * (w + 18) + (h + 18) * (w + 2) + (h + 2) * (w + 10) + (h + 10) * (w + 2) + (h + 2) * (w + 2) // 2)


def test_every_instantiation_lives_in_registers_and_lds(metadata):
    group = kernels(metadata)
    assert set(group) == {(s, d, q) for s in (0, 1) for d in (0, 1) for q in (0, 1)} and len(metadata) == 8
    for key, m in group.items():
        print(key, {k: m[k] for k in ('vgpr_count', 'sgpr_count', 'private_segment_fixed_size', 'group_segment_fixed_size', 'wavefront_size')})
        assert m['private_segment_fixed_size'] == 0, (key, m)
        assert m['sgpr_spill_count'] == 0 and m['vgpr_spill_count'] == 0, (key, m)
        assert m['group_segment_fixed_size'] == planes_bytes() <= 40 * 1024, (key, m)   # four workgroups in the 160 KB of a CU
        assert m['wavefront_size'] == 64 and m['max_flat_workgroup_size'] == 256, (key, m)
        assert m['vgpr_count'] <= 128, (key, m)   # four workgroups of four waves per CU (the LDS's limit) need no more than 128


def test_lds_query_answers_the_static_size(td, metadata):
    from torch_darktable import _native
    from torch_darktable._native import lib

    assert (_native.TDK_LMMSE_TILE_W, _native.TDK_LMMSE_TILE_H, _native.TDK_LMMSE_APRON) == (TILE_W, TILE_H, 11)
    for (src, dst, sqrt), m in kernels(metadata).items():
        assert lib.tdk_lmmse_lds_bytes(src, dst, 0 if sqrt else _native.TDK_LMMSE_LINEAR) == m['group_segment_fixed_size'] == planes_bytes()
    for bad in ((2, 0, 0), (0, -1, 0), (0, 0, 2), (0, 0, -1)):
        assert lib.tdk_lmmse_lds_bytes(*bad) == 0, bad


def test_no_atomics():
    asm = kernel_isa.device_asm('lmmse')
    for word in ('global_atomic', 'flat_atomic', 'buffer_atomic', 'ds_add', 'ds_cmpst', 'ds_max', 'ds_min', '_atomic'):
        assert word not in asm, word
    text = SOURCE.read_text()
    assert 'atomic' not in text.replace('no atomics', '')


def test_one_launch_and_nothing_else():
    text = SOURCE.read_text()
    assert text.count('TDK_LAUNCH(') == 1
    assert 'TDK_LAUNCH("tdk_lmmse", (lmmse_kernel<TI, TO, SQRT>)' in text
    assert 'hipLaunchKernelGGL' not in text and '<<<' not in text
    for call in ('hipMalloc', 'hipMemcpy', 'hipMemset', 'Synchronize', 'hipFree', 'hipHostMalloc'):
        assert call not in text, call
    assert '__shared__ LmLds lds;' in text and 'extern __shared__' not in text   # static LDS
