"""CPU-only (hipcc cross-compiles): the resource contract of the two kernels of the purple-fringe removal (csrc/defringe.hip), read
from the gfx950 code-object metadata and the source alone.

  * every instantiation -- launch x storage type x domain -- keeps its state in registers and LDS: no private segment, no SGPR or
    VGPR spills;
  * the LDS is static, at most 40 KB in both launches (four workgroups per CU), the restatement's count of the planes, and
    tdk_defringe_lds_bytes answers the larger of the two;
  * they are wave64 kernels of 256 threads whose registers let four workgroups share a CU;
  * the source launches through two TDK_LAUNCH and holds no allocation, copy, memset or synchronisation."""
import re
from pathlib import Path

import pytest

import defringe_spec as spec
import kernel_isa

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'torch-darktable_amd' / 'csrc' / 'defringe.hip'
TYPES = {'f': 0, '6__half': 1}   # mangled storage type -> dtype tag


@pytest.fixture(scope='module')
def metadata():
    return kernel_isa.metadata(kernel_isa.device_asm('defringe'))


def kernels(metadata):
    """{(launch, dtype tag, square-root domain): metadata}"""
    out = {}
    for name, m in metadata.items():
        found = re.search(r'\d+defringe_(edge|correct)_kernelI(f|6__half)Lb([01])EE', name)
        if found:
            out[(found.group(1), TYPES[found.group(2)], int(found.group(3)))] = m
    return out


def test_every_instantiation_lives_in_registers_and_lds(metadata):
    group = kernels(metadata)
    assert set(group) == {(launch, t, q) for launch in ('edge', 'correct') for t in (0, 1) for q in (0, 1)} and len(metadata) == 8
    for key, m in group.items():
        print(key, {k: m[k] for k in ('vgpr_count', 'sgpr_count', 'private_segment_fixed_size', 'group_segment_fixed_size', 'wavefront_size')})
        assert m['private_segment_fixed_size'] == 0, (key, m)
        assert m['sgpr_spill_count'] == 0 and m['vgpr_spill_count'] == 0, (key, m)
        want = spec.lds_bytes() if key[0] == 'edge' else spec.lds_bytes_correct()
        assert m['group_segment_fixed_size'] == want <= 40 * 1024 < 64 * 1024, (key, m)   # four workgroups in the 160 KB of a CU
        assert m['wavefront_size'] == 64 and m['max_flat_workgroup_size'] == 256, (key, m)
        assert m['vgpr_count'] <= 128, (key, m)   # four workgroups of four waves per CU (the LDS's limit) need no more than 128


def test_lds_query_answers_the_larger_launch(td, metadata):
    from torch_darktable import _native
    from torch_darktable._native import lib

    assert (_native.TDK_DEFRINGE_TILE, _native.TDK_DEFRINGE_MAX_RADIUS, _native.TDK_DEFRINGE_MAX_SAMPLE_RADIUS) == (spec.TILE, spec.MAX_RADIUS, spec.MAX_SAMPLE_RADIUS)
    group = kernels(metadata)
    for tag in (0, 1):
        for sqrt in (0, 1):
            larger = max(group[('edge', tag, sqrt)]['group_segment_fixed_size'], group[('correct', tag, sqrt)]['group_segment_fixed_size'])
            for radius, sample_radius in ((1, 1), (6, 6), (12, 8)):
                for mode in (0, _native.TDK_DEFRINGE_STATIC):
                    flags = mode | (0 if sqrt else _native.TDK_DEFRINGE_LINEAR)
                    assert lib.tdk_defringe_lds_bytes(tag, radius, sample_radius, flags) == larger == spec.lds_bytes() <= 64 * 1024
    for bad in ((2, 6, 6, 0), (0, 13, 6, 0), (0, 6, 9, 0), (0, 6, 6, 4), (0, 6, 6, -1)):
        assert lib.tdk_defringe_lds_bytes(*bad) == 0, bad


def test_two_launches_and_nothing_else():
    text = SOURCE.read_text()
    assert text.count('TDK_LAUNCH(') == 2
    assert 'TDK_LAUNCH("tdk_defringe(edge)", (defringe_edge_kernel<T, SQRT>)' in text and 'TDK_LAUNCH("tdk_defringe(correct)", (defringe_correct_kernel<T, SQRT>)' in text
    assert text.index('TDK_LAUNCH("tdk_defringe(edge)"') < text.index('TDK_LAUNCH("tdk_defringe(correct)"')
    assert 'hipLaunchKernelGGL' not in text and '<<<' not in text
    for call in ('hipMalloc', 'hipMemcpy', 'hipMemset', 'Synchronize', 'hipFree', 'hipHostMalloc'):
        assert call not in text, call
    assert 'atomic' not in text.replace('there is no atomic', '')
    assert '__shared__ DfEdgeLds lds;' in text and '__shared__ DfCorrectLds lds;' in text and 'extern __shared__' not in text   # static LDS
