"""CPU-only (hipcc cross-compiles): the resource contract of the capture sharpening's kernel (csrc/deconv.hip), read from the gfx950
code-object metadata alone.

  * every instantiation -- storage type x channels x fused iterations F in {1, 2, 4} -- keeps its state in registers and LDS: no
    private segment, no SGPR or VGPR spills;
  * the LDS is static and at most 64 KB (two workgroups per CU), and tdk_deconv_lds_bytes answers the metadata;
  * they are wave64 kernels of 256 threads;
  * the final product is not folded into its binary16 rounding (v_fma_mixlo_f16 and its kin): the specification rounds the float32
    product first;
  * no atomics of any kind;
  * the source launches through one TDK_LAUNCH under the names tdk_deconv(...) and holds no allocation, copy, memset or
    synchronisation."""
import re
from pathlib import Path

import pytest

import kernel_isa

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'torch-darktable_amd' / 'csrc' / 'deconv.hip'
TYPES = {'f': 0, '6__half': 1}   # mangled storage type -> dtype tag
FUSED = (1, 2, 4)


@pytest.fixture(scope='module')
def metadata():
    return kernel_isa.metadata(kernel_isa.device_asm('deconv'))


def kernels(metadata):
    """{(dtype tag, channels, F): metadata}"""
    out = {}
    for name, m in metadata.items():
        found = re.search(r'\d+deconv_kernelI(f|6__half)Li(\d+)ELi(\d+)EE', name)
        if found:
            out[(TYPES[found.group(1)], int(found.group(2)), int(found.group(3)))] = m
    return out


def test_every_instantiation_lives_in_registers_and_lds(metadata):
    group = kernels(metadata)
    assert set(group) == {(t, c, f) for t in TYPES.values() for c in (1, 3) for f in FUSED} and len(metadata) == 12
    for key, m in group.items():
        print(key, {k: m[k] for k in ('vgpr_count', 'sgpr_count', 'private_segment_fixed_size', 'group_segment_fixed_size', 'wavefront_size')})
        assert m['private_segment_fixed_size'] == 0, (key, m)
        assert m['sgpr_spill_count'] == 0 and m['vgpr_spill_count'] == 0, (key, m)
        assert 0 < m['group_segment_fixed_size'] <= 64 * 1024, (key, m)
        assert m['wavefront_size'] == 64 and m['max_flat_workgroup_size'] == 256, (key, m)
        assert m['vgpr_count'] <= 128, (key, m)   # two workgroups of four waves per CU need no more than 256; 128 leaves room for four
    for (t, c, f), m in group.items():   # four planes of the tile with the largest apron 2 * RMAX * F
        assert m['group_segment_fixed_size'] == 4 * 4 * (32 + 2 * 2 * {1: 6, 2: 4, 4: 2}[f] * f) ** 2, (t, c, f)


def test_lds_query_answers_the_static_size(td, metadata):
    from torch_darktable._native import lib

    for (tag, channels, fused), m in kernels(metadata).items():
        for radius in range(1, {1: 6, 2: 4, 4: 2}[fused] + 1):
            for mask in (0, 1):
                assert lib.tdk_deconv_lds_bytes(channels, tag, radius, mask | (fused << 8)) == m['group_segment_fixed_size'], (tag, channels, fused, radius)
            if lib.tdk_deconv_fused_iterations(radius) == fused:
                assert lib.tdk_deconv_lds_bytes(channels, tag, radius, 1) == m['group_segment_fixed_size']


def test_no_product_is_fused_with_its_binary16_rounding():
    """out = x * g is a float32 value, rounded once more at a binary16 store; a mixed-precision multiply-add would round the exact product once."""
    asm = kernel_isa.device_asm('deconv')
    assert 'v_cvt_f16_f32' in asm or 'v_cvt_pk' in asm
    for fused in ('v_fma_mixlo_f16', 'v_fma_mixhi_f16', 'v_mad_mixlo_f16', 'v_mad_mixhi_f16'):
        assert fused not in asm, fused
    assert len(kernel_isa.kernel_bodies(asm, 'deconv_kernel')) == 12


def test_no_atomics():
    asm = kernel_isa.device_asm('deconv')
    for word in ('global_atomic', 'flat_atomic', 'buffer_atomic', 'ds_add', 'ds_cmpst', 'ds_max', 'ds_min', '_atomic'):
        assert word not in asm, word
    text = SOURCE.read_text()
    assert 'atomic' not in text.replace('no atomics', '')


def test_launches_and_nothing_else():
    text = SOURCE.read_text()
    assert text.count('TDK_LAUNCH(') == 1   # one kernel, launched ceil(N / F) times from one loop
    for name in ('tdk_deconv(only)', 'tdk_deconv(first)', 'tdk_deconv(iterate)', 'tdk_deconv(last)'):
        assert f'"{name}"' in text, name
    assert 'TDK_LAUNCH(name, (deconv_kernel<T, C, F>)' in text
    assert 'hipLaunchKernelGGL' not in text and '<<<' not in text
    for call in ('hipMalloc', 'hipMemcpy', 'hipMemset', 'Synchronize', 'hipFree', 'hipHostMalloc'):
        assert call not in text, call
    assert '__shared__ DcLds<F> lds;' in text and 'extern __shared__' not in text   # static LDS
    assert 'sharpen.hip' not in text   # the blur is restated, not included
