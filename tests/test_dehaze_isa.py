"""CPU-only (hipcc cross-compiles): the resource contract of the haze removal's kernels (csrc/dehaze.hip), read from the gfx950
code-object metadata alone.

  * every instantiation -- dh_cells and dh_apply per storage type and cell size, dh_dark, dh_select, dh_coeff -- keeps its state in
    registers and LDS: no private segment, no SGPR or VGPR spills;
  * the LDS is static and at most 64 KB: none for dh_cells, the staged tiles and the histogram for the others, and what
    tdk_dehaze_lds_bytes answers is the largest of a call;
  * they are wave64 kernels, of 256 threads but for the one workgroup of dh_select, which has 1024;
  * the final add is not folded into its binary16 rounding (v_fma_mixlo_f16 and its kin): the specification rounds the float32 sum first;
  * the atomics are integer adds on LDS, none on memory;
  * the source launches five times through TDK_LAUNCH and holds no allocation, copy, memset or synchronisation."""
import re
from pathlib import Path

import pytest

import kernel_isa

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'torch-darktable_amd' / 'csrc' / 'dehaze.hip'
TYPES = {'f': 0, '6__half': 1}   # mangled storage type -> dtype tag
CELLS = (2, 4, 8, 16)
PLAIN = ('dark', 'select', 'coeff')


@pytest.fixture(scope='module')
def metadata():
    return kernel_isa.metadata(kernel_isa.device_asm('dehaze'))


def kernels(metadata, stem):
    """{(dtype tag, cell) or None for a kernel that is no template: metadata} of the kernels called dh_<stem>."""
    out = {}
    for name, m in metadata.items():
        found = re.search(rf'\d+dh_{stem}(?:I(f|6__half)Li(\d+)EE)?E', name)
        if found:
            out[None if found.group(1) is None else (TYPES[found.group(1)], int(found.group(2)))] = m
    return out


def test_every_kernel_lives_in_registers_and_lds(metadata):
    groups = {stem: kernels(metadata, stem) for stem in ('cells', 'apply', *PLAIN)}
    every = {(t, s) for t in TYPES.values() for s in CELLS}
    assert set(groups['cells']) == set(groups['apply']) == every and all(set(groups[stem]) == {None} for stem in PLAIN)
    assert len(metadata) == 8 + 3 + 8
    for stem, group in groups.items():
        for key, m in group.items():
            print(stem, key, {k: m[k] for k in ('vgpr_count', 'sgpr_count', 'private_segment_fixed_size', 'group_segment_fixed_size', 'wavefront_size')})
            assert m['private_segment_fixed_size'] == 0, (stem, key, m)
            assert m['sgpr_spill_count'] == 0 and m['vgpr_spill_count'] == 0, (stem, key, m)
            assert m['group_segment_fixed_size'] <= 64 * 1024, (stem, key, m)
            assert m['wavefront_size'] == 64 and m['max_flat_workgroup_size'] == (1024 if stem == 'select' else 256), (stem, key, m)
    for m in groups['cells'].values():
        assert m['group_segment_fixed_size'] == 0, m
    assert 32 * 1024 < groups['coeff'][None]['group_segment_fixed_size'] <= 48 * 1024   # a tile of 32 x 32 cells with an apron of 12
    assert 32 * 1024 < groups['select'][None]['group_segment_fixed_size'] <= 34 * 1024   # 32 copies of the histogram of 256 bins, their total, the sums
    assert groups['dark'][None]['group_segment_fixed_size'] == 4 * (40 * 40 + 40 * 32)


def test_lds_query_answers_the_static_size(td, metadata):
    from torch_darktable._native import lib

    others = max(kernels(metadata, stem)[None]['group_segment_fixed_size'] for stem in PLAIN)
    apply = kernels(metadata, 'apply')
    for (tag, cell), m in apply.items():
        for dark_radius, radius in ((0, 0), (1, 4), (4, 8)):
            assert lib.tdk_dehaze_lds_bytes(tag, cell, dark_radius, radius) == max(m['group_segment_fixed_size'], others), (tag, cell, dark_radius, radius)
    assert apply[(0, 2)]['group_segment_fixed_size'] > apply[(0, 4)]['group_segment_fixed_size'] > apply[(0, 16)]['group_segment_fixed_size']
    assert apply[(0, 2)]['group_segment_fixed_size'] > others > apply[(0, 4)]['group_segment_fixed_size']   # either can be the largest


def test_no_sum_is_fused_with_its_binary16_rounding():
    """out = (x - A)*rt + A is a float32 value, rounded once more at a binary16 store; v_fma_mixlo_f16 would round the exact sum once."""
    asm = kernel_isa.device_asm('dehaze')
    assert 'v_cvt_f16_f32' in asm or 'v_cvt_pk' in asm
    for fused in ('v_fma_mixlo_f16', 'v_fma_mixhi_f16', 'v_mad_mixlo_f16', 'v_mad_mixhi_f16'):
        assert fused not in asm, fused


def test_the_only_atomics_are_integer_adds_on_lds():
    asm = kernel_isa.device_asm('dehaze')
    select = kernel_isa.kernel_bodies(asm, 'dh_select')
    assert len(select) == 1
    body = '\n'.join(next(iter(select.values())))
    assert 'ds_add_u32' in body and 'ds_add_u64' in body
    for other in kernel_isa.kernel_bodies(asm, 'dh_(cells|dark|coeff|apply)').values():
        assert not any(line.startswith('ds_add') or '_atomic' in line for line in other)
    for word in ('global_atomic', 'flat_atomic', 'buffer_atomic', 'ds_add_f32', 'ds_add_rtn_f32', 'ds_cmpst'):
        assert word not in asm, word


def test_launches_and_nothing_else():
    text = SOURCE.read_text()
    assert text.count('TDK_LAUNCH(') == 5   # cells, dark, select, coefficients, apply
    for name in ('tdk_dehaze(cells)', 'tdk_dehaze(dark)', 'tdk_dehaze(select)', 'tdk_dehaze(coefficients)', 'tdk_dehaze(apply)'):
        assert f'TDK_LAUNCH("{name}"' in text, name
    assert 'hipLaunchKernelGGL' not in text and '<<<' not in text
    for call in ('hipMalloc', 'hipMemcpy', 'hipMemset', 'Synchronize', 'hipFree', 'hipHostMalloc'):
        assert call not in text, call
    assert text.count('atomicAdd(&lds.') + text.count('atomicAdd(&copy[') == text.count('atomicAdd(') == 6 and 'const copy = lds.hist +' in text and 'atomicCAS' not in text and 'atomicMax' not in text   # every one names an LDS member
    assert '__shared__' in text and 'extern __shared__' not in text   # static LDS
    assert 'toneequal.hip' not in text.replace('(csrc/toneequal.hip)', '')   # restated, not included
