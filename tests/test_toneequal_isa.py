"""CPU-only (hipcc cross-compiles): the resource contract of the tone equalizer's kernels (csrc/toneequal.hip), read from the gfx950
code-object metadata alone.

  * every instantiation -- te_cells and te_apply per storage type and cell size, te_coeff -- keeps its state in registers and LDS:
    no private segment, no SGPR or VGPR spills;
  * the LDS is static and at most 64 KB: none for te_cells, the staged tiles for the two others, and what tdk_toneeq_lds_bytes
    answers is the largest of a call;
  * they are wave64 kernels;
  * no product is folded into its binary16 rounding (v_fma_mixlo_f16 and its kin): the specification rounds the float32 product first;
  * the source launches three times through TDK_LAUNCH and holds no allocation, copy, memset, synchronisation or atomic."""
import re
from pathlib import Path

import pytest

import kernel_isa

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'torch-darktable_amd' / 'csrc' / 'toneequal.hip'
TYPES = {'f': 0, '6__half': 1}   # mangled storage type -> dtype tag
CELLS = (2, 4, 8, 16)


@pytest.fixture(scope='module')
def metadata():
    return kernel_isa.metadata(kernel_isa.device_asm('toneequal'))


def kernels(metadata, stem):
    """{(dtype tag, cell) or None for a kernel that is no template: metadata} of the kernels called te_<stem>."""
    out = {}
    for name, m in metadata.items():
        found = re.search(rf'\d+te_{stem}(?:I(f|6__half)Li(\d+)EE)?E', name)
        if found:
            out[None if found.group(1) is None else (TYPES[found.group(1)], int(found.group(2)))] = m
    return out


def test_every_kernel_lives_in_registers_and_lds(metadata):
    cells, coeff, apply = (kernels(metadata, stem) for stem in ('cells', 'coeff', 'apply'))
    every = {(t, s) for t in TYPES.values() for s in CELLS}
    assert set(cells) == set(apply) == every and set(coeff) == {None}
    assert len(metadata) == 8 + 1 + 8
    for stem, group in (('cells', cells), ('coeff', coeff), ('apply', apply)):
        for key, m in group.items():
            print(stem, key, {k: m[k] for k in ('vgpr_count', 'sgpr_count', 'private_segment_fixed_size', 'group_segment_fixed_size', 'wavefront_size')})
            assert m['private_segment_fixed_size'] == 0, (stem, key, m)
            assert m['sgpr_spill_count'] == 0 and m['vgpr_spill_count'] == 0, (stem, key, m)
            assert m['group_segment_fixed_size'] <= 64 * 1024, (stem, key, m)
            assert m['wavefront_size'] == 64 and m['max_flat_workgroup_size'] == 256, (stem, key, m)
    for m in cells.values():
        assert m['group_segment_fixed_size'] == 0, m
    assert 16 * 1024 < coeff[None]['group_segment_fixed_size'] <= 32 * 1024


def test_lds_query_answers_the_static_size(td, metadata):
    from torch_darktable._native import lib

    coeff, apply = kernels(metadata, 'coeff')[None], kernels(metadata, 'apply')
    for (tag, cell), m in apply.items():
        for radius in (0, 4, 8):
            assert lib.tdk_toneeq_lds_bytes(tag, cell, radius) == max(m['group_segment_fixed_size'], coeff['group_segment_fixed_size']), (tag, cell, radius)
    assert apply[(0, 2)]['group_segment_fixed_size'] > apply[(0, 4)]['group_segment_fixed_size'] > apply[(0, 16)]['group_segment_fixed_size']


def test_no_product_is_fused_with_its_binary16_rounding():
    """out = x * gain is a float32 value, rounded once more at a binary16 store; v_fma_mixlo_f16 would round the exact product once."""
    asm = kernel_isa.device_asm('toneequal')
    assert 'v_cvt_f16_f32' in asm or 'v_cvt_pk' in asm
    for fused in ('v_fma_mixlo_f16', 'v_fma_mixhi_f16', 'v_mad_mixlo_f16', 'v_mad_mixhi_f16'):
        assert fused not in asm, fused


def test_launches_and_nothing_else():
    text = SOURCE.read_text()
    assert text.count('TDK_LAUNCH(') == 3   # cells, coefficients, apply
    for name in ('tdk_toneeq(cells)', 'tdk_toneeq(coefficients)', 'tdk_toneeq(apply)'):
        assert f'TDK_LAUNCH("{name}"' in text, name
    assert 'hipLaunchKernelGGL' not in text and '<<<' not in text
    for call in ('hipMalloc', 'hipMemcpy', 'hipMemset', 'Synchronize', 'atomic'):
        assert call not in text, call
    assert '__shared__' in text and 'extern __shared__' not in text   # static LDS
