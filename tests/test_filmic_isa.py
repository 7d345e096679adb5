"""CPU-only (hipcc cross-compiles): the resource contract of the tone mapping's kernel (csrc/filmic.hip), read from the gfx950
code-object metadata alone.

  * every instantiation -- two source types, three destination types, four norms -- keeps its state in registers and LDS: no private
    segment, no SGPR or VGPR spills;
  * the LDS is static, the same for all of them, what tdk_filmic_lds_bytes answers, and at most 64 KB;
  * they are wave64 kernels of 512 threads with at most 80 VGPRs, so that three workgroups share a compute unit;
  * no lerp's add is folded into its binary16 rounding (v_fma_mixlo_f16 and its kin): the specification rounds the float32 sum first;
  * float32 denormals are kept (the tables hold some, next to black);
  * no atomics;
  * the source launches once through TDK_LAUNCH and holds no allocation, copy, memset or synchronisation."""
import re
from pathlib import Path

import pytest

import kernel_isa

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'torch-darktable_amd' / 'csrc' / 'filmic.hip'
SRC = {'f': 0, '6__half': 1}
DST = {'f': 0, '6__half': 1, 'h': 2}


@pytest.fixture(scope='module')
def metadata():
    return kernel_isa.metadata(kernel_isa.device_asm('filmic'))


def kernels(metadata):
    """{(source tag, destination tag, norm): metadata}"""
    out = {}
    for name, m in metadata.items():
        found = re.search(r'13filmic_kernelI(f|6__half)(f|h|6__half|S\d_)Li(\d)EE', name)   # (S1_: binary16 again, a substitution)
        assert found, name
        out[(SRC[found.group(1)], DST.get(found.group(2), 1), int(found.group(3)))] = m
    return out


def test_every_kernel_lives_in_registers_and_lds(td, metadata):
    from torch_darktable._native import lib

    every = kernels(metadata)
    assert set(every) == {(s, d, n) for s in (0, 1) for d in (0, 1, 2) for n in (0, 1, 2, 3)} and len(metadata) == 24
    for key, m in every.items():
        print(key, {k: m[k] for k in ('vgpr_count', 'sgpr_count', 'private_segment_fixed_size', 'group_segment_fixed_size', 'wavefront_size')})
        assert m['private_segment_fixed_size'] == 0, (key, m)
        assert m['sgpr_spill_count'] == 0 and m['vgpr_spill_count'] == 0, (key, m)
        assert m['group_segment_fixed_size'] == lib.tdk_filmic_lds_bytes() == 20480 <= 64 * 1024, (key, m)
        assert m['wavefront_size'] == 64 and m['max_flat_workgroup_size'] == 512, (key, m)
        assert m['vgpr_count'] <= 80, (key, m)   # six waves per SIMD: three workgroups of eight waves per compute unit


def test_no_sum_is_fused_with_its_binary16_rounding():
    """v = G[i] + f*(G[i+1] - G[i]) is a float32 value, rounded once more at a binary16 store; v_fma_mixlo_f16 would round the exact sum once."""
    asm = kernel_isa.device_asm('filmic')
    assert 'v_cvt_f16_f32' in asm or 'v_cvt_pk' in asm
    for fused in ('v_fma_mixlo_f16', 'v_fma_mixhi_f16', 'v_mad_mixlo_f16', 'v_mad_mixhi_f16'):
        assert fused not in asm, fused
    # one rounding per written operation: no multiply-add but the fused ones of the division's own sequence (v_div_scale, v_fma,
    # v_div_fmas, v_div_fixup), which is correctly rounded as a whole
    for contracted in ('v_mad_f32', 'v_mac_f32', 'v_pk_fma_f32', 'v_pk_mul_f32', 'v_pk_add_f32'):
        assert contracted not in asm, contracted
    assert 'v_div_fixup_f32' in asm and 'v_rcp_iflag_f32' not in asm   # the correctly rounded division, not an approximate one


def test_denormals_are_kept_and_nothing_is_atomic():
    asm = kernel_isa.device_asm('filmic')
    modes = re.findall(r'\.amdhsa_float_denorm_mode_32\s+(\d)', asm)
    assert len(modes) == 24 and set(modes) == {'3'}
    for word in ('global_atomic', 'flat_atomic', 'buffer_atomic', 'ds_add', 'ds_cmpst', 'ds_max', 'ds_min'):
        assert word not in asm, word


def test_the_tables_are_read_wide():
    """A lane's T[i], T[i+1], D[i], D[i+1] come as one 16-byte LDS read (8 bytes under 'none', which takes T alone) and G[i], G[i+1]
    as one 8-byte read: no 4-byte gathers."""
    asm = kernel_isa.device_asm('filmic')
    for name, body in kernel_isa.kernel_bodies(asm, 'filmic_kernel').items():
        reads = [line.split()[0] for line in body if line.startswith('ds_read')]
        assert reads and set(reads) <= {'ds_read_b128', 'ds_read_b64', 'ds_read2_b64', 'ds_read2st64_b64'}, (name, sorted(set(reads)))


def test_one_launch_and_nothing_else():
    text = SOURCE.read_text()
    assert text.count('TDK_LAUNCH(') == 1 and 'TDK_LAUNCH("tdk_filmic"' in text
    assert 'hipLaunchKernelGGL' not in text and '<<<' not in text
    for call in ('hipMalloc', 'hipMemcpy', 'hipMemset', 'Synchronize', 'hipFree', 'hipHostMalloc', 'atomic', 'hipFuncSetAttribute', 'tdk_raise_lds_limit'):
        assert call not in text, call
    assert '__shared__' in text and 'extern __shared__' not in text   # static LDS
    assert '#include "colorlut.hip"' not in text and 'colorlut.hip"' not in text   # restated, not included
    for fn in ('logf', 'log2f', 'powf', 'expf', 'exp2f', '__logf', '__powf', '__expf'):
        assert fn + '(' not in text, fn   # no logarithm, power or exponential runs on the device
