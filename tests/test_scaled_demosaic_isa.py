"""CPU-only (hipcc cross-compiles): the resource contract of the kernel of the reduced-size demosaic (csrc/scaled_demosaic.hip), read
from the gfx950 code-object metadata and the source alone.

  * every instantiation -- source kind x output type -- keeps its state in registers and LDS: no private segment, no SGPR or VGPR
    spills;
  * the LDS is static, no larger than tdk_demosaic_scaled_lds_bytes answers, at most 80 KB (two workgroups per CU);
  * they are wave64 kernels of 256 threads;
  * the source launches through one TDK_LAUNCH and holds no allocation, copy, memset or synchronisation."""
import re
from pathlib import Path

import pytest

import kernel_isa
import scaled_demosaic_spec as spec

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'torch-darktable_amd' / 'csrc' / 'scaled_demosaic.hip'
OUTPUTS = {'f': 0, '6__half': 1}   # mangled output type -> dtype tag
SOURCES = {0: 'float32', 1: 'binary16', 2: 'packed', 3: 'packed, IDS nibble order'}


@pytest.fixture(scope='module')
def metadata():
    return kernel_isa.metadata(kernel_isa.device_asm('scaled_demosaic'))


def kernels(metadata):
    """{(source kind, output dtype tag): metadata}"""
    out = {}
    for name, m in metadata.items():
        found = re.search(r'\d+scaled_demosaic_kernelILi(\d)E(f|6__half)EE', name)
        if found:
            out[(int(found.group(1)), OUTPUTS[found.group(2)])] = m
    return out


def test_every_instantiation_lives_in_registers_and_lds(td, metadata):
    from torch_darktable._native import lib

    group = kernels(metadata)
    assert set(group) == {(s, t) for s in SOURCES for t in (0, 1)} and len(metadata) == 8
    answer = lib.tdk_demosaic_scaled_lds_bytes(4096, 3072, 1024, 768)
    assert answer == spec.LDS_BYTES <= 80 * 1024
    for sizes in ((2, 2, 1, 1), (64, 32, 4, 2), (65535, 65535, 4096, 32767), (37, 22, 13, 9)):
        assert lib.tdk_demosaic_scaled_lds_bytes(*sizes) == answer, sizes
    for key, m in group.items():
        print(key, SOURCES[key[0]], {k: m[k] for k in ('vgpr_count', 'sgpr_count', 'private_segment_fixed_size', 'group_segment_fixed_size', 'wavefront_size')})
        assert m['private_segment_fixed_size'] == 0, (key, m)
        assert m['sgpr_spill_count'] == 0 and m['vgpr_spill_count'] == 0, (key, m)
        assert 0 < m['group_segment_fixed_size'] <= answer, (key, m)
        assert m['wavefront_size'] == 64 and m['max_flat_workgroup_size'] == 256, (key, m)
        assert m['vgpr_count'] <= 128, (key, m)   # two workgroups of four waves per CU (the LDS's limit) need no more than 256


def test_one_launch_and_nothing_else():
    text = SOURCE.read_text()
    assert text.count('TDK_LAUNCH(') == 1
    assert 'TDK_LAUNCH("tdk_demosaic_scaled", (scaled_demosaic_kernel<SRC, TO>)' in text
    assert 'hipLaunchKernelGGL' not in text and '<<<' not in text
    for call in ('hipMalloc', 'hipMemcpy', 'hipMemset', 'Synchronize', 'hipFree', 'hipHostMalloc', 'hipFuncSetAttribute', 'TDK_MAX_LDS_ONCE'):
        assert call not in text, call
    assert 'atomic' not in text.lower()
    assert '__shared__ SdLds lds;' in text and 'extern __shared__' not in text   # static LDS
