"""CPU-only (hipcc cross-compiles): the resource contract of the noise-profile kernels (csrc/noiseprofile.hip), read from the gfx950
code-object metadata alone.

  * every instantiation (the gather launch for {float, __half, uint16}, the two finishing kernels, the transform for {float, __half}
    on either side x {one row, RGB, mosaic} x {forward, inverse}) keeps its state in registers and LDS: no private segment, no SGPR or
    VGPR spills;
  * the gather launch's LDS is static, below 64 KB, and exactly what tdk_noise_lds_bytes answers; the transform uses none;
  * the source launches through TDK_LAUNCH only and holds no allocation, copy, memset or synchronisation."""
import re
from pathlib import Path

import pytest

import kernel_isa

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'torch-darktable_amd' / 'csrc' / 'noiseprofile.hip'


@pytest.fixture(scope='module')
def metadata():
    return kernel_isa.metadata(kernel_isa.device_asm('noiseprofile'))


def test_every_noiseprofile_kernel_lives_in_registers_and_lds(metadata):
    gathers = {name: m for name, m in metadata.items() if 'np_gather' in name}
    transforms = {name: m for name, m in metadata.items() if 'np_vst' in name}
    others = sorted(name for name in metadata if name not in gathers and name not in transforms)
    assert len(others) == 2 and 'np_derive' in others[0] and 'np_reduce' in others[1], others
    kinds = set()
    for name in gathers:
        m = re.search(r'np_gatherI(f|6__half|t)EE', name)
        assert m, name
        kinds.add(m.group(1))
    assert kinds == {'f', '6__half', 't'} and len(gathers) == 3
    kinds = set()
    for name in transforms:
        m = re.search(r'np_vstI(ff|f6__half|6__halff|6__halfS\d_)Li([012])ELb([01])EE', name)
        assert m, name
        kinds.add((m.group(1)[:2], m.group(1), m.group(2), m.group(3)))
    assert len(kinds) == len(transforms) == 4 * 3 * 2
    for name, m in metadata.items():
        print(name, {k: m[k] for k in ('vgpr_count', 'sgpr_count', 'private_segment_fixed_size', 'group_segment_fixed_size')})
        assert m['private_segment_fixed_size'] == 0, (name, m)
        assert m['sgpr_spill_count'] == 0 and m['vgpr_spill_count'] == 0, (name, m)
        assert m['group_segment_fixed_size'] <= 64 * 1024, (name, m)
    for name, m in gathers.items():
        assert m['vgpr_count'] <= 128, (name, m)   # four waves per SIMD: the two 512-lane workgroups per compute unit
        assert m['max_flat_workgroup_size'] == 512, (name, m)
    for name, m in transforms.items():
        assert m['group_segment_fixed_size'] == 0 and m['vgpr_count'] <= 64, (name, m)   # the rows of constants stay in registers


def test_the_lds_is_what_the_query_answers(td, metadata):
    from torch_darktable._native import lib

    sizes = {m['group_segment_fixed_size'] for name, m in metadata.items() if 'np_gather' in name}
    assert sizes == {lib.tdk_noise_lds_bytes(32)} == {lib.tdk_noise_lds_bytes(2)}
    assert max(m['group_segment_fixed_size'] for m in metadata.values()) == max(sizes) <= 64 * 1024   # the gather launch is the largest


def test_launches_and_nothing_else():
    text = SOURCE.read_text()
    assert text.count('TDK_LAUNCH(') == 8   # the gather launch for the three storage types, the two finishing launches, the transform's three kinds
    assert text.count('"tdk_noise_profile(gather)"') == 3 and text.count('"tdk_noise_profile(reduce)"') == 1 and text.count('"tdk_noise_profile(derive)"') == 1
    assert text.count('TDK_LAUNCH(what, (np_vst<') == 3
    assert 'hipLaunchKernelGGL' not in text and '<<<' not in text
    for call in ('hipMalloc', 'hipMemcpy', 'hipMemset', 'Synchronize', 'atomicAdd(&rec', 'atomicAdd(counts'):
        assert call not in text, call
