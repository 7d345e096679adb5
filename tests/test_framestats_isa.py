"""CPU-only (hipcc cross-compiles): the resource contract of the frame-statistics kernels (csrc/framestats.hip), read from the gfx950
code-object metadata alone.

  * every instantiation (the gather launch for {float, __half, uint8, uint16} x {1-channel image, 3-channel image, mosaic}, and the
    two finishing kernels) keeps its state in registers and LDS: no private segment, no SGPR or VGPR spills;
  * the gather launch's LDS is static, below 64 KB, and exactly what tdk_framestats_lds_bytes answers;
  * the source launches through TDK_LAUNCH only and holds no allocation, copy, memset or synchronisation."""
import re
from pathlib import Path

import pytest

import kernel_isa

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'torch-darktable_amd' / 'csrc' / 'framestats.hip'


@pytest.fixture(scope='module')
def metadata():
    return kernel_isa.metadata(kernel_isa.device_asm('framestats'))


def test_every_framestats_kernel_lives_in_registers_and_lds(metadata):
    gathers = {name: m for name, m in metadata.items() if 'fs_gather' in name}
    others = sorted(name for name in metadata if name not in gathers)
    assert len(others) == 2 and 'fs_derive' in others[0] and 'fs_reduce' in others[1], others
    kinds = set()
    for name in gathers:
        m = re.search(r'fs_gatherI(f|6__half|h|t)Li([012])EE', name)
        assert m, name
        kinds.add(m.groups())
    assert kinds == {(t, k) for t in ('f', '6__half', 'h', 't') for k in '012'} and len(gathers) == 12
    for name, m in metadata.items():
        print(name, {k: m[k] for k in ('vgpr_count', 'sgpr_count', 'private_segment_fixed_size', 'group_segment_fixed_size')})
        assert m['private_segment_fixed_size'] == 0, (name, m)
        assert m['sgpr_spill_count'] == 0 and m['vgpr_spill_count'] == 0, (name, m)
        assert m['group_segment_fixed_size'] <= 64 * 1024, (name, m)
    for name, m in gathers.items():
        assert m['vgpr_count'] <= 128, (name, m)   # four waves per SIMD: the two 512-lane workgroups per compute unit
        assert m['max_flat_workgroup_size'] == 512, (name, m)


def test_the_lds_is_what_the_query_answers(td, metadata):
    from torch_darktable._native import lib

    sizes = {m['group_segment_fixed_size'] for name, m in metadata.items() if 'fs_gather' in name}
    assert sizes == {lib.tdk_framestats_lds_bytes(256, 3)} == {lib.tdk_framestats_lds_bytes(1024, 1)}
    assert max(m['group_segment_fixed_size'] for m in metadata.values()) == max(sizes) <= 64 * 1024   # the gather launch is the largest


def test_launches_and_nothing_else():
    text = SOURCE.read_text()
    assert text.count('TDK_LAUNCH(') == 5   # the gather launch for the three frame kinds, the two finishing launches
    assert text.count('"tdk_framestats(gather)"') == 3 and text.count('"tdk_framestats(reduce)"') == 1 and text.count('"tdk_framestats(derive)"') == 1
    assert 'hipLaunchKernelGGL' not in text and '<<<' not in text
    for call in ('hipMalloc', 'hipMemcpy', 'hipMemset', 'Synchronize'):
        assert call not in text, call
