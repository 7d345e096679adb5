"""CPU-only (hipcc cross-compiles): the resource contract of the raw codec's kernels (csrc/rawcodec.hip), read from the gfx950
code-object metadata alone.

  * every instantiation -- measure and pack per source form (uint16, packed, packed IDS), the scan, unpack per output form (uint16,
    float32, float16, packed, packed IDS) -- keeps its state in registers and LDS: no private segment, no SGPR or VGPR spills;
  * the LDS is static and at most 64 KB: none for measure and pack, 1 KB per wave for unpack;
  * they are wave64 kernels;
  * the source launches through TDK_LAUNCH only and holds no allocation, copy, memset, synchronisation or atomic."""
import re
from pathlib import Path

import pytest

import kernel_isa

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'torch-darktable_amd' / 'csrc' / 'rawcodec.hip'


@pytest.fixture(scope='module')
def metadata():
    return kernel_isa.metadata(kernel_isa.device_asm('rawcodec'))


def kernels(metadata, stem):
    """{format tag (None for a kernel that is no template): metadata} of the kernels called rc_<stem>."""
    out = {}
    for name, m in metadata.items():
        found = re.search(rf'\d+rc_{stem}(?:ILi(\d)E)?E', name)
        if found:
            out[None if found.group(1) is None else int(found.group(1))] = m
    return out


def test_every_kernel_lives_in_registers_and_lds(metadata):
    measure, scan, pack, unpack = (kernels(metadata, stem) for stem in ('measure', 'scan', 'pack', 'unpack'))
    assert set(measure) == set(pack) == {0, 1, 2} and set(scan) == {None} and set(unpack) == {0, 1, 2, 3, 4}
    assert len(metadata) == 3 + 1 + 3 + 5
    for stem, group in (('measure', measure), ('scan', scan), ('pack', pack), ('unpack', unpack)):
        for tag, m in group.items():
            print(stem, tag, {k: m[k] for k in ('vgpr_count', 'sgpr_count', 'private_segment_fixed_size', 'group_segment_fixed_size', 'wavefront_size')})
            assert m['private_segment_fixed_size'] == 0, (stem, tag, m)
            assert m['sgpr_spill_count'] == 0 and m['vgpr_spill_count'] == 0, (stem, tag, m)
            assert m['group_segment_fixed_size'] <= 64 * 1024, (stem, tag, m)
            assert m['wavefront_size'] == 64, (stem, tag, m)
    for m in (*measure.values(), *pack.values()):
        assert m['group_segment_fixed_size'] == 0 and m['max_flat_workgroup_size'] == 256, m
    for m in unpack.values():
        assert 16 * 1024 <= m['group_segment_fixed_size'] <= 17 * 1024 and m['max_flat_workgroup_size'] == 1024, m   # 16 waves, 1 KB of payload each
    assert scan[None]['max_flat_workgroup_size'] == 1024 and 0 < scan[None]['group_segment_fixed_size'] <= 256


def test_launches_and_nothing_else():
    text = SOURCE.read_text()
    assert text.count('TDK_LAUNCH(') == 4   # measure, scan, pack; unpack
    for name in ('tdk_rawcodec_measure', 'tdk_rawcodec_scan', 'tdk_rawcodec_pack', 'tdk_rawcodec_unpack'):
        assert f'TDK_LAUNCH("{name}"' in text, name
    assert 'hipLaunchKernelGGL' not in text and '<<<' not in text
    for call in ('hipMalloc', 'hipMemcpy', 'hipMemset', 'Synchronize', 'atomic'):
        assert call not in text, call
