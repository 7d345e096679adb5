"""CPU-only (hipcc cross-compiles): the resource contract of the highlight kernels (csrc/highlights.hip), read from the gfx950
code-object metadata alone.

  * every instantiation (the statistics launch per input type, the apply and the clip launch per input and output type, and the
    finishing launch: eleven kernels -- DESIGN.md 3.10) keeps its state in registers and static LDS: no private segment, no SGPR or
    VGPR spills;
  * LDS at most 64 KB, none at all in the streaming clip launch, and the largest workgroup of a call is what
    tdk_highlights_lds_bytes answers;
  * at most 128 VGPRs, so registers admit four waves per SIMD of the 512-entry file."""
import re
from pathlib import Path

import pytest

import kernel_isa

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'torch-darktable_amd' / 'csrc' / 'highlights.hip'
CLIP, OPPOSED = 0, 1


@pytest.fixture(scope='module')
def metadata():
    return kernel_isa.metadata(kernel_isa.device_asm('highlights'))


def kinds(metadata):
    """{(kernel, its template types): fields}"""
    out = {}
    for name, m in metadata.items():
        k = re.search(r'hl_(stats|apply|clip)I((?:f|6__half|S\d_)+)E', name) or re.search(r'hl_(finish)()E', name)
        assert k, name
        out[(k.group(1), k.group(2))] = m
    return out


def test_every_highlights_kernel_lives_in_registers_and_lds(metadata):
    table = kinds(metadata)
    assert len(metadata) == 11 and len(table) == 11
    assert sorted(k for k, _ in table) == ['apply'] * 4 + ['clip'] * 4 + ['finish'] + ['stats'] * 2
    for name, m in metadata.items():
        print(name, {k: m[k] for k in ('vgpr_count', 'sgpr_count', 'private_segment_fixed_size', 'group_segment_fixed_size')})
        assert m['private_segment_fixed_size'] == 0, (name, m)
        assert m['sgpr_spill_count'] == 0 and m['vgpr_spill_count'] == 0, (name, m)
        assert m['group_segment_fixed_size'] <= 65536, (name, m)
        assert m['vgpr_count'] <= 128, (name, m)
        assert m['max_flat_workgroup_size'] == 256, (name, m)
    for (kind, _), m in table.items():
        assert (m['group_segment_fixed_size'] == 0) == (kind == 'clip'), (kind, m)


def test_lds_query_is_the_largest_workgroup_of_the_call(metadata, td):
    from torch_darktable._native import lib

    table = kinds(metadata)
    opposed = max(m['group_segment_fixed_size'] for (kind, _), m in table.items() if kind in ('stats', 'apply', 'finish'))
    assert lib.tdk_highlights_lds_bytes(OPPOSED) == opposed
    assert lib.tdk_highlights_lds_bytes(CLIP) == max(m['group_segment_fixed_size'] for (kind, _), m in table.items() if kind == 'clip') == 0


def test_launches_and_nothing_else():
    text = SOURCE.read_text()
    assert text.count('TDK_LAUNCH(') == 4   # statistics, finish, clip, apply
    for call in ('hipMalloc', 'hipMemcpy', 'hipMemset', 'Synchronize', 'hipFuncSetAttribute', 'TDK_MAX_LDS_ONCE', 'atomic', 'extern __shared__'):
        assert call not in text, call
