"""CPU-only (hipcc cross-compiles): the resource contract of the chromatic-aberration kernels (csrc/cacorrect.hip), read from the gfx950
code-object metadata alone.

  * every instantiation of the correction ({float, __half} source x {float, __half} output x {bilinear, bicubic}), the two gather
    kernels and the finishing kernel keep their state in registers and LDS: no private segment, no SGPR or VGPR spills;
  * the LDS is static, at most 64 KB, and for the correction exactly what tdk_ca_lds_bytes answers for its interpolation;
  * they stay within 128 vector registers;
  * the source launches through TDK_LAUNCH only and holds no allocation, copy, memset, synchronisation or atomic."""
import re
from pathlib import Path

import pytest

import chromatic_spec as spec
import kernel_isa

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'torch-darktable_amd' / 'csrc' / 'cacorrect.hip'


@pytest.fixture(scope='module')
def metadata():
    return kernel_isa.metadata(kernel_isa.device_asm('cacorrect'))


def corrections(metadata):
    """{(source, output, cubic): metadata} of the instantiations of ca_correct."""
    out = {}
    for name, m in metadata.items():
        found = re.search(r'ca_correctI(f|6__half)(f|6__half|S\d_)Lb([01])EE', name)
        if found:
            kinds = tuple('h' if k != 'f' else 'f' for k in found.groups()[:2])
            out[(*kinds, int(found.group(3)))] = m
    return out


def test_every_kernel_lives_in_registers_and_lds(metadata):
    tiles = corrections(metadata)
    assert set(tiles) == {(s, o, c) for s in 'fh' for o in 'fh' for c in (0, 1)}
    others = {name: m for name, m in metadata.items() if 'ca_correct' not in name}
    assert len(others) == 3 and sum('ca_gather' in name for name in others) == 2 and sum('ca_finish' in name for name in others) == 1
    for key, m in {**tiles, **others}.items():
        print(key, {k: m[k] for k in ('vgpr_count', 'sgpr_count', 'private_segment_fixed_size', 'group_segment_fixed_size')})
        assert m['private_segment_fixed_size'] == 0, (key, m)
        assert m['sgpr_spill_count'] == 0 and m['vgpr_spill_count'] == 0, (key, m)
        assert 0 < m['group_segment_fixed_size'] <= 64 * 1024, (key, m)
        assert m['max_flat_workgroup_size'] == 256, (key, m)
        assert m['vgpr_count'] <= 128, (key, m)


def test_the_lds_is_what_the_query_answers(td, metadata):
    from torch_darktable._native import lib

    for cubic in (0, 1):
        sizes = {m['group_segment_fixed_size'] for key, m in corrections(metadata).items() if key[2] == cubic}
        assert sizes == {lib.tdk_ca_lds_bytes(cubic, 0)} == {lib.tdk_ca_lds_bytes(cubic, 1)} == {spec.lds_bytes(cubic)}, cubic


def test_launches_and_nothing_else():
    text = SOURCE.read_text()
    assert text.count('TDK_LAUNCH(') == 4   # the correction (two interpolations), the gather, the finish
    for name in ('tdk_ca_correct', 'tdk_ca_gather', 'tdk_ca_finish'):
        assert f'TDK_LAUNCH("{name}"' in text, name
    assert 'hipLaunchKernelGGL' not in text and '<<<' not in text
    for call in ('hipMalloc', 'hipMemcpy', 'hipMemset', 'Synchronize', 'atomic'):
        assert call not in text, call
