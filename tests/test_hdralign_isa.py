"""CPU-only (hipcc cross-compiles): the resource contract of the kernels of csrc/hdralign.hip, read from the gfx950 code-object metadata
alone.

  * the file compiles to exactly its kernels: the aligned merge for {float, __half} source x {float, __half} output x radius {2, 3} and
    the bracket pyramid for {float, __half} sources; every one keeps its state in registers and LDS: no private segment, no SGPR or
    VGPR spills -- the per-frame displacements, which a lane indexes with the anchor of a site, live in LDS next to the frame addresses;
  * the merge's LDS is static, at most 64 KB, exactly what tdk_hdralign_lds_bytes answers for its radius, and 64 bytes more than the
    plain merge's; the pyramid's is the 1024 bytes of the plain pyramid;
  * the merge stays within 128 vector registers: four waves per SIMD, like the plain merge;
  * the source launches through TDK_LAUNCH only, and neither it nor the two bodies it instantiates hold an allocation, copy, memset,
    synchronisation or atomic."""
import re
from pathlib import Path

import pytest

import kernel_isa

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'torch-darktable_amd' / 'csrc' / 'hdralign.hip'
SHARED = [SOURCE.with_name(name) for name in ('tdk_mosaic_tile.h', 'tdk_hdr_tile.h', 'tdk_motion_pyramid.h')]


@pytest.fixture(scope='module')
def metadata():
    return kernel_isa.metadata(kernel_isa.device_asm('hdralign'))


def merges(metadata):
    """{(source, output, radius): metadata} of the instantiations of the aligned merge."""
    out = {}
    for name, m in metadata.items():
        if 'ha_merge' not in name:
            continue
        found = re.search(r'ha_mergeI(f|6__half)(f|6__half|S\d_)Li([23])EE', name)
        assert found, name
        kinds = tuple('h' if k != 'f' else 'f' for k in found.groups()[:2])
        out[(*kinds, int(found.group(3)))] = m
    return out


def test_every_kernel_lives_in_registers_and_lds(metadata):
    tiles = merges(metadata)
    assert set(tiles) == {(s, o, r) for s in 'fh' for o in 'fh' for r in (2, 3)}
    pyramids = sorted(name for name in metadata if 'ha_merge' not in name)
    assert len(pyramids) == 2 and all('ha_pyramid' in name for name in pyramids), pyramids
    for name, m in metadata.items():
        print(name, {k: m[k] for k in ('vgpr_count', 'sgpr_count', 'private_segment_fixed_size', 'group_segment_fixed_size')})
        assert m['private_segment_fixed_size'] == 0, (name, m)
        assert m['sgpr_spill_count'] == 0 and m['vgpr_spill_count'] == 0, (name, m)
        assert 0 < m['group_segment_fixed_size'] <= 64 * 1024, (name, m)
        assert m['max_flat_workgroup_size'] == 256, (name, m)
    for key, m in tiles.items():
        assert (160 * 1024) // m['group_segment_fixed_size'] >= 2, (key, m)
        assert m['vgpr_count'] <= 128, (key, m)
    for name in pyramids:
        assert metadata[name]['group_segment_fixed_size'] == 1024, name


def test_the_lds_is_what_the_query_answers(td, metadata):
    from torch_darktable._native import lib

    for r in (2, 3):
        sizes = {m['group_segment_fixed_size'] for key, m in merges(metadata).items() if key[2] == r}
        assert sizes == {lib.tdk_hdralign_lds_bytes(r)} == {lib.tdk_hdr_lds_bytes(r) + 64}, r


def test_launches_and_nothing_else():
    text = SOURCE.read_text()
    assert text.count('TDK_LAUNCH(') == 2   # one templated launcher each
    for name in ('"tdk_hdralign_merge"', '"tdk_hdralign_pyramid"'):
        assert text.count(f'TDK_LAUNCH({name}') == 1, name
    assert 'hipLaunchKernelGGL' not in text and '<<<' not in text
    for header in SHARED:   # the bodies and the tile layer launch nothing
        shared = header.read_text()
        assert 'TDK_LAUNCH' not in shared and 'hipLaunchKernelGGL' not in shared and '<<<' not in shared, header.name
        text += shared
    for call in ('hipMalloc', 'hipMemcpy', 'hipMemset', 'Synchronize', 'atomic'):
        assert call not in text, call


def test_the_bodies_exist_once():
    """hdrmerge.hip and motion.hip keep their kernels as wrappers over the same two headers this file instantiates."""
    csrc = SOURCE.parent
    assert 'hd_merge_tile<' in (csrc / 'hdrmerge.hip').read_text() and 'hd_merge_tile<' in SOURCE.read_text()
    assert 'mo_pyramid_tile<' in (csrc / 'motion.hip').read_text() and 'mo_pyramid_tile<' in SOURCE.read_text()
    for body, header in (('void hd_merge_tile(', 'tdk_hdr_tile.h'), ('void mo_pyramid_tile(', 'tdk_motion_pyramid.h')):
        holders = [p.name for p in sorted(csrc.glob('*')) if body in p.read_text()]
        assert holders == [header], (body, holders)
