"""CPU-only (hipcc cross-compiles): the resource contract of the bracket-merge kernel (csrc/hdrmerge.hip), read from the gfx950
code-object metadata alone.

  * every instantiation ({float, __half} source x {float, __half} output x radius {2, 3}) keeps its state in registers and LDS: no
    private segment, no SGPR or VGPR spills -- the frame addresses and exposure ratios, which a lane indexes with the anchor of a site,
    live in LDS and not in an indexed register array;
  * its LDS is static, at most 64 KB (at least two workgroups share a compute unit), and exactly what tdk_hdr_lds_bytes answers for
    its radius;
  * it stays within 128 vector registers: four waves per SIMD;
  * the source launches through TDK_LAUNCH only, once, and holds no allocation, copy, memset, synchronisation or atomic."""
import re
from pathlib import Path

import pytest

import kernel_isa

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'torch-darktable_amd' / 'csrc' / 'hdrmerge.hip'
SHARED = [SOURCE.with_name('tdk_mosaic_tile.h')]


@pytest.fixture(scope='module')
def metadata():
    return kernel_isa.metadata(kernel_isa.device_asm('hdrmerge'))


def merges(metadata):
    """{(source, output, radius): metadata} of the instantiations."""
    out = {}
    for name, m in metadata.items():
        found = re.search(r'hd_mergeI(f|6__half)(f|6__half|S\d_)Li([23])EE', name)
        assert found, name
        kinds = tuple('h' if k != 'f' else 'f' for k in found.groups()[:2])
        out[(*kinds, int(found.group(3)))] = m
    return out


def test_every_merge_kernel_lives_in_registers_and_lds(metadata):
    tiles = merges(metadata)
    assert set(tiles) == {(s, o, r) for s in 'fh' for o in 'fh' for r in (2, 3)} and len(metadata) == 8
    for key, m in tiles.items():
        print(key, {k: m[k] for k in ('vgpr_count', 'sgpr_count', 'private_segment_fixed_size', 'group_segment_fixed_size')})
        assert m['private_segment_fixed_size'] == 0, (key, m)
        assert m['sgpr_spill_count'] == 0 and m['vgpr_spill_count'] == 0, (key, m)
        assert 0 < m['group_segment_fixed_size'] <= 64 * 1024, (key, m)
        assert (160 * 1024) // m['group_segment_fixed_size'] >= 2, (key, m)
        assert m['max_flat_workgroup_size'] == 256, (key, m)
        assert m['vgpr_count'] <= 128, (key, m)


def test_the_lds_is_what_the_query_answers(td, metadata):
    from torch_darktable._native import lib

    for r in (2, 3):
        sizes = {m['group_segment_fixed_size'] for key, m in merges(metadata).items() if key[2] == r}
        assert sizes == {lib.tdk_hdr_lds_bytes(r)}, r


def test_launches_and_nothing_else():
    text = SOURCE.read_text()
    assert text.count('TDK_LAUNCH(') == 1 and text.count('TDK_LAUNCH("tdk_hdr_merge"') == 1   # one templated launcher
    assert 'hipLaunchKernelGGL' not in text and '<<<' not in text
    for header in SHARED:   # the tile layer the kernel is built from launches nothing
        shared = header.read_text()
        assert 'TDK_LAUNCH' not in shared and 'hipLaunchKernelGGL' not in shared and '<<<' not in shared, header.name
        text += shared
    for call in ('hipMalloc', 'hipMemcpy', 'hipMemset', 'Synchronize', 'atomic'):
        assert call not in text, call
