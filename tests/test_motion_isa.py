"""CPU-only (hipcc cross-compiles): the resource contract of the motion kernels (csrc/motion.hip), read from the gfx950 code-object
metadata alone.

  * every kernel (the pyramid for {float, __half} sources, the match, the compensated filter for {float, __half} source x state x
    output x radius {2, 3}, the one-lane advance) keeps its state in registers and LDS: no private segment, no SGPR or VGPR spills;
  * static LDS is at most 64 KB everywhere, and the compensated filter's is exactly what tdk_temporal_lds_bytes answers for its radius:
    it shares a compute unit like the plain filter does;
  * the compensated filter stays within the register budget tests/test_temporal_isa.py holds the plain filter to: 128 at radius 2
    (four waves per SIMD), 168 at radius 3 (three);
  * the source launches through TDK_LAUNCH only and holds no allocation, copy, memset, synchronisation or atomic."""
import re
from pathlib import Path

import pytest

import kernel_isa

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'torch-darktable_amd' / 'csrc' / 'motion.hip'
SHARED = [SOURCE.with_name('tdk_mosaic_tile.h'), SOURCE.with_name('tdk_temporal_tile.h')]


@pytest.fixture(scope='module')
def metadata():
    return kernel_isa.metadata(kernel_isa.device_asm('motion'))


def filters(metadata):
    """{(source, state, output, radius): metadata} of the instantiations of the compensated filter."""
    out = {}
    for name, m in metadata.items():
        if 'mc_filter' not in name:
            continue
        found = re.search(r'mc_filterI(f|6__half)(f|6__half|S\d_)(f|6__half|S\d_)Li([23])EE', name)
        assert found, name
        kinds = tuple('h' if k != 'f' else 'f' for k in found.groups()[:3])
        out[(*kinds, int(found.group(4)))] = m
    return out


def test_every_motion_kernel_lives_in_registers_and_lds(metadata):
    tiles = filters(metadata)
    assert set(tiles) == {(s, a, o, r) for s in 'fh' for a in 'fh' for o in 'fh' for r in (2, 3)}
    others = sorted(name for name in metadata if 'mc_filter' not in name)
    assert len(others) == 4, others
    assert sum('mo_pyramid' in n for n in others) == 2 and sum('mo_match' in n for n in others) == 1 and sum('mc_advance' in n for n in others) == 1, others
    for name, m in metadata.items():
        print(name, {k: m[k] for k in ('vgpr_count', 'sgpr_count', 'private_segment_fixed_size', 'group_segment_fixed_size')})
        assert m['private_segment_fixed_size'] == 0, (name, m)
        assert m['sgpr_spill_count'] == 0 and m['vgpr_spill_count'] == 0, (name, m)
        assert m['group_segment_fixed_size'] <= 64 * 1024, (name, m)
    for name in others:
        m = metadata[name]
        if 'mc_advance' in name:
            assert m['group_segment_fixed_size'] == 0 and m['vgpr_count'] <= 8, name
        elif 'mo_match' in name:
            assert m['max_flat_workgroup_size'] == 64, name   # a wave per tile: the block (512 B) and the widest window (24 rows of 11 dwords)
            assert m['group_segment_fixed_size'] == 512 + 24 * 11 * 4, m
        else:
            assert m['max_flat_workgroup_size'] == 256 and m['group_segment_fixed_size'] == 1024, (name, m)
    for (s, a, o, r), m in tiles.items():
        assert m['max_flat_workgroup_size'] == 256, (s, a, o, r)
        assert m['vgpr_count'] <= (128 if r == 2 else 168), ((s, a, o, r), m)


def test_the_compensated_filter_has_the_lds_of_the_plain_one(td, metadata):
    from torch_darktable._native import lib

    for r in (2, 3):
        sizes = {m['group_segment_fixed_size'] for key, m in filters(metadata).items() if key[3] == r}
        assert sizes == {lib.tdk_temporal_lds_bytes(r)}, r


def test_launches_and_nothing_else():
    text = SOURCE.read_text()
    assert text.count('TDK_LAUNCH(') == 4   # the pyramid and the filter (one templated launcher each), the match and the advance
    for name in ('"tdk_motion_pyramid"', '"tdk_motion_match"', '"tdk_motion_temporal_denoise(filter)"', '"tdk_motion_temporal_denoise(advance)"'):
        assert text.count(f'TDK_LAUNCH({name}') == 1, name
    assert 'hipLaunchKernelGGL' not in text and '<<<' not in text
    for header in SHARED:   # the tile layer the compensated filter is built from launches nothing
        shared = header.read_text()
        assert 'TDK_LAUNCH' not in shared and 'hipLaunchKernelGGL' not in shared and '<<<' not in shared, header.name
        text += shared
    for call in ('hipMalloc', 'hipMemcpy', 'hipMemset', 'Synchronize', 'atomic'):
        assert call not in text, call
