"""CPU-only (hipcc cross-compiles): the resource contract of the temporal-denoiser kernels (csrc/temporal.hip), read from the gfx950
code-object metadata alone.

  * every instantiation (the filter for {float, __half} source x {float, __half} state x {float, __half} output x radius {2, 3}, the
    one-lane advance and reset kernels) keeps its state in registers and LDS: no private segment, no SGPR or VGPR spills;
  * the filter's LDS is static, at most 64 KB, and exactly what tdk_temporal_lds_bytes answers for its radius;
  * the filter stays within the registers of the waves its LDS admits: four workgroups per compute unit at radius 2 (four waves per
    SIMD: 128 registers), three at radius 3 (168);
  * the source launches through TDK_LAUNCH only and holds no allocation, copy, memset, synchronisation or atomic."""
import re
from pathlib import Path

import pytest

import kernel_isa

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'torch-darktable_amd' / 'csrc' / 'temporal.hip'
SHARED = [SOURCE.with_name('tdk_mosaic_tile.h'), SOURCE.with_name('tdk_temporal_tile.h')]


@pytest.fixture(scope='module')
def metadata():
    return kernel_isa.metadata(kernel_isa.device_asm('temporal'))


def filters(metadata):
    """{(source, state, output, radius): metadata} of the filter instantiations."""
    out = {}
    for name, m in metadata.items():
        if 'tp_filter' not in name:
            continue
        found = re.search(r'tp_filterI(f|6__half)(f|6__half|S\d_)(f|6__half|S\d_)Li([23])EE', name)
        assert found, name
        kinds = tuple('h' if k != 'f' else 'f' for k in found.groups()[:3])
        out[(*kinds, int(found.group(4)))] = m
    return out


def test_every_temporal_kernel_lives_in_registers_and_lds(metadata):
    tiles = filters(metadata)
    assert set(tiles) == {(s, a, o, r) for s in 'fh' for a in 'fh' for o in 'fh' for r in (2, 3)}
    others = sorted(name for name in metadata if 'tp_filter' not in name)
    assert len(others) == 2 and 'tp_advance' in others[0] and 'tp_reset' in others[1], others
    for name, m in metadata.items():
        print(name, {k: m[k] for k in ('vgpr_count', 'sgpr_count', 'private_segment_fixed_size', 'group_segment_fixed_size')})
        assert m['private_segment_fixed_size'] == 0, (name, m)
        assert m['sgpr_spill_count'] == 0 and m['vgpr_spill_count'] == 0, (name, m)
        assert m['group_segment_fixed_size'] <= 64 * 1024, (name, m)
    for name in others:
        assert metadata[name]['group_segment_fixed_size'] == 0 and metadata[name]['vgpr_count'] <= 8, name
    for (s, a, o, r), m in tiles.items():
        assert m['max_flat_workgroup_size'] == 256, (s, a, o, r)
        # 160 KB of LDS admit floor(160 KB / LDS) workgroups of four waves, one wave per SIMD each: 512 registers shared by that many waves
        waves = (160 * 1024) // m['group_segment_fixed_size']
        assert waves == (4 if r == 2 else 3), (r, m)
        assert m['vgpr_count'] <= (512 // waves) // 8 * 8, ((s, a, o, r), m)


def test_the_lds_is_what_the_query_answers(td, metadata):
    from torch_darktable._native import lib

    for r in (2, 3):
        sizes = {m['group_segment_fixed_size'] for key, m in filters(metadata).items() if key[3] == r}
        assert sizes == {lib.tdk_temporal_lds_bytes(r)}, r


def test_launches_and_nothing_else():
    text = SOURCE.read_text()
    assert text.count('TDK_LAUNCH(') == 3   # the filter (one templated launcher), the advance and the reset
    assert text.count('"tdk_temporal_denoise(filter)"') == 1 and text.count('"tdk_temporal_denoise(advance)"') == 1 and text.count('TDK_LAUNCH("tdk_temporal_reset"') == 1
    assert 'hipLaunchKernelGGL' not in text and '<<<' not in text
    for header in SHARED:   # the tile layer the kernels are built from launches nothing
        shared = header.read_text()
        assert 'TDK_LAUNCH' not in shared and 'hipLaunchKernelGGL' not in shared and '<<<' not in shared, header.name
        text += shared
    for call in ('hipMalloc', 'hipMemcpy', 'hipMemset', 'Synchronize', 'atomic'):
        assert call not in text, call
