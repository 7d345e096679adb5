"""CPU-only (hipcc cross-compiles): the resource contract of the non-local-means kernels (csrc/nlmeans.hip), read from the gfx950
code-object metadata and ISA.

  * every instantiation ({float, __half} x C in {1, 3} x P in 1..4) keeps its state in registers and LDS: no private segment, no
    SGPR or VGPR spills;
  * at most 168 VGPRs, so registers admit the three workgroups (three waves per SIMD) the LDS admits at the default radii;
  * the tile is dynamic LDS only, and for every legal (S, P, C) it is at most 80 KB, so at least two workgroups share a CU;
  * the horizontal half of the patch sum is 2P whole-wave DPP adds per output row -- no LDS round trip, no permute."""
import re

import pytest

from kernel_isa import device_asm, kernel_bodies, metadata

ROWS = 8   # output rows per lane (NLM_ROWS)


@pytest.fixture(scope='module')
def asm():
    return device_asm('nlmeans')


def _metadata(asm):
    return {k: v for k, v in metadata(asm).items() if 'nlmeans' in k}


def test_every_nlmeans_kernel_lives_in_registers_and_lds(asm):
    meta = _metadata(asm)
    assert len(meta) == 16, sorted(meta)   # {float, __half} x C in {1, 3} x P in 1..4
    for name, m in meta.items():
        assert m['private_segment_fixed_size'] == 0, (name, m)
        assert m['sgpr_spill_count'] == 0 and m['vgpr_spill_count'] == 0, (name, m)
        assert m['group_segment_fixed_size'] == 0, (name, m)   # the tile is dynamic LDS: tdk_nlmeans_lds_bytes
        assert m['vgpr_count'] <= 168, (name, m)


def test_lds_leaves_room_for_two_workgroups_per_cu(td):
    from torch_darktable._native import lib

    for c in (1, 3):
        for s in range(1, 11):
            for p in range(1, 5):
                assert 0 < lib.tdk_nlmeans_lds_bytes(s, p, c) <= 80 * 1024, (s, p, c)
    assert 3 * lib.tdk_nlmeans_lds_bytes(7, 2, 3) <= 160 * 1024   # the default radii: three workgroups per CU


def test_horizontal_patch_sum_is_dpp(asm):
    bodies = kernel_bodies(asm, r'^_Z\w*nlmeans_kernel\w+$')
    assert len(bodies) == 16
    for name, body in bodies.items():
        p = int(re.search(r'Li[13]ELi(\d)E', name).group(1))
        left = sum(l.startswith('v_add_f32_dpp') and 'wave_shr:1' in l for l in body)
        right = sum(l.startswith('v_add_f32_dpp') and 'wave_shl:1' in l for l in body)
        assert left == right == p * ROWS, (name, left, right)
        assert not any(l.startswith(('ds_bpermute', 'ds_permute', 'ds_swizzle', 'v_readlane')) for l in body), name
        assert sum(l.startswith('v_exp_f32') for l in body) == ROWS, name
