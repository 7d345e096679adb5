"""CPU-only (hipcc cross-compiles): the resource contract of the wavelet kernels (csrc/wavelet.hip), read from the gfx950
code-object metadata alone.

  * every instantiation ({float, __half} x {C = 1, C = 3, C = 3 luma/chroma}: twelve fine kernels, one or two fused scales each, and six
    coarse ones -- DESIGN.md 3.9) keeps its state in registers and LDS: no private segment, no SGPR or VGPR spills;
  * the planes are static LDS, at most 64 KB, and the largest workgroup of a call is what tdk_wavelet_lds_bytes answers;
  * at most 128 VGPRs, so registers admit four waves per SIMD of the 512-entry file."""
import re
from pathlib import Path

import pytest

import kernel_isa

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'torch-darktable_amd' / 'csrc' / 'wavelet.hip'
F32, F16, YCC = 0, 1, 1


@pytest.fixture(scope='module')
def metadata():
    return kernel_isa.metadata(kernel_isa.device_asm('wavelet'))


def kinds(metadata):
    """{(kernel, type, channels, ycc, fused scales or 0): fields}"""
    out = {}
    for name, m in metadata.items():
        fine = re.search(r'wavelet_fineI(f|6__half)Li([13])ELb([01])ELi([12])E', name)
        coarse = re.search(r'wavelet_coarseI(f|6__half)Li([13])ELb([01])E', name)
        assert fine or coarse, name
        g = (fine or coarse).groups()
        out[('fine' if fine else 'coarse', g[0], int(g[1]), int(g[2]), int(g[3]) if fine else 0)] = m
    return out


def test_every_wavelet_kernel_lives_in_registers_and_lds(metadata):
    table = kinds(metadata)
    modes = [(1, 0), (3, 0), (3, 1)]
    assert set(table) == ({('fine', t, c, y, nf) for t in ('f', '6__half') for c, y in modes for nf in (1, 2)}
                          | {('coarse', t, c, y, 0) for t in ('f', '6__half') for c, y in modes})
    assert len(metadata) == 18
    for name, m in metadata.items():
        print(name, {k: m[k] for k in ('vgpr_count', 'sgpr_count', 'private_segment_fixed_size', 'group_segment_fixed_size')})
        assert m['private_segment_fixed_size'] == 0, (name, m)
        assert m['sgpr_spill_count'] == 0 and m['vgpr_spill_count'] == 0, (name, m)
        assert 0 < m['group_segment_fixed_size'] <= 65536, (name, m)
        assert m['vgpr_count'] <= 128, (name, m)
        assert m['max_flat_workgroup_size'] == 256, (name, m)


def test_lds_query_is_the_largest_workgroup_of_the_call(metadata, td):
    from torch_darktable._native import lib

    table = kinds(metadata)
    for tag, t in ((F32, 'f'), (F16, '6__half')):
        for c, y in ((1, 0), (3, 0), (3, 1)):
            for scales in range(1, 6):
                launches = [table[('fine', t, c, y, min(scales, td.Wavelet.FUSED))]]
                if scales > td.Wavelet.FUSED:
                    launches.append(table[('coarse', t, c, y, 0)])
                want = max(m['group_segment_fixed_size'] for m in launches)
                assert lib.tdk_wavelet_lds_bytes(c, tag, scales, YCC if y else 0) == want, (t, c, y, scales, want)


def test_launches_and_nothing_else():
    text = SOURCE.read_text()
    assert text.count('TDK_LAUNCH(') == 3   # the fine launch with one or with two fused scales, and the coarse launch in its loop
    for call in ('hipMalloc', 'hipMemcpy', 'hipMemset', 'Synchronize', 'hipFuncSetAttribute', 'TDK_MAX_LDS_ONCE', 'atomic', 'extern __shared__'):
        assert call not in text, call
