"""CPU-only (hipcc cross-compiles): the resource contract of the colour-transform kernels (csrc/colorlut.hip), read from the gfx950
code-object metadata alone.

  * every instantiation ({float, __half, uint8} source x {float, __half, uint8} destination x {nodes in LDS, nodes in global
    memory}: the eighteen of DESIGN.md 3.11) keeps its state in registers and LDS: no private segment, no SGPR or VGPR spills;
  * at most 128 VGPRs: four waves per SIMD, the two 512-lane workgroups per compute unit the grid is sized for;
  * the tables are dynamic LDS only -- the documented size is tdk_lut_lds_bytes, at most TDK_LUT_LDS_BUDGET = 80 KB, so two workgroups
    share the 160 KB of a compute unit -- and the host raises the kernel's dynamic-LDS limit to exactly that budget."""
import re
from pathlib import Path

import pytest

import kernel_isa

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'torch-darktable_amd' / 'csrc' / 'colorlut.hip'
HEADER = ROOT / 'include' / 'tdk_hip_lut.h'


@pytest.fixture(scope='module')
def metadata():
    return kernel_isa.metadata(kernel_isa.device_asm('colorlut'))


def test_every_colorlut_kernel_lives_in_registers_and_lds(metadata):
    assert all('colorlut_kernel' in name for name in metadata), sorted(metadata)
    kinds = set()
    for name in metadata:
        m = re.search(r'colorlut_kernelI(f|6__half|h)(f|6__half|h|S\d_)Lb([01])E', name)
        assert m, name
        src, dst, staged = m.groups()
        kinds.add((src, src if dst.startswith('S') else dst, staged))     # S<n>_ is the mangler's back-reference to the first type
    types = ('f', '6__half', 'h')
    assert kinds == {(s, d, l) for s in types for d in types for l in '01'}
    design = (ROOT / 'DESIGN.md').read_text()
    stated = re.search(r'colorlut_kernel[^\n]*?\b(\w+) instantiations', design)
    assert stated and stated.group(1) == 'eighteen' and len(metadata) == 18, (stated and stated.group(0), sorted(metadata))
    for name, m in metadata.items():
        print(name, {k: m[k] for k in ('vgpr_count', 'sgpr_count', 'private_segment_fixed_size', 'group_segment_fixed_size')})
        assert m['private_segment_fixed_size'] == 0, (name, m)
        assert m['sgpr_spill_count'] == 0 and m['vgpr_spill_count'] == 0, (name, m)
        assert m['group_segment_fixed_size'] == 0, (name, m)   # the tables are dynamic LDS: tdk_lut_lds_bytes
        assert m['vgpr_count'] <= 128, (name, m)
        assert m['max_flat_workgroup_size'] == 512, (name, m)


def test_the_dynamic_lds_is_the_documented_size_and_within_80_kb(td):
    """The launch passes the very sum tdk_lut_lds_bytes returns (one helper pair in the source), the staging rule is the header's
    budget, and the limit the host raises for a kernel is that budget: a launch can never ask for more than 80 KB."""
    from torch_darktable._native import lib

    text, header = SOURCE.read_text(), HEADER.read_text()
    budget = int(re.search(r'#define TDK_LUT_LDS_BUDGET (\d+)', header).group(1))
    assert budget == 80 * 1024 and 2 * budget <= 160 * 1024
    size = 'cl_shaper_bytes(shaper_size, shaper_tables) + (cl_staged(shaper_size, shaper_tables, lut_size, flags) ? cl_node_bytes(lut_size) : 0)'
    assert size in text                                                     # tdk_lut_lds_bytes
    assert 'const size_t lds = cl_shaper_bytes(shaper_size, shaper_tables) + (staged ? cl_node_bytes(lut_size) : 0);' in text   # the launch
    assert 'const bool staged = cl_staged(shaper_size, shaper_tables, lut_size, flags);' in text
    assert '<= TDK_LUT_LDS_BUDGET;' in text and re.search(r'tdk_raise_lds_limit\([^;]*TDK_LUT_LDS_BUDGET', text)
    largest = max(lib.tdk_lut_lds_bytes(s, t, n, 0) for n in range(2, 66) for s, t in ((0, 1), (1024, 1), (1024, 3), (700, 3)))
    assert 64 * 1024 < largest <= budget
    assert lib.tdk_lut_lds_bytes(1024, 3, 17, 0) == 12 * 17 ** 3 + 12288 <= budget


def test_one_launch_per_call_and_nothing_else():
    text = SOURCE.read_text()
    assert text.count('TDK_LAUNCH(') == 1
    for call in ('hipMalloc', 'hipMemcpy', 'hipMemset', 'Synchronize', 'atomic', 'TDK_MAX_LDS_ONCE'):
        assert call not in text, call
    assert text.count('tdk_raise_lds_limit(') == 1 and 'if (lds > CL_LDS_PLAIN)' in text   # only configurations above 64 KB raise the limit
