"""CPU-only (hipcc cross-compiles): the resource contract of the sharpening kernels (csrc/sharpen.hip), read from the gfx950
code-object metadata alone.

  * every instantiation ({float, __half, uint8} x {C = 1, C = 3 per channel, C = 3 luminance}: the nine of DESIGN.md 3.8) keeps its
    state in registers and LDS: no private segment, no SGPR or VGPR spills;
  * at most 128 VGPRs, so registers admit four waves per SIMD of the 512-entry file;
  * the tile is dynamic LDS only -- its size is tdk_sharpen_lds_bytes, held to 64 KB in tests/test_sharpen_abi.py -- and the kernel
    never raises its dynamic-LDS limit, so no call but the launch is made."""
import re
from pathlib import Path

import pytest

import kernel_isa

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'torch-darktable_amd' / 'csrc' / 'sharpen.hip'


@pytest.fixture(scope='module')
def metadata():
    return kernel_isa.metadata(kernel_isa.device_asm('sharpen'))


def test_every_sharpen_kernel_lives_in_registers_and_lds(metadata):
    assert all('sharpen_kernel' in name for name in metadata), sorted(metadata)
    kinds = {re.search(r'sharpen_kernelI(f|6__half|h)Li([13])ELb([01])E', name).groups() for name in metadata}
    assert kinds == {(t, c, l) for t in ('f', '6__half', 'h') for c, l in (('1', '0'), ('3', '0'), ('3', '1'))}
    design = (ROOT / 'DESIGN.md').read_text()
    stated = re.search(r'sharpen_kernel[^\n]*?\b(\w+) instantiations', design)
    assert stated and stated.group(1) == 'nine' and len(metadata) == 9, (stated and stated.group(0), sorted(metadata))
    for name, m in metadata.items():
        print(name, {k: m[k] for k in ('vgpr_count', 'sgpr_count', 'private_segment_fixed_size', 'group_segment_fixed_size')})
        assert m['private_segment_fixed_size'] == 0, (name, m)
        assert m['sgpr_spill_count'] == 0 and m['vgpr_spill_count'] == 0, (name, m)
        assert m['group_segment_fixed_size'] == 0, (name, m)   # the planes are dynamic LDS: tdk_sharpen_lds_bytes
        assert m['vgpr_count'] <= 128, (name, m)
        assert m['max_flat_workgroup_size'] == 256, (name, m)


def test_one_launch_per_call_and_nothing_else():
    text = SOURCE.read_text()
    assert text.count('TDK_LAUNCH(') == 1
    for call in ('hipMalloc', 'hipMemcpy', 'hipMemset', 'Synchronize', 'hipFuncSetAttribute', 'TDK_MAX_LDS_ONCE', 'atomic'):
        assert call not in text, call
