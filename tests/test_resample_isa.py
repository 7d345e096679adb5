"""CPU-only (hipcc cross-compiles): the resource contract of the scaling kernels (csrc/resample.hip), read from the gfx950
code-object metadata.

  * every instantiation ({float, __half, uint8} x C in {1, 3}) keeps its state in registers and LDS: no private segment, no SGPR
    or VGPR spills;
  * at most 128 VGPRs, so registers admit four waves per SIMD of the 512-entry file (the kernels take about 60, which admits all
    eight; 128 is the contract);
  * the tile is dynamic LDS only -- its size is tdk_resample_lds_bytes, held to 80 KB over a sweep of geometries in
    tests/test_resample_abi.py -- and the kernel never raises its dynamic-LDS limit, so no call but the launch is made."""
import re
from pathlib import Path

import pytest

from kernel_isa import device_asm, metadata

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'torch-darktable_amd' / 'csrc' / 'resample.hip'


@pytest.fixture(scope='module')
def asm():
    return device_asm('resample')


def _metadata(asm):
    return {k: v for k, v in metadata(asm).items() if 'resample_kernel' in k}


def test_every_resample_kernel_lives_in_registers_and_lds(asm):
    meta = _metadata(asm)
    assert len(meta) == 6, sorted(meta)   # {float, __half, unsigned char} x C in {1, 3}
    kinds = {re.search(r'resample_kernelI(f|6__half|h)Li([13])E', name).groups() for name in meta}
    assert kinds == {(t, c) for t in ('f', '6__half', 'h') for c in ('1', '3')}
    for name, m in meta.items():
        print(name, {k: m[k] for k in ('vgpr_count', 'sgpr_count', 'private_segment_fixed_size', 'group_segment_fixed_size')})
        assert m['private_segment_fixed_size'] == 0, (name, m)
        assert m['sgpr_spill_count'] == 0 and m['vgpr_spill_count'] == 0, (name, m)
        assert m['group_segment_fixed_size'] == 0, (name, m)   # the tile is dynamic LDS: tdk_resample_lds_bytes
        assert m['vgpr_count'] <= 128, (name, m)
        assert m['max_flat_workgroup_size'] == 256, (name, m)


def test_no_scratch_instructions_and_one_launch_per_call(asm):
    assert not re.search(r'^\s*(scratch_|buffer_(load|store)\S*\s.*\boffen\b)', asm, flags=re.M)
    text = SOURCE.read_text()
    assert text.count('TDK_LAUNCH(') == 1
    for call in ('hipMalloc', 'hipMemcpy', 'hipMemset', 'hipStreamSynchronize', 'hipDeviceSynchronize', 'hipFuncSetAttribute', 'TDK_MAX_LDS_ONCE', 'atomic'):
        assert call not in text, call
