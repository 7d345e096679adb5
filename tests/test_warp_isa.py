"""CPU-only (hipcc cross-compiles): the resource contract of the warp kernels (csrc/warp.hip), read from the gfx950 code-object
metadata -- kernel names and resource fields only.

  * every instantiation ({float, __half, uint8} x C in {1, 3} x {bilinear, bicubic}) and the coordinates kernel keep their state in
    registers and LDS: no private segment, no SGPR or VGPR spills;
  * at most 128 VGPRs, so registers admit four waves per SIMD (the kernels take 45 to 65, which admits seven or eight);
  * workgroups of 256 threads; the source box is dynamic LDS only -- its size is tdk_warp_lds_bytes, held to 64 KB in
    tests/test_warp_abi.py -- so the kernel never raises its dynamic-LDS limit and no call but the launch is made."""
import re
from pathlib import Path

import pytest

from kernel_isa import device_asm, metadata

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'torch-darktable_amd' / 'csrc' / 'warp.hip'


@pytest.fixture(scope='module')
def asm():
    return device_asm('warp')


def test_every_warp_kernel_lives_in_registers_and_lds(asm):
    meta = metadata(asm)
    warp = {k: v for k, v in meta.items() if 'warp_kernel' in k}
    coords = {k: v for k, v in meta.items() if 'warp_coordinates_kernel' in k}
    assert len(meta) == 13 and len(warp) == 12 and len(coords) == 1, sorted(meta)
    kinds = {re.search(r'warp_kernelI(f|6__half|h)Li([13])ELi([01])E', name).groups() for name in warp}
    assert kinds == {(t, c, i) for t in ('f', '6__half', 'h') for c in ('1', '3') for i in ('0', '1')}
    for name, m in meta.items():
        print(name, {k: m[k] for k in ('vgpr_count', 'sgpr_count', 'private_segment_fixed_size', 'group_segment_fixed_size')})
        assert m['private_segment_fixed_size'] == 0, (name, m)
        assert m['sgpr_spill_count'] == 0 and m['vgpr_spill_count'] == 0, (name, m)
        assert m['group_segment_fixed_size'] == 0, (name, m)   # the box is dynamic LDS: tdk_warp_lds_bytes
        assert m['vgpr_count'] <= 128, (name, m)
        assert m['max_flat_workgroup_size'] == 256, (name, m)


def test_one_launch_per_entry_point_and_no_other_runtime_call():
    text = SOURCE.read_text()
    assert text.count('TDK_LAUNCH(') == 2   # tdk_warp and tdk_warp_coordinates
    assert len(re.findall(r'^TDK_EXPORT int tdk_warp(_coordinates)?\(', text, flags=re.M)) == 2
    for call in ('hipMalloc', 'hipFree', 'hipMemcpy', 'hipMemset', 'hipStreamSynchronize', 'hipDeviceSynchronize', 'hipEventSynchronize',
                 'hipFuncSetAttribute', 'TDK_MAX_LDS_ONCE', 'tdk_raise_lds_limit', 'atomic'):
        assert call not in text, call
