"""CPU-only (hipcc cross-compiles): the resource contract of the raw-stage kernel (csrc/rawprepare.hip), read from the gfx950
code-object metadata -- kernel names and resource fields only.

  * sixteen instantiations of one kernel: input form {packed bytes, uint16, float32, binary16} x output {float32, binary16} x
    {streaming, tile with apron}.  The nibble order of the packed form, the enabled defect rules, shading, white balance and clip
    are launch constants in scalar registers (branches the whole wave takes alike), not instantiations;
  * every one keeps its state in registers and LDS: no private segment, no SGPR or VGPR spills;
  * at most 128 VGPRs, so registers admit four waves per SIMD (the kernels take about 40 to 46, which admits eight);
  * workgroups of 256 threads; LDS is dynamic only -- its size is tdk_raw_prepare_lds_bytes, held to 64 KB in
    tests/test_rawprepare_abi.py -- so the kernel never raises its dynamic-LDS limit and no call but the launch is made."""
import re
from pathlib import Path

import pytest

from kernel_isa import device_asm, metadata

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / 'torch-darktable_amd' / 'csrc' / 'rawprepare.hip'


@pytest.fixture(scope='module')
def asm():
    return device_asm('rawprepare')


def test_every_raw_kernel_lives_in_registers_and_lds(asm):
    meta = metadata(asm)
    assert len(meta) == 16 and all('raw_prepare_kernel' in k for k in meta), sorted(meta)
    # mangled template arguments: input form (NS_8RpPackedE, t = unsigned short, f, 6__half), output (f, 6__half or the
    # substitution S1_ of a repeated __half), DEFECT (Lb0E / Lb1E)
    kinds = set()
    for name in meta:
        m = re.search(r'raw_prepare_kernelI(NS_8RpPackedE|t|f|6__half)(f|6__half|S1_)Lb([01])E', name)
        assert m, name
        kinds.add((m.group(1), 'h' if m.group(2) != 'f' else 'f', m.group(3)))
    assert kinds == {(i, o, d) for i in ('NS_8RpPackedE', 't', 'f', '6__half') for o in ('f', 'h') for d in ('0', '1')}
    for name, m in meta.items():
        print(name, {k: m[k] for k in ('vgpr_count', 'sgpr_count', 'private_segment_fixed_size', 'group_segment_fixed_size')})
        assert m['private_segment_fixed_size'] == 0, (name, m)
        assert m['sgpr_spill_count'] == 0 and m['vgpr_spill_count'] == 0, (name, m)
        assert m['group_segment_fixed_size'] == 0, (name, m)   # tile, records and nodes are dynamic LDS: tdk_raw_prepare_lds_bytes
        assert m['vgpr_count'] <= 128, (name, m)
        assert m['max_flat_workgroup_size'] == 256, (name, m)


def test_one_launch_per_entry_point_and_no_other_runtime_call():
    text = SOURCE.read_text()
    assert text.count('TDK_LAUNCH(') == 1   # tdk_raw_prepare
    assert len(re.findall(r'^TDK_EXPORT int tdk_raw_prepare\(', text, flags=re.M)) == 1
    for call in ('hipMalloc', 'hipFree', 'hipMemcpy', 'hipMemset', 'hipStreamSynchronize', 'hipDeviceSynchronize', 'hipEventSynchronize',
                 'hipFuncSetAttribute', 'TDK_MAX_LDS_ONCE', 'tdk_raise_lds_limit', 'atomic'):
        assert call not in text, call
