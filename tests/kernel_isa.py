"""What the ISA tests (test_*_isa.py and the few like them) share: the gfx950 assembly of one csrc/*.hip file, compiled with the flags
the library is built with, the code-object metadata in it, and the bodies of its kernels."""

import functools
import re
import subprocess

from abi_header import load_build_module


@functools.lru_cache(maxsize=None)
def device_asm(stem):
    """The device-side assembly of csrc/<stem>.hip under build.CXXFLAGS; compiled once per process however many tests read it."""
    build = load_build_module()
    r = subprocess.run([build.HIPCC, *build.CXXFLAGS, '--cuda-device-only', '-S', '-o', '-', str(build.CSRC / f'{stem}.hip')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def metadata(asm):
    """{kernel: {field: value}} from the code-object metadata: one map per kernel, opened by a '  - .' line, fields in any order."""
    out = {}
    text = asm[asm.index('amdhsa.kernels:'):asm.index('.end_amdgpu_metadata')]
    for chunk in re.split(r'\n  - (?=\.)', text)[1:]:
        fields = dict(re.findall(r'^\s*\.(\w+):\s+(\S+)\s*$', chunk, flags=re.M))
        out[fields['name']] = {k: int(v) for k, v in fields.items() if v.isdigit()}
    return out


def kernel_bodies(asm, pattern):
    """{symbol: body lines, stripped, up to s_endpgm} of the kernels whose mangled name matches."""
    out, cur, name = {}, None, None
    for line in asm.split('\n'):
        m = re.match(r'^(_Z\w+):', line)
        if m and re.search(pattern, m.group(1)):
            name, cur = m.group(1), []
            continue
        if cur is not None:
            cur.append(line.strip())
            if line.strip().startswith('s_endpgm'):
                out[name] = cur
                cur = None
    return out
