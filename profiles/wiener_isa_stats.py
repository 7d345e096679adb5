"""Static figures of the Wiener strip kernel (csrc/tdk_wiener_ystream.h) from the gfx950 assembly of csrc/wiener.hip: registers,
spills, LDS, code bytes, and the instruction mix of the round loop (the depth-2 loop `blk`; one per body of the kernel).

  python profiles/wiener_isa_stats.py [--csrc DIR] [--asm FILE] [--kernel REGEX]

--csrc: another checkout's csrc directory (to set a parent beside a child); --asm: an assembly file made earlier with the build's
flags plus `--cuda-device-only -S`.  No GPU needed.  The loop figures are static counts over every basic block of the loop, both
sides of its branches included (the column stage and the flush rounds, the edge and the vector staging): they compare two builds of
the same source shape, they are not cycles."""

import argparse
import importlib.util
import re
import subprocess
from collections import Counter
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def build_module():
  spec = importlib.util.spec_from_file_location('tdk_build', ROOT / 'torch-darktable_amd' / 'build.py')
  m = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(m)
  return m


def assembly(csrc):
  b = build_module()
  r = subprocess.run([b.HIPCC, *b.CXXFLAGS, '--cuda-device-only', '-S', '-o', '-', str(Path(csrc) / 'wiener.hip')], capture_output=True, text=True)
  assert r.returncode == 0, r.stderr[-2000:]
  return r.stdout


def kind(op):
  if op in ('v_readlane_b32', 'v_writelane_b32'):
    return 'lane(spill)'
  if op.startswith('v_'):
    return 'VALU'
  if op.startswith(('s_waitcnt', 's_nop', 's_barrier', 's_branch', 's_cbranch', 's_setprio', 's_sleep')):
    return 'ctl'
  if op.startswith(('s_load', 's_buffer_load')):
    return 'SMEM'
  if op.startswith('s_'):
    return 'SALU'
  if op.startswith('ds_'):
    return 'LDS'
  if op.startswith(('global_', 'buffer_', 'flat_', 'scratch_')):
    return 'VMEM'
  return 'other'


def kernels(asm, pattern):
  """{symbol: (lines of the body, code bytes)}"""
  out, cur, name = {}, None, None
  for line in asm.split('\n'):
    m = re.match(r'^(_Z\w+):', line)
    if m and re.search(pattern, m.group(1)):
      name, cur = m.group(1), []
      continue
    if cur is not None:
      cur.append(line)
      m = re.search(r'; codeLenInByte = (\d+)', line)
      if m:
        out[name] = (cur, int(m.group(1)))
        cur = None
  return out


def loops(lines):
  """{header label of a depth-2 loop: Counter of instruction kinds over its blocks (deeper loops inside it included)}, and the
  Counter of the whole kernel."""
  per, whole = {}, Counter()
  header2 = None  # the loop the current block is counted under: its depth-2 loop, else 'phase A of <its depth-1 loop>'
  label = None
  for line in lines:
    s = line.strip()
    m = re.match(r'^(\.LBB\d+_\d+):', s) or re.match(r'^; %bb\.(\d+):', s)
    if m:
      label, header2 = m.group(1).lstrip('.L'), None
    if s.startswith(';') or re.match(r'^\.LBB\d+_\d+:', s):
      c = s[s.index(';'):] if ';' in s else ''
      m = re.search(r'This (?:Inner )?Loop Header: Depth=(\d+)', c)
      if m and int(m.group(1)) <= 2:
        header2 = label if int(m.group(1)) == 2 else f'phase A of {label}'
      m = re.search(r'in Loop: Header=(BB\d+_\d+) Depth=1', c)
      if m:
        header2 = f'phase A of {m.group(1)}'
      m = re.search(r'in Loop: Header=(BB\d+_\d+) Depth=2', c) or re.search(r'Parent Loop (BB\d+_\d+) Depth=2', c)
      if m:
        header2 = m.group(1)
      if s.startswith(';'):
        continue
      s = s.split(':', 1)[1].strip() if re.match(r'^\.LBB\d+_\d+:', s) else s
    if not s or s.startswith(('.', ';')) or s.endswith(':'):
      continue
    op = s.split()[0]
    if not re.match(r'^[a-z_0-9]+$', op):
      continue
    whole[kind(op)] += 1
    if header2:
      per.setdefault(header2, Counter())[kind(op)] += 1
  return per, whole


def metadata(asm):
  out = {}
  text = asm[asm.index('amdhsa.kernels:'):asm.index('.end_amdgpu_metadata')]
  for chunk in re.split(r'\n  - (?=\.)', text)[1:]:
    fields = dict(re.findall(r'^\s*\.(\w+):\s+(\S+)\s*$', chunk, flags=re.M))
    out[fields['name']] = {k: int(v) for k, v in fields.items() if v.isdigit()}
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--csrc', default=str(ROOT / 'torch-darktable_amd' / 'csrc'))
  ap.add_argument('--asm', default=None)
  ap.add_argument('--kernel', default=r'wiener_ystreamI(f|6__half)Lb0E')
  a = ap.parse_args()
  asm = Path(a.asm).read_text() if a.asm else assembly(a.csrc)
  meta = metadata(asm)
  order = ('VALU', 'SALU', 'lane(spill)', 'SMEM', 'VMEM', 'LDS', 'ctl', 'other')
  for name, (lines, code) in kernels(asm, a.kernel).items():
    md = meta[name]
    print(name)
    print(f"  vgprs {md['vgpr_count']}  sgprs {md['sgpr_count']}  vgpr spills {md['vgpr_spill_count']}  sgpr spills {md['sgpr_spill_count']}  "
          f"scratch {md['private_segment_fixed_size']} B  LDS {md['group_segment_fixed_size']} B  code {code} B")
    per, whole = loops(lines)
    print('  whole kernel: ' + '  '.join(f'{k} {whole[k]}' for k in order if whole[k]))
    for h, c in per.items():
      what = h if h.startswith('phase A') else f'round loop at {h}'
      print(f'  {what}: ' + '  '.join(f'{k} {c[k]}' for k in order if c[k]))


if __name__ == '__main__':
  main()
