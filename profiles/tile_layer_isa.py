"""Resources of every instantiation of the three mosaic tile kernels (tp_filter, mc_filter, hd_merge), from a cross-compile: no GPU.

  python profiles/tile_layer_isa.py [--parent FILE] > profiles/r23/tile_layer_isa.txt
  python profiles/tile_layer_isa.py --stems sharpen,deconv,... [--parent FILE] > profiles/r29/frame_layer_isa.txt

One row per instantiation: VGPRs, SGPRs, LDS bytes, private segment, SGPR and VGPR spills from the code-object metadata, and the static
instruction count of the body (labels, directives and comments left out; loops and branches not weighted).  --parent FILE: the output of
this script on another tree (run there without --parent); its numbers are set beside these, with the difference in instructions.
--stems a,b: every kernel of csrc/a.hip and csrc/b.hip in place of the three tile kernels, named stem:symbol, with a digest of the body's
text as a last column; beside a parent, a row then ends in "identical" (the numbers and the body, line for line) or "DIFFERS"."""
import argparse
import hashlib
import re
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / 'tests'))
import kernel_isa  # noqa: E402

KERNELS = {'temporal': 'tp_filter', 'motion': 'mc_filter', 'hdrmerge': 'hd_merge'}
FIELDS = ('vgpr_count', 'sgpr_count', 'group_segment_fixed_size', 'private_segment_fixed_size', 'sgpr_spill_count', 'vgpr_spill_count')


def key(symbol, kernel):
    """'tp_filter<f,h,h,2>' of a mangled instantiation: f = float, h = __half (spelled out or as a substitution)."""
    found = re.search(kernel + r'I((?:f|6__half|S\d_)+)Li([23])EE', symbol)
    kinds = ['f' if k == 'f' else 'h' for k in re.findall(r'f|6__half|S\d_', found.group(1))]
    return f'{kernel}<{",".join(kinds)},{found.group(2)}>'


def rows(stems=()):
    out = {}
    for stem, kernel in ((s, '.') for s in stems) if stems else KERNELS.items():
        asm = kernel_isa.device_asm(stem)
        meta = kernel_isa.metadata(asm)
        for symbol, body in kernel_isa.kernel_bodies(asm, kernel).items():
            insns = sum(1 for line in body if line and not line.startswith(('.', ';', '//')) and not re.match(r'^[\w.$]+:', line))
            out[f'{stem}:{symbol}' if stems else key(symbol, kernel)] = [*(meta[symbol][f] for f in FIELDS), insns]
            if stems:
                out[f'{stem}:{symbol}'].append(hashlib.sha256('\n'.join(body).encode()).hexdigest()[:16])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default='')
    ap.add_argument('--stems', default='', help='comma-separated csrc stems: all their kernels, with a digest of each body')
    a = ap.parse_args()
    stems = tuple(s for s in a.stems.split(',') if s)
    parent = {}
    if a.parent:
        for line in Path(a.parent).read_text().splitlines():
            if line and not line.startswith('#'):
                name, *numbers = line.split()
                parent[name] = [int(n) for n in numbers[:7]] + numbers[7:8]
    head = '# kernel vgpr sgpr lds private sgpr_spill vgpr_spill instructions' + (' body' if stems else '')
    print(head + (' | parent: vgpr sgpr lds private sgpr_spill vgpr_spill instructions | instructions - parent' if parent else ''))
    mine = rows(stems)
    assert not parent or set(parent) == set(mine), sorted(set(parent) ^ set(mine))
    for name, r in sorted(mine.items()):
        line = f'{name:24s} ' + ' '.join(f'{n:5d}' if isinstance(n, int) else n for n in r)
        if parent:
            p = parent[name]
            line += ' | ' + ' '.join(f'{n:5d}' for n in p[:7]) + f' | {r[6] - p[6]:+d}' + ((' identical' if r == p else ' DIFFERS') if stems else '')
        print(line)


if __name__ == '__main__':
    main()
