#!/usr/bin/env python3
"""Per-kernel comparison of two builds' gfx950 assembly (no GPU needed).

  for f in gemm gemm_h3 ...; do hipcc --offload-arch=gfx950 -O3 -std=c++17 <the library's flags> --cuda-device-only -S -o DIR/$f.s $f.hip; done
  tools/isa_table.py PARENT_DIR NEW_DIR > profiles/<name>_isa.txt

Per kernel symbol: instruction lines, VGPRs, SGPRs, LDS bytes, scratch bytes of both builds, and a class:
  identical  the kernel's text is the same once comments, labels' numbers and directives are stripped
  renamed    the same text once every register name (v12, s[4:5], a3, vcc, ...) is masked: registers renamed or operands commuted, every
             mnemonic, immediate, offset and modifier equal
  changed    anything else
Exit status 1 when a kernel gains scratch, changes its LDS size, or exists in one build only."""
import os
import re
import sys

REG = re.compile(r'\b(?:[vsa]\d+|[vsa]\[\d+:\d+\]|vcc(?:_lo|_hi)?|exec(?:_lo|_hi)?|ttmp\d+|m0)\b')
META = {'.vgpr_count': 'vgpr', '.sgpr_count': 'sgpr', '.group_segment_fixed_size': 'lds', '.private_segment_fixed_size': 'scratch'}


def parse(path):
    """-> {symbol: {'body': [instruction lines], 'vgpr': ..., ...}}"""
    kernels, cur, meta, funcs = {}, None, {}, set()
    for line in open(path):
        m = re.match(r'^\s+\.type\s+(_Z\w+),@function', line)
        if m:
            funcs.add(m.group(1))
        m = re.match(r'^(_Z\w+):', line)
        if m and m.group(1) in funcs:                  # (data symbols have labels too)
            cur = kernels.setdefault(m.group(1), {'body': []})
            continue
        s = line.split(';')[0].strip()
        if cur is not None:
            if s.startswith('.Lfunc_end'):
                cur = None
            elif s and not s.startswith('.') and not s.endswith(':'):
                cur['body'].append(re.sub(r'\s+', ' ', s))
            continue
        # amdhsa.kernels: one list item per kernel at two spaces of indentation, its keys (sorted: .name comes after the LDS size) at four
        m = re.match(r'^  (- | {2})(\.\w+):\s*(\S+)', line)
        if not m:
            continue
        if m.group(1) == '- ':
            meta = {}
        if m.group(2) == '.name':
            kernels.get(m.group(3), {}).update(meta)
            meta = kernels.get(m.group(3), {})
        elif m.group(2) in META:
            meta[META[m.group(2)]] = int(m.group(3))
    return {k: v for k, v in kernels.items() if 'vgpr' in v}


def short(sym):
    m = re.match(r'_ZN6tepose(?:\d+_GLOBAL__N_1)?(\d+)', sym) or re.match(r'_ZN6tepose12_GLOBAL__N_1(\d+)', sym)
    if not m:
        return sym
    n = int(m.group(1))
    i = m.end()
    name, rest = sym[i:i + n], sym[i + n:]
    t = re.match(r'I((?:L[ib]\d+E)+)E', rest)
    if t:
        name += '<' + ','.join(re.findall(r'L[ib](\d+)E', t.group(1))) + '>'
    return name


def main(parent, new):
    bad = 0
    print('%-14s %-44s %15s %11s %9s %15s %9s  %s' % ('file', 'kernel', 'lines', 'vgpr', 'sgpr', 'lds', 'scratch', 'class'))
    for f in sorted(os.listdir(parent)):
        if not f.endswith('.s'):
            continue
        a, b = parse(os.path.join(parent, f)), parse(os.path.join(new, f))
        for sym in sorted(set(a) | set(b)):
            if sym not in a or sym not in b:
                print('%-14s %-44s only in %s' % (f[:-2], short(sym), 'parent' if sym in a else 'new'))
                bad = 1
                continue
            ka, kb = a[sym], b[sym]
            if ka['body'] == kb['body']:
                cls = 'identical'
            elif [REG.sub('R', l) for l in ka['body']] == [REG.sub('R', l) for l in kb['body']]:
                cls = 'renamed'
            else:
                cls = 'changed'
            if kb['scratch'] > ka['scratch'] or kb['lds'] != ka['lds']:
                cls += ' FAIL'
                bad = 1
            pair = lambda k: '%d/%d' % (ka[k], kb[k])
            print('%-14s %-44s %15s %11s %9s %15s %9s  %s' % (f[:-2], short(sym), '%d/%d' % (len(ka['body']), len(kb['body'])), pair('vgpr'), pair('sgpr'),
                                                               pair('lds'), pair('scratch'), cls))
    return bad


if __name__ == '__main__':
    sys.exit(main(sys.argv[1], sys.argv[2]))
