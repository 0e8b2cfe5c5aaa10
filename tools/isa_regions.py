#!/usr/bin/env python3
"""Exec-mask regions and basic blocks of one kernel from an AMDGPU assembly listing (hipcc -S --cuda-device-only with the
unit's flags).  A short-circuit `&&` / `||` or a select written as `if` in a lane-parallel phase becomes a region: the mask
is saved and narrowed (s_and_saveexec), the region is skipped when no lane is left (s_cbranch_execz) and the mask restored
behind it.  A wave that is alone on its SIMD pays an issue slot for each of these, and every region ends a basic block: the
scheduler moves nothing across it.

  python tools/isa_regions.py file.s kernel-name-substring [min-loop-size] [--summary]

Same listing, same kernel selection and same regions as tools/isa_waits.py: the loops inside one interior-point iteration
and the iteration's straight-line remainder, with the tail that is laid out behind its back edge.  Per region:
  instructions      all of them, both sides of a branch counted once
  s_and_saveexec    mask narrowed to a condition (the head of an `if` / `&&` region)
  other saveexec    s_or_saveexec, s_andn2_saveexec, ...: the `else` side of a region
  s_cbranch_exec    s_cbranch_execz / execnz
  other s_cbranch   s_cbranch_scc* / vcc* (wave-uniform tests, back edges)
  basic blocks      leaders are the region's first instruction, every target of a branch and what follows a branch
  FP64 arithmetic   tools/isa_loops.py's class: v_{fma,fmac,mul,add,rcp,rsq,min,max}_f64 and MFMA
The total line also carries the kernel's count of v_{fma,fmac,mul,add}_f64, prologue and epilogue included: the figure that
must not move when only control flow is rewritten.  Without --summary every saveexec is listed with its offset."""
import re
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from isa_waits import find_loops, op, parse_kernel, regions_of  # noqa: E402

ARITH = re.compile(r'^v_(fma|fmac|mul|add|rcp|rsq|min|max)_f64|^v_mfma')
FMA4 = re.compile(r'^v_(fma|fmac|mul|add)_f64')
KEYS = ('instructions', 'and_saveexec', 'other_saveexec', 'cbranch_exec', 'cbranch_other', 'blocks', 'f64_arith')


def is_branch(t):
    return op(t).startswith(('s_cbranch', 's_branch'))


def leaders_of(ins, label_at):
    """indices at which a basic block starts: targets of the kernel's branches and what follows a branch or s_endpgm"""
    lead = set()
    for i, t in enumerate(ins):
        if is_branch(t):
            lead.add(i + 1)
            if t.split()[-1] in label_at:
                lead.add(label_at[t.split()[-1]])
        elif op(t) == 's_endpgm':
            lead.add(i + 1)
    return lead


def count(ins, ranges, lead):
    c = dict.fromkeys(KEYS, 0)
    c['saveexec_at'] = []
    pos = 0
    for a, b in ranges:
        if b > a:
            c['blocks'] += 1 + sum(1 for i in range(a + 1, b) if i in lead)
        for i in range(a, b):
            o = op(ins[i])
            c['instructions'] += 1
            if 'saveexec' in o:
                c['and_saveexec' if o.startswith('s_and_saveexec') else 'other_saveexec'] += 1
                c['saveexec_at'].append((pos + i - a, ins[i]))
            elif o.startswith('s_cbranch_exec'):
                c['cbranch_exec'] += 1
            elif o.startswith('s_cbranch'):
                c['cbranch_other'] += 1
            if ARITH.match(o):
                c['f64_arith'] += 1
        pos += b - a
    return c


def analyse(lines, key, minsz=60):
    """{'kernel': name, 'regions': [{'title', 'summary': {...}}], 'total': {...}, 'kernel_fma4': n}"""
    name, ins, label_at = parse_kernel(lines, key)
    label_of = {v: k for k, v in label_at.items()}
    lead = leaders_of(ins, label_at)
    what, whole, bw, kids, rest = regions_of(ins, find_loops(ins, label_at))
    regions, small = [], []
    for x, y in kids:
        if y - x < minsz and (x, y) != bw:
            small.append((x, y))      # short loops are reported with the remainder, as isa_waits.py does
            continue
        title = ('backward pass, one knot' if (x, y) == bw else 'loop') + f" at {label_of.get(x, '?')}"
        regions.append({'title': title, 'summary': count(ins, [(x, y)], lead)})
    regions.append({'title': f"one {what} outside its loops (at {label_of.get(whole[0], '?')}; every branch side counted once)",
                    'summary': count(ins, sorted(rest + small), lead)})
    total = {k: sum(r['summary'][k] for r in regions) for k in KEYS}
    return {'kernel': name, 'regions': regions, 'total': total, 'kernel_fma4': sum(1 for t in ins if FMA4.match(op(t)))}


def fmt_summary(s):
    return (f"{s['instructions']} instructions, {s['f64_arith']} FP64 arithmetic; s_and_saveexec {s['and_saveexec']}, other saveexec "
            f"{s['other_saveexec']}; s_cbranch_exec {s['cbranch_exec']}, other s_cbranch {s['cbranch_other']}; {s['blocks']} basic blocks")


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    brief = '--summary' in sys.argv[1:]
    lines = open(args[0]).read().split('\n')
    rep = analyse(lines, args[1], int(args[2]) if len(args) > 2 else 60)
    print(f"kernel {rep['kernel']}")
    for r in rep['regions']:
        print(f"{r['title']}: {fmt_summary(r['summary'])}")
        if not brief:
            for at, t in r['summary']['saveexec_at']:
                print(f"    +{at:5d}  {t}")
    print(f"total: {fmt_summary(rep['total'])}; v_fma/fmac/mul/add_f64 in the whole kernel {rep['kernel_fma4']}")


if __name__ == '__main__':
    main()
