#!/usr/bin/env python3
"""Issue-slot budget of one kernel from an AMDGPU assembly listing (hipcc -S --cuda-device-only with the unit's flags):
the instruction count per class of every loop of the kernel and of the straight-line remainder of the enclosing loop.
A wave that is alone on its SIMD issues one instruction per 4 cycles whatever its kind, so the count IS the budget.

  python tools/isa_loops.py file.s kernel-name-substring [min-loop-size]

Loops are found from the back edges of the listing (a branch to a label that stands earlier).  For the wave kernel of
the wrench form the loops are named by what only they hold: the backward pass's knot is the one with MFMA, the interior-point
iteration the loop around it, the trial rollout's knot pair the loop of the iteration with the most v_readlane and no MFMA."""
import collections
import re
import sys

ARITH = re.compile(r'^v_(fma|fmac|mul|add|rcp|rsq|min|max)_f64|^v_mfma')


def classify(t):
    o = t.split()[0]
    if 'mfma' in o: return 'mfma'
    if o.startswith('v_mov_b64_dpp'): return 'dpp_mov_b64'
    if o.startswith('v_mov_b32_dpp'): return 'dpp_mov_b32'
    if ARITH.match(o): return 'f64_arith' + ('_dpp' if '_dpp' in o else '')
    if o.startswith('v_cndmask'): return 'v_cndmask'
    if o.startswith('v_mov_b'): return 'v_mov'
    if 'readlane' in o or 'readfirstlane' in o: return 'v_readlane'
    if 'permlane' in o: return 'v_permlane'
    if 'permute' in o: return 'ds_bpermute'
    if o.startswith('ds_read'): return 'ds_read'
    if o.startswith('ds_write'): return 'ds_write'
    if o.startswith('global_') or o.startswith('flat_') or o.startswith('buffer_'): return 'vmem'
    if o.startswith('scratch_'): return 'scratch'
    if o.startswith('s_nop'): return 's_nop'
    if o.startswith('s_waitcnt'): return 's_waitcnt'
    if o.startswith('s_cbranch') or o.startswith('s_branch'): return 's_branch'
    if o.startswith('s_'): return 's_other'
    if o.startswith('v_cmp'): return 'v_cmp'
    return 'v_other'


def main():
    lines = open(sys.argv[1]).read().split('\n')
    key = sys.argv[2]
    minsz = int(sys.argv[3]) if len(sys.argv) > 3 else 60
    start = [i for i, l in enumerate(lines) if re.match(r'^_Z\S*:', l) and key in l][0]
    end = next(i for i in range(start, len(lines)) if lines[i].startswith('.Lfunc_end'))
    ins, label_at = [], {}      # instructions in order; label -> index of the first instruction after it
    for l in lines[start + 1:end]:
        m = re.match(r'^(\.LBB\d+_\d+):', l)
        if m:
            label_at[m.group(1)] = len(ins)
            continue
        t = l.split(';')[0].strip()
        if t and not t.startswith('.'):
            ins.append(t)
    loops = set()
    for i, t in enumerate(ins):
        p = t.split()
        if p[0].startswith(('s_cbranch', 's_branch')) and p[-1] in label_at and label_at[p[-1]] <= i:
            loops.add((label_at[p[-1]], i + 1))
    # back edges to one header are one loop
    by_head = {}
    for a, b in loops:
        by_head[a] = max(b, by_head.get(a, 0))
    loops = sorted(by_head.items())
    name_of = {v: k for k, v in label_at.items()}

    def count(rng_list):
        c = collections.Counter()
        for a, b in rng_list:
            for t in ins[a:b]:
                c[classify(t)] += 1
        return c

    def show(title, c):
        n = sum(c.values())
        ar = c['mfma'] + c['f64_arith'] + c['f64_arith_dpp']
        print(f"{title}: {n} instructions, {ar} FP64 arithmetic ({c['mfma']} MFMA), {n - ar} other")
        print("    " + ", ".join(f"{k} {v}" for k, v in sorted(c.items(), key=lambda kv: -kv[1])))

    print(f"kernel {lines[start].split(':')[0]}: {len(ins)} instructions")
    for l in lines[end:end + 80]:
        if re.match(r'^; (NumVgprs|NumAgprs|TotalNumVgprs|ScratchSize|Occupancy|TotalNumSgprs)', l) or 'spill' in l.lower():
            print("  " + l[2:].strip())
    inner = lambda a, b: [(x, y) for x, y in loops if (x, y) != (a, b) and a <= x and y <= b]
    bw = ro = None
    for a, b in loops:
        if inner(a, b):
            continue
        c = count([(a, b)])
        if c['mfma'] and (bw is None or sum(c.values()) > sum(count([bw]).values())):
            bw = (a, b)
    outer = [(a, b) for a, b in loops if bw and a <= bw[0] and bw[1] <= b and (a, b) != bw]
    it = min(outer, key=lambda r: r[1] - r[0]) if outer else None
    for a, b in (inner(*it) if it else []):
        c = count([(a, b)])      # (the body's two knots may show as a loop with a second back edge inside: the outer one)
        if c['v_readlane'] >= 8 and not c['mfma'] and (ro is None or c['v_readlane'] > count([ro])['v_readlane']):
            ro = (a, b)
    if bw:
        show(f"backward pass, one knot (loop at {name_of.get(bw[0], '?')})", count([bw]))
    if ro:
        show(f"trial rollout, knot loop body (loop at {name_of.get(ro[0], '?')}; two knots per trip where the operands are prefetched)", count([ro]))
    if bw:
        if it:
            a, b = it
            kids = [r for r in inner(a, b) if not any(r != q and q[0] <= r[0] and r[1] <= q[1] for q in inner(a, b))]
            rest, pos = [], a
            for x, y in sorted(kids):
                rest.append((pos, x)); pos = y
            rest.append((pos, b))
            show(f"one iteration outside its loops (loop at {name_of.get(a, '?')}; every branch side counted once)", count(rest))
            for x, y in sorted(kids):
                if (x, y) not in (bw, ro) and y - x >= minsz:
                    show(f"  other loop at {name_of.get(x, '?')}", count([(x, y)]))


if __name__ == '__main__':
    main()
