#!/usr/bin/env python3
"""LDS round trips and register parking of one kernel from an AMDGPU assembly listing (hipcc -S --cuda-device-only with
the unit's flags): every `s_waitcnt lgkmcnt(n)` of one interior-point iteration with what it waits for, and the count of
v_accvgpr_read / v_accvgpr_write.  A wave that is alone on its SIMD has nothing to overlap a wait with: a wait that stands
right behind the ds_read it needs parks the wave for the whole LDS latency.

  python tools/isa_waits.py file.s kernel-name-substring [min-loop-size] [--summary]

Same listing and same kernel selection as tools/isa_loops.py.  The regions are the loops isa_loops.py finds inside the
iteration (the loop around the loop with MFMA, with the pieces of it that the compiler laid out behind its back edge) and
the straight-line remainder of the iteration; a kernel without such a loop is reported as one region per loop plus the remainder of the kernel.  Per wait:
  lgkmcnt  the count it waits down to
  batch    DS instructions issued since the previous lgkmcnt wait of the region
  dist     instructions between the youngest DS read the wait covers and the wait (0: directly behind it; -: no read
           outstanding).  lgkmcnt(n) leaves the n youngest LGKM instructions in flight: those are skipped.
  repeat   the wait retires a read of its own group, and the group's DS instructions are those of the previous group
           (opcode by opcode, same count waited for): the "load, drain, load, drain" pattern of loads that could have
           been issued together.  A counted wait that streams (one more load out, the oldest one in) is not one.
Instructions are taken in listing order; both sides of a branch count once, as in isa_loops.py."""
import re
import sys

CLOSE = 6      # a wait at most this many instructions behind its read has (almost) the whole LDS latency exposed
WAIT = re.compile(r'lgkmcnt\((\d+)\)')


def parse_kernel(lines, key):
    """(name, instructions in order, label -> index of the first instruction behind it) of the first kernel whose label holds key"""
    start = [i for i, l in enumerate(lines) if re.match(r'^_Z\S*:', l) and key in l][0]
    end = next(i for i in range(start, len(lines)) if lines[i].startswith('.Lfunc_end'))
    ins, label_at = [], {}
    for l in lines[start + 1:end]:
        m = re.match(r'^(\.LBB\d+_\d+):', l)
        if m:
            label_at[m.group(1)] = len(ins)
            continue
        t = l.split(';')[0].strip()
        if t and not t.startswith('.'):
            ins.append(t)
    return lines[start].split(':')[0], ins, label_at


def find_loops(ins, label_at):
    by_head = {}
    for i, t in enumerate(ins):
        p = t.split()
        if p[0].startswith(('s_cbranch', 's_branch')) and p[-1] in label_at and label_at[p[-1]] <= i:
            a = label_at[p[-1]]
            by_head[a] = max(i + 1, by_head.get(a, 0))      # back edges to one header are one loop
    return sorted(by_head.items())


def op(t):
    return t.split()[0]


def is_ds(t):
    return op(t).startswith('ds_')


def is_ds_read(t):      # what returns data through the LGKM counter to a register the wave then reads
    o = op(t)
    return o.startswith('ds_read') or 'permute' in o or o.startswith('ds_swizzle')


def is_lgkm(t):
    o = op(t)
    return o.startswith('ds_') or o.startswith('s_load') or o.startswith('s_buffer_load')


def waits_of(seq):
    """the lgkmcnt waits of an instruction sequence: dicts with at (index in seq), lgkmcnt, batch, dist, repeat"""
    out, group, prev_sig, retired, first = [], [], None, -1, 0      # retired: youngest LGKM instruction an earlier wait has retired
    for i, t in enumerate(seq):
        if is_ds(t):
            if not group:
                first = i
            group.append(op(t))
            continue
        m = WAIT.search(t) if op(t) == 's_waitcnt' else None
        if not m:
            continue
        n = int(m.group(1))
        lg = [j for j in range(retired + 1, i) if is_lgkm(seq[j])]
        covered = lg[:len(lg) - n] if n else lg      # lgkmcnt(n) leaves the n youngest in flight
        reads = [j for j in covered if is_ds_read(seq[j])]
        dist = i - reads[-1] - 1 if reads else None
        if covered:
            retired = covered[-1]
        sig = (tuple(group), n)
        out.append({'at': i, 'lgkmcnt': n, 'batch': len(group), 'dist': dist, 'repeat': bool(group) and sig == prev_sig and bool(reads) and reads[-1] >= first})
        prev_sig, group = sig, []
    return out


def agpr_moves(seq):
    return (sum(1 for t in seq if op(t).startswith('v_accvgpr_read')), sum(1 for t in seq if op(t).startswith('v_accvgpr_write')))


def summarise(ws, seq):
    rd, wr = agpr_moves(seq)
    return {'instructions': len(seq), 'waits': len(ws),
            'close': sum(1 for w in ws if w['dist'] is not None and w['dist'] <= CLOSE),
            'adjacent': sum(1 for w in ws if w['dist'] == 0),
            'repeats': sum(1 for w in ws if w['repeat']),
            'accvgpr_read': rd, 'accvgpr_write': wr}


def regions_of(ins, loops):
    """[(title, [instruction ranges])]: the loops inside the iteration and its remainder (see the module text)"""
    inner = lambda a, b: [(x, y) for x, y in loops if (x, y) != (a, b) and a <= x and y <= b]
    bw = None
    for a, b in loops:
        if inner(a, b):
            continue
        if any('mfma' in op(t) for t in ins[a:b]) and (bw is None or b - a > bw[1] - bw[0]):
            bw = (a, b)
    outer = [(a, b) for a, b in loops if bw and a <= bw[0] and bw[1] <= b and (a, b) != bw]
    if outer:
        a, b = min(outer, key=lambda r: r[1] - r[0])
        what = 'iteration'
    else:
        a, b = 0, len(ins)
        what = 'kernel'
    # the tail of the iteration (what follows its `continue`) may be laid out behind the back edge, as a loop of its own that
    # starts inside the iteration and ends behind it: such loops are pieces of the one iteration, not loops inside it
    pieces = [(a, b)]
    while what == 'iteration':
        ext = [(x, y) for x, y in loops if a < x < b < y]
        if not ext:
            break
        pieces += ext
        b = max(y for _, y in ext)
    cand = [r for r in inner(a, b) if r not in pieces]
    kids = [r for r in cand if not any(r != q and q[0] <= r[0] and r[1] <= q[1] for q in cand)]
    rest, pos = [], a
    for x, y in sorted(kids):
        rest.append((pos, x)); pos = y
    rest.append((pos, b))
    return what, (a, b), bw, sorted(kids), rest


def analyse(lines, key, minsz=60):
    """{'kernel': name, 'regions': [{'title', 'waits': [...], 'summary': {...}}], 'total': {...}}"""
    name, ins, label_at = parse_kernel(lines, key)
    label_of = {v: k for k, v in label_at.items()}
    loops = find_loops(ins, label_at)
    what, whole, bw, kids, rest = regions_of(ins, loops)
    regions, small = [], []
    for x, y in kids:
        if y - x < minsz and (x, y) != bw:
            small.append((x, y))      # short loops are reported with the remainder, as isa_loops.py leaves them out
            continue
        title = ('backward pass, one knot' if (x, y) == bw else 'loop') + f" at {label_of.get(x, '?')}"
        seq = ins[x:y]
        ws = waits_of(seq)
        regions.append({'title': title, 'waits': ws, 'summary': summarise(ws, seq)})
    ws, seq_all = [], []
    for x, y in sorted(rest + small):      # each straight-line piece on its own: a wait does not look across a loop
        seq = ins[x:y]
        for w in waits_of(seq):
            w['at'] += len(seq_all)
            ws.append(w)
        seq_all += seq
    regions.append({'title': f"one {what} outside its loops (at {label_of.get(whole[0], '?')}; every branch side counted once)",
                    'waits': ws, 'summary': summarise(ws, seq_all)})
    total = {k: sum(r['summary'][k] for r in regions) for k in regions[0]['summary']}
    return {'kernel': name, 'regions': regions, 'total': total}


def fmt_summary(s):
    return (f"{s['instructions']} instructions, {s['waits']} lgkmcnt waits: {s['close']} at most {CLOSE} behind their read "
            f"({s['adjacent']} directly behind it), {s['repeats']} repeats; v_accvgpr_read {s['accvgpr_read']}, v_accvgpr_write {s['accvgpr_write']}")


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    brief = '--summary' in sys.argv[1:]
    lines = open(args[0]).read().split('\n')
    rep = analyse(lines, args[1], int(args[2]) if len(args) > 2 else 60)
    print(f"kernel {rep['kernel']}")
    for r in rep['regions']:
        print(f"{r['title']}: {fmt_summary(r['summary'])}")
        if brief:
            continue
        for w in r['waits']:
            d = '-' if w['dist'] is None else str(w['dist'])
            print(f"    +{w['at']:5d}  lgkmcnt({w['lgkmcnt']})  batch {w['batch']:3d}  dist {d:>3s}{'  repeat' if w['repeat'] else ''}")
    print(f"total: {fmt_summary(rep['total'])}")


if __name__ == '__main__':
    main()
