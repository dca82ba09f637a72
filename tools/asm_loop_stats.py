#!/usr/bin/env python3
"""Instruction mix of the innermost loop around a pattern in a hipcc --save-temps .s file.

    python tools/asm_loop_stats.py <file.s> <kernel-symbol-substring> <regex> [nth]
Counts VALU / SALU / branch / LDS / VMEM instructions in the blocks of that loop (nested
child loops excluded), i.e. the straight-line cost of one iteration.

    python tools/asm_loop_stats.py --moves <file.s> <kernel-symbol-substring> [<regex> [nth]]
The register-copy blocks of that loop: every block at the loop's own depth (child loops
excluded) that holds at least MIN_MOVES v_mov_b32 which are more than half of its
instructions, with its VALU and move counts, then the loop's totals.  Without a regex: the
same for every outermost loop of the kernel that has 200 VALU or more (the chunk loops).
Such a block is glue between two register assignments of the same state; on the path of every
iteration it is work the result does not need.
"""
import re
import sys

MIN_MOVES = 8


def kernel_lines(path, ksub):
    L = open(path).read().split('\n')
    start = next(i for i, l in enumerate(L) if re.match(r'^\S*' + re.escape(ksub) + r'\S*:', l) or (ksub in l and l.endswith(':') and not l.startswith('\t')))
    end = next(i for i in range(start, len(L)) if 's_endpgm' in L[i])
    return L[start:end]


def is_label(l):
    return re.match(r'^(\.LBB\S+:|; %bb)', l)


def loop_of(K, i):
    """(header, depth) of the loop whose own blocks include the block labelled at line i."""
    m = re.search(r'Header=(BB\S+) Depth=(\d+)', ' '.join(K[i:i + 3]))
    if m:
        return m.group(1), int(m.group(2))
    m = re.match(r'^\.L(BB\S+):', K[i])
    for j in range(i, min(i + 4, len(K))):
        d = re.search(r'Loop Header: Depth=(\d+)', K[j])
        if m and d:
            return m.group(1), int(d.group(1))
    return None


def find_loop(K, pat, nth):
    hits = [i for i, l in enumerate(K) if re.search(pat, l)]
    h = hits[nth]
    # loop header of the block containing h: walk back to the nearest label, read its "Loop: Header=" note
    blk = max(i for i in range(h + 1) if is_label(K[i]))
    hdr = None
    for i in range(blk, min(blk + 4, len(K))):
        m = re.search(r'Header=(BB\S+) Depth=(\d+)', K[i])
        if m:
            hdr, depth = m.group(1), int(m.group(2))
            break
    if hdr is None:
        m = re.match(r'^\.L(BB\S+):', K[blk])
        hdr, depth = m.group(1), 1
    return hdr, depth


def kind(t):
    if t.startswith('s_cbranch') or t.startswith('s_branch'):
        return 'branch'
    if t.startswith('s_waitcnt'):
        return 'wait'
    if t.startswith('ds_'):
        return 'lds'
    if t.startswith(('global_', 'buffer_', 'flat_', 'scratch_')):
        return 'vmem'
    if t.startswith('v_'):
        return 'valu'
    if t.startswith('s_'):
        return 'salu'
    return None


def stats(K, hdr, depth):
    # blocks belonging to this loop at this depth
    counts = dict(valu=0, salu=0, branch=0, lds=0, vmem=0, wait=0)
    blocks = 0
    cur_in = False
    for i, l in enumerate(K):
        if is_label(l):
            note = ' '.join(K[i:i + 3])
            m = re.search(r'Header=(BB\S+) Depth=(\d+)', note)
            cur_in = bool(m and m.group(1) == hdr and int(m.group(2)) == depth) or l.startswith('.L' + hdr + ':')
            blocks += cur_in
            continue
        if not cur_in:
            continue
        k = kind(l.strip())
        if k:
            counts[k] += 1
    print(f"loop {hdr} depth {depth}: {blocks} blocks", counts)


def blocks_by_loop(K):
    """{(header, depth): [(block name, instructions)]} over the loops' own blocks."""
    loops, cur = {}, None
    for i, l in enumerate(K):
        if is_label(l):
            lp = loop_of(K, i)
            cur = None
            if lp:
                m = re.match(r'^(?:\.L|; %)(\S+):', l)
                cur = []
                loops.setdefault(lp, []).append((m.group(1), cur))
            continue
        t = l.strip()
        if cur is not None and kind(t):
            cur.append(t)
    return loops


def moves(K, which):
    loops = blocks_by_loop(K)
    for (hdr, depth), blocks in loops.items():
        valu = sum(kind(t) == 'valu' for _, ins in blocks for t in ins)
        if which is None and (depth != 1 or valu < 200):
            continue
        if which is not None and (hdr, depth) != which:
            continue
        mov = sum(t.startswith('v_mov_b32') for _, ins in blocks for t in ins)
        dot = sum('dot2' in t for _, ins in blocks for t in ins)
        print(f"loop {hdr} depth {depth}: {len(blocks)} own blocks, valu {valu}, v_mov_b32 {mov}, v_dot2 {dot}")
        n = 0
        for name, ins in blocks:
            m = sum(t.startswith('v_mov_b32') for t in ins)
            if m >= MIN_MOVES and 2 * m > len(ins):
                print(f"    copy block {name}: valu {sum(kind(t) == 'valu' for t in ins)}, v_mov_b32 {m}")
                n += 1
        if n == 0:
            print("    no copy block")


def main():
    args = sys.argv[1:]
    mv = bool(args) and args[0] == '--moves'
    if mv:
        args = args[1:]
    path, ksub = args[:2]
    K = kernel_lines(path, ksub)
    if mv:
        moves(K, find_loop(K, args[2], int(args[3]) if len(args) > 3 else 0) if len(args) > 2 else None)
        return
    hdr, depth = find_loop(K, args[2], int(args[3]) if len(args) > 3 else 0)
    stats(K, hdr, depth)


if __name__ == '__main__':
    main()
