"""bnflac_resync_plan_host: the rule of bnflac_index_streams_resync on host tables, no GPU.

The reference is a restatement of the rule in Python integers (include/bnflac.h states it): hand-made
candidate tables for every branch, then a few thousand random ones.  Then the refusals, and the
rule's own code (csrc/bnf_resync.h) in a program of its own under AddressSanitizer and UBSan.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from birdnest.audio_amd import libflac
from tests.test_select_ranges_host import CANARY, ROOT, _cxx

M64 = (1 << 64) - 1
U32 = (1 << 32) - 1
RESYNCED, CONTRADICTION, HEAD, LEADING = 1, 2, 4, 8
VALID, SAMPLE_NUMBER = 1, 2


# ------------------------------------------------------------------ the rule, restated
def plan_py(cands, streams, B, cap):
    """cands: [(offset, number, succ, stream, blocksize, flags)], streams: [(begin, end, first_offset,
    total)] -> (slots [(cand, gap, position)] below cap, sf, ss, recs [(flags, segments, gap_frames,
    gap_samples, base)], status)"""
    n = len(cands)

    def P(i):
        return cands[i][1] if cands[i][5] & SAMPLE_NUMBER else (cands[i][1] * B) & M64

    def succ(i):
        a = cands[i][2]
        if not (0 <= a < n and a > i and cands[a][3] == cands[i][3]):
            return None
        return a if P(a) == (P(i) + cands[i][4]) & M64 else None  # the header numbers run on

    slots, sf, ss, recs = [], [0], [0], []
    nrec = nsmp = nph = bits = 0
    for s, (_, _, first, total) in enumerate(streams):
        mine = [i for i in range(n) if cands[i][3] == s]
        valid = [i for i in mine if cands[i][5] & VALID]
        heads = [i for i in valid if cands[i][0] >= first]
        flags = segments = gaps = base = T = 0
        if heads:
            h = heads[0]
            base = 0 if total else P(h)
            if total and (P(h) % B or P(h) >= total):
                flags = HEAD
            else:
                def start_ok(j):
                    return (succ(j) is not None and cands[j][0] >= first and cands[j][4] == B and P(j) >= base and
                            (P(j) - base) % B == 0 and (total == 0 or P(j) < total))
                # (candidate, position, placeholders in front of it, where they start, reached by a resync step)
                x, L = h, P(h) - base
                flags |= LEADING if L // B else 0
                chain = [(x, L, L // B, 0, False)]
                while True:
                    E = (L + cands[x][4]) & M64
                    nx = succ(x)
                    if nx is not None:
                        if total and E >= total:  # EOS: this frame ends the chain, nothing behind it is looked at
                            break
                        x, L = nx, E
                        chain.append((x, L, 0, E, False))
                        continue
                    later = [j for j in valid if j > x and start_ok(j)]
                    if not later:
                        break
                    Ln = P(later[0]) - base
                    if Ln < E or (Ln - E) % B:
                        flags |= CONTRADICTION
                        break
                    x, L = later[0], Ln
                    chain.append((x, L, (Ln - E) // B, E, True))
                segments = 1
                for x, L, count, at, stepped in chain:
                    assert not (total and L >= total)  # the head and every resumed start lie below the total
                    for t in range(min(count, max(cap - nrec, 0))):
                        slots.append((x, 1, at + t * B))
                    nrec += count
                    gaps += count
                    if nrec < cap:
                        slots.append((x, 0, L))
                    nrec += 1
                    T = (L + cands[x][4]) & M64
                    if stepped:
                        segments += 1
                        flags |= RESYNCED
        nsmp += T
        nph += gaps
        sf.append(min(nrec, U32))
        ss.append(nsmp & M64)
        recs.append((flags, segments, min(gaps, U32), (gaps * B) & M64, base))
        if gaps or flags & RESYNCED:
            bits |= 8
        if flags & (CONTRADICTION | HEAD):
            bits |= 16
    status = [bits | (2 if nrec > cap else 0), n, min(nrec, U32), min(nph, U32)]
    return slots, sf, ss, recs, status


def cand_table(cands):
    t = np.zeros(len(cands), dtype=libflac.INDEX_CAND_DTYPE)
    for k, c in enumerate(cands):
        t[k] = c
    return t


def stream_descs(streams):
    t = np.zeros(len(streams), dtype=libflac.STREAM_DESC_DTYPE)
    for k, s in enumerate(streams):
        t[k] = s
    return t


def check(cands, streams, B, cap):
    slots, sf, ss, rec, status = libflac.resync_plan_host(cand_table(cands), stream_descs(streams), B, cap)
    w_slots, w_sf, w_ss, w_rec, w_status = plan_py(cands, streams, B, cap)
    assert status.tolist() == w_status
    assert sf.tolist() == w_sf and ss.tolist() == w_ss
    assert [(int(r["flags"]), int(r["segments"]), int(r["gap_frames"]), int(r["gap_samples"]), int(r["base"]))
            for r in rec] == w_rec
    assert (rec["reserved"] == 0).all()
    assert [(int(x["cand"]), int(x["gap"]), int(x["position"])) for x in slots] == w_slots
    return slots, sf, ss, rec, status


def frames(numbers, stream=0, B=16, first=100, step=50, link=True, flags=VALID, last_bs=None):
    """A run of linked frames with these header numbers -> candidate tuples (succ relative to the run:
    the caller shifts them)."""
    out = []
    for k, num in enumerate(numbers):
        out.append([first + k * step, num, k + 1 if link and k + 1 < len(numbers) else -1, stream, B, flags])
    if last_bs is not None:
        out[-1][4] = last_bs
    return out


def join(*runs):
    """Concatenate runs of candidates, shifting each run's succ by its position; offsets ascend."""
    out, off = [], 0
    for run in runs:
        base = len(out)
        for c in run:
            c = list(c)
            if c[2] >= 0:
                c[2] += base
            c[0] += off
            out.append(tuple(c))
        off = out[-1][0] + 50 if out else 0
    return out


B = 16
STREAM = [(0, 1 << 20, 100, 0)]


def with_total(total):
    return [(0, 1 << 20, 100, total)]


# ------------------------------------------------------------------ 1. every branch by hand
def test_intact_chain():
    slots, sf, ss, rec, st = check(join(frames(range(8))), with_total(8 * B), B, 64)
    assert sf.tolist() == [0, 8] and ss.tolist() == [0, 8 * B]
    assert (slots["gap"] == 0).all() and slots["position"].tolist() == [k * B for k in range(8)]
    assert rec["segments"][0] == 1 and rec["flags"][0] == 0 and st[0] == 0 and st[3] == 0


def test_gap_of_zero():
    """The chain breaks (frame 3 has no successor) and resumes at frame 4: two segments, no placeholder."""
    slots, sf, ss, rec, st = check(join(frames(range(4)), frames(range(4, 9))), with_total(9 * B), B, 64)
    assert sf[1] == 9 and rec["flags"][0] == RESYNCED and rec["segments"][0] == 2 and rec["gap_frames"][0] == 0
    assert st[0] == 8 and st[3] == 0


def test_gap_of_n():
    slots, sf, ss, rec, st = check(join(frames(range(4)), frames(range(7, 12))), with_total(12 * B), B, 64)
    assert sf[1] == 12 and ss[1] == 12 * B
    assert slots["gap"].tolist() == [0] * 4 + [1] * 3 + [0] * 5
    assert slots["cand"][4:7].tolist() == [4, 4, 4]  # the frame behind the gap
    assert slots["position"].tolist() == [k * B for k in range(12)]
    assert rec["gap_frames"][0] == 3 and rec["gap_samples"][0] == 3 * B and st[3] == 3


def test_link_over_a_hole():
    """Every frame has a CRC-16 successor, but the numbers jump from 3 to 7: the CRC-16 of zeroed
    frames is zero, so the link across them closes.  It does not count; the hole gets placeholders."""
    slots, sf, ss, rec, st = check(join(frames([0, 1, 2, 3, 7, 8, 9])), with_total(10 * B), B, 64)
    assert slots["gap"].tolist() == [0] * 4 + [1] * 3 + [0] * 3
    assert slots["position"].tolist() == [k * B for k in range(10)]
    assert rec["flags"][0] == RESYNCED and rec["segments"][0] == 2 and st[3] == 3


def test_leading_gap():
    slots, sf, ss, rec, st = check(join(frames(range(2, 6))), with_total(6 * B), B, 64)
    assert slots["gap"].tolist() == [1, 1, 0, 0, 0, 0] and rec["flags"][0] == LEADING and rec["segments"][0] == 1
    assert st[0] == 8 and st[3] == 2


def test_rebase_without_total():
    slots, sf, ss, rec, st = check(join(frames(range(2, 6)), frames(range(8, 10))), STREAM, B, 64)
    assert rec["base"][0] == 2 * B and rec["flags"][0] == RESYNCED
    assert slots["position"].tolist() == [k * B for k in range(8)] and slots["gap"].tolist() == [0] * 4 + [1] * 2 + [0] * 2


def test_sample_numbers():
    run = frames([k * B for k in (0, 1, 2)], flags=VALID | SAMPLE_NUMBER)
    late = frames([k * B for k in (5, 6)], flags=VALID | SAMPLE_NUMBER)
    slots, sf, ss, rec, st = check(join(run, late), with_total(7 * B), B, 64)
    assert sf[1] == 7 and rec["gap_frames"][0] == 2


def test_head_cases():
    for run, total in ((frames([5 * B + 3], flags=VALID | SAMPLE_NUMBER) + frames([7 * B], flags=VALID | SAMPLE_NUMBER), 9 * B),
                       (frames(range(9, 12)), 9 * B)):  # off the grid; at or past the total
        slots, sf, ss, rec, st = check(join(run), with_total(total), B, 64)
        assert sf[1] == 0 and ss[1] == 0 and rec["flags"][0] == HEAD and rec["segments"][0] == 0 and st[0] == 16


def test_contradictions():
    back = join(frames(range(6)), frames(range(3, 12)))  # the numbers go back
    slots, sf, ss, rec, st = check(back, with_total(12 * B), B, 64)
    assert sf[1] == 6 and ss[1] == 6 * B and rec["flags"][0] == CONTRADICTION and st[0] == 16
    # off the grid of the samples before it: a short frame ends the first segment
    off = join(frames(range(4), last_bs=5), frames(range(6, 9)))
    slots, sf, ss, rec, st = check(off, with_total(12 * B), B, 64)
    assert sf[1] == 4 and ss[1] == 3 * B + 5 and rec["flags"][0] == CONTRADICTION


def test_start_past_total_and_eos():
    # the only later start lies at or past the total: not a start, the chain ends
    slots, sf, ss, rec, st = check(join(frames(range(4)), frames(range(9, 12))), with_total(9 * B), B, 64)
    assert sf[1] == 4 and rec["flags"][0] == 0
    # the total falls inside the gap: the start behind it is past the total as well
    slots, sf, ss, rec, st = check(join(frames(range(4)), frames(range(8, 12))), with_total(6 * B), B, 64)
    assert sf[1] == 4 and st[3] == 0
    # EOS inside a resumed segment: frames at or past the total are dropped, their gap stays
    slots, sf, ss, rec, st = check(join(frames(range(4)), frames(range(6, 12))), with_total(8 * B), B, 64)
    assert sf[1] == 8 and ss[1] == 8 * B and rec["gap_frames"][0] == 2 and rec["flags"][0] == RESYNCED


def test_unlinked_lone_frame():
    lone = frames([5], link=False)
    slots, sf, ss, rec, st = check(join(frames(range(4)), lone, frames(range(7, 9))), with_total(9 * B), B, 64)
    assert slots["gap"].tolist() == [0] * 4 + [1] * 3 + [0] * 2  # frame 5 is not resumed at
    # with nothing behind it the chain ends
    slots, sf, ss, rec, st = check(join(frames(range(4)), lone), with_total(9 * B), B, 64)
    assert sf[1] == 4


def test_succ_backwards_or_outside():
    c = [list(x) for x in join(frames(range(6)))]
    c[2][2] = 1  # points backwards: none
    c[4][2] = 99  # past the table: none
    other = [list(x) for x in join(frames(range(3), stream=1))]
    for x in other:
        x[0] += 1000
        if x[2] >= 0:
            x[2] += 6
    c[5][2] = 6  # into the next stream: none
    cands = [tuple(x) for x in c + other]
    streams = [(0, 1000, 100, 6 * B), (1000, 2000, 1000, 3 * B)]
    slots, sf, ss, rec, st = check(cands, streams, B, 64)
    assert sf.tolist() == [0, 5, 8]  # frame 5 has no successor of its own: not resumed at
    assert rec["segments"].tolist() == [2, 1]  # 0-2, 3-4


def test_cap_below_the_total():
    cands = join(frames(range(4)), frames(range(40, 44)))
    for cap in (0, 1, 5, 20, 43, 44, 45):
        slots, sf, ss, rec, st = check(cands, with_total(44 * B), B, cap)
        assert sf[1] == 44 and int(st[0] & 2) == (2 if cap < 44 else 0) and len(slots) == min(cap, 44)


def test_long_gap_is_no_loop():
    """2^36 placeholders from one gap: counted, never walked."""
    run = join(frames(range(4)), frames([1 << 36, (1 << 36) + 1]))
    slots, sf, ss, rec, st = check(run, STREAM, B, 8)
    gaps = (1 << 36) - 4
    assert sf[1] == U32 and st[2] == U32 and st[3] == U32 and rec["gap_frames"][0] == U32
    assert rec["gap_samples"][0] == gaps * B and ss[1] == ((1 << 36) + 2) * B
    assert slots["gap"].tolist() == [0] * 4 + [1] * 4


def test_three_streams_one_empty():
    a = join(frames(range(3)), frames(range(5, 8)))
    c = [list(x) for x in join(frames(range(1, 4), stream=2))]
    for x in c:
        x[0] += 5000
        if x[2] >= 0:
            x[2] += len(a)
    junk = [(3000, 0, -1, -1, 0, 0), (3500, 7, -1, 1, B, 0)]  # no owner; owned by the empty stream, not valid
    cands = a + junk + [tuple(x) for x in c]
    for x in cands[len(a) + 2:]:
        assert x[2] < 0 or x[2] >= len(a)
    cands = cands[:len(a)] + junk + [(x[0], x[1], x[2] + 2 if x[2] >= 0 else -1, x[3], x[4], x[5]) for x in cands[len(a) + 2:]]
    streams = [(0, 2500, 100, 8 * B), (3200, 4000, 3300, 5 * B), (5000, 9000, 5000, 4 * B)]
    slots, sf, ss, rec, st = check(cands, streams, B, 64)
    assert sf.tolist() == [0, 8, 8, 12] and ss.tolist() == [0, 8 * B, 8 * B, 12 * B]
    assert rec["flags"].tolist() == [RESYNCED, 0, LEADING] and rec["segments"].tolist() == [2, 0, 1]


def random_table(rng):
    """Streams of runs of linked frames with breaks, junk candidates, odd numbers and short frames."""
    B = int(rng.choice([1, 4, 16, 256]))
    nstreams = int(rng.integers(1, 5))
    cands, streams, off = [], [], 0
    for s in range(nstreams):
        begin = off
        first = begin + int(rng.integers(0, 120))
        nruns = int(rng.integers(0, 5))
        num = int(rng.integers(0, 4))
        frames_total = 0
        for _ in range(nruns):
            length = int(rng.integers(1, 7))
            for k in range(length):
                kind = rng.random()
                idx = len(cands)
                flags = VALID | (SAMPLE_NUMBER if rng.random() < 0.3 else 0)
                number = num * B if flags & SAMPLE_NUMBER else num
                if kind < 0.06:
                    number += int(rng.integers(1, 3))  # off by a frame, or off the grid for a sample number
                bs = B if rng.random() > 0.08 else int(rng.integers(1, B + 1))
                succ = idx + 1 if k + 1 < length else -1
                if rng.random() < 0.04:
                    succ = int(rng.integers(-1, idx + 3))
                if rng.random() < 0.08:
                    flags &= ~VALID
                cands.append((off + 10, number, succ, s, bs, flags))
                off += 60
                num += 1
                frames_total = max(frames_total, num)
                if rng.random() < 0.15:  # a junk candidate inside the frame
                    cands.append((off - 20, int(rng.integers(0, 50)), -1, s if rng.random() < 0.8 else -1, B,
                                  VALID if rng.random() < 0.3 else 0))
            jump = rng.random()
            num += 0 if jump < 0.3 else int(rng.integers(1, 6)) if jump < 0.85 else -int(rng.integers(1, 4))
            num = max(num, 0)
        total = 0 if rng.random() < 0.3 else max(1, frames_total * B - int(rng.integers(0, 3 * B + 1)))
        off += 40
        streams.append((begin, off, min(first, off), total))
    # a succ may point anywhere: clamp into int32 range only
    return cands, streams, B


def test_random_tables():
    rng = np.random.default_rng(20240521)
    seen = 0
    for _ in range(3000):
        cands, streams, bsz = random_table(rng)
        total = plan_py(cands, streams, bsz, 1 << 20)[4][2]
        cap = int(rng.choice([1 << 10, max(total - 1, 0), total // 2]))
        slots, sf, ss, rec, st = check(cands, streams, bsz, cap)
        seen |= int(np.bitwise_or.reduce(rec["flags"])) if len(rec) else 0
    assert seen == RESYNCED | CONTRADICTION | HEAD | LEADING  # the tables reach every flag


# ------------------------------------------------------------------ 2. refusals
def test_refusals_leave_the_outputs_alone():
    L = libflac.load()
    cands, streams = cand_table(join(frames(range(4)))), stream_descs(with_total(4 * B))
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def outputs():
        return (np.full(8, CANARY, np.uint8).repeat(16).view(libflac.RESYNC_SLOT_DTYPE).copy(),
                np.full(2, CANARY, np.uint32), np.full(2, CANARY, np.uint64),
                np.full(32, CANARY, np.uint8).view(libflac.RESYNC_REC_DTYPE).copy(), np.full(4, CANARY, np.uint32))

    def call(c, nc, sd, ns, bsz, out, null=None):
        slots, sf, ss, rec, st = out
        ptr = [vp(slots), vp(sf), vp(ss), vp(rec), vp(st)]
        if null is not None:
            ptr[null] = None
        return L.bnflac_resync_plan_host(c, nc, sd, ns, bsz, ptr[0], 8, ptr[1], ptr[2], ptr[3], ptr[4])

    for args in ((vp(cands), 4, vp(streams), 1, 0), (None, 4, vp(streams), 1, B), (vp(cands), 4, None, 1, B),
                 (vp(cands), 1 << 30, vp(streams), 1, B), (vp(cands), 4, vp(streams), 1 << 30, B)):
        out = outputs()
        want = [o.tobytes() for o in out]
        assert call(*args, out) < 0
        assert L.bnflac_last_error()
        assert [o.tobytes() for o in out] == want
    for null in (1, 2, 4):  # stream_frames, stream_samples, status
        out = outputs()
        want = [o.tobytes() for o in out]
        assert call(vp(cands), 4, vp(streams), 1, B, out, null) < 0
        assert [o.tobytes() for o in out] == want
    out = outputs()  # slots and resync may be null
    assert call(vp(cands), 4, vp(streams), 1, B, out, 0) == 0 and out[1].tolist() == [0, 4]
    out = outputs()
    assert call(vp(cands), 4, vp(streams), 1, B, out, 3) == 0 and out[1].tolist() == [0, 4]


def test_wrapper_refuses_like_the_call():
    with pytest.raises(RuntimeError):
        libflac.resync_plan_host(cand_table(join(frames(range(4)))), stream_descs(STREAM), 0, 8)


# ------------------------------------------------------------------ 3. the rule under the sanitizers
@pytest.mark.skipif(_cxx() is None, reason="no C++ compiler")
def test_rule_under_asan_ubsan(tmp_path):
    """A program of its own (tools/resync_sanitize.cpp), run directly: nothing is loaded into Python."""
    exe = str(tmp_path / "resync_sanitize")
    subprocess.check_call([_cxx(), "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "birdnest", "audio_amd", "csrc"),
                           os.path.join(ROOT, "tools", "resync_sanitize.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "resync_sanitize: ok" in r.stdout
