"""The rule of bnflac_window_health on the host (bnflac_window_health_host, no GPU).

Three references, all independent of the library and of its prefix sums, every comparison exact:
`marks_reference` marks every sample frame of the compact PCM that a bad record covers, by the
record's out_sample and blocksize (which the rule never reads), and counts the marks inside each
window; `rule_by_loop` is the rule of include/bnflac.h restated with Python integers and a loop
over the window's run; `missing_by_formula` is the request rule with Python integers.
tests/test_gpu_window_health.py runs the device call over tables made here (`carry_tables`).

The last part builds tools/window_health_sanitize.cpp (the same rule, csrc/bnf_health.h, in a
program of its own) with AddressSanitizer and UBSan and runs it.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from birdnest.audio_amd import libflac
from tests.test_select_ranges_host import CANARY, MIXED, ROOT, U64, _cxx, fabricate

U32 = (1 << 32) - 1
DAMAGED, SHORT, UNKNOWN, EMPTY, NO_STREAM = 1, 2, 4, 8, 16
WIN_EMPTY = 2
HEALTH_FIELDS = ("flags", "bad_frames", "crc_frames", "reserved", "bad_samples", "missing")


# ------------------------------------------------------------------ the references
def is_bad(rec):
    return int(rec["status"]) != 0 or int(rec["crc_ok"]) == 0


def rule_by_loop(sel, sel_cap, win, f):
    """The records' part of the rule for one window -> (flags, bad_frames, crc_frames, 0, bad_samples, 0)"""
    n, skip, want = int(win["nframes"]), int(win["skip"]), int(win["nsamples"])
    f = int(f)
    lo, hi = min(f, sel_cap), min(f + n, sel_cap)
    bad_frames = crc_frames = A = B = 0
    for p in range(lo, hi):
        bs = int(sel["blocksize"][p])
        A += bs
        if is_bad(sel[p]):
            bad_frames += 1
            crc_frames += int(sel["status"][p]) == 0
            B += bs
    head = skip if n > 0 and f < sel_cap and is_bad(sel[f]) else 0
    tail = (A - skip - want) if n > 0 and f + n <= sel_cap and is_bad(sel[f + n - 1]) else 0
    flags = (DAMAGED if bad_frames else 0) | (UNKNOWN if n > 0 and f + n > sel_cap else 0)
    flags |= EMPTY if int(win["flags"]) & WIN_EMPTY else 0
    return [flags, bad_frames, crc_frames, 0, (B - head - tail) & U64, 0]


def missing_by_formula(req, totals, ss):
    """The request's part of the rule -> (flag bits, missing)"""
    t, lo, want = (int(x) for x in req)
    if t >= len(totals):
        return NO_STREAM, 0
    total, T = int(totals[t]), (int(ss[t + 1]) - int(ss[t])) & U64
    hi = min(lo + want, U64)
    promised = min(hi, total) - min(lo, total)
    have = min(hi, T) - min(lo, T)
    missing = promised - have if total > T and promised > have else 0
    return (SHORT if missing else 0), missing


def ref_health(sel, sel_cap, wins, first, reqs=None, totals=None, ss=None):
    """-> ([record as a list of HEALTH_FIELDS], status [4])"""
    recs = []
    for w in range(len(wins)):
        r = rule_by_loop(sel, sel_cap, wins[w], first[w])
        if reqs is not None:
            bits, r[5] = missing_by_formula(reqs[w], totals, ss)
            r[0] |= bits
        recs.append(r)
    counts = [sum(1 for r in recs if r[0] & bit) for bit in (DAMAGED, SHORT, UNKNOWN)]
    return recs, [sum(bit for bit, c in zip((DAMAGED, SHORT, UNKNOWN), counts) if c)] + counts


def marks_reference(sel, nrecords, pcm_samples, wins):
    """bad_samples of every window by marking: independent of the window's records and of skip."""
    mark = np.zeros(pcm_samples, bool)
    for p in range(nrecords):
        if is_bad(sel[p]):
            o = int(sel["out_sample"][p])
            mark[o: o + int(sel["blocksize"][p])] = True
    return [int(mark[int(w["pcm_first"]): int(w["pcm_first"]) + int(w["nsamples"])].sum()) for w in wins]


# ------------------------------------------------------------------ the call, with canaries
def stream_descs(totals):
    sd = np.zeros(len(totals), dtype=libflac.STREAM_DESC_DTYPE)
    sd["begin"], sd["end"], sd["first_offset"] = 11, 22, 33  # never read
    sd["total_samples"] = np.array(totals, np.uint64) if len(totals) else 0
    return sd


def _ptr(a):
    """The address of a's first entry; a table without entries still gets one"""
    return (a if a.size else np.zeros(1, a.dtype)).ctypes.data_as(ctypes.c_void_p)


def call_host_health(sel, sel_cap, wins, first, reqs=None, totals=None, ss=None):
    """bnflac_window_health_host itself on outputs one entry longer than the contract says, the
    extra entry a canary -> ref_health's shape"""
    L = libflac.load()
    k = len(wins)
    sel, wins = np.ascontiguousarray(sel), np.ascontiguousarray(wins)
    first = np.ascontiguousarray(first, np.uint32)
    health = np.full((k + 1) * 32, CANARY, np.uint8)
    status = np.full(5, 0xA5A5A5A5, np.uint32)
    r = sd = s = None
    if reqs is not None:
        r, sd, s = libflac.window_requests(reqs), stream_descs(totals), np.ascontiguousarray(ss, np.uint64)
    opt = lambda a: _ptr(a) if a is not None else None
    rc = L.bnflac_window_health_host(_ptr(sel), sel_cap, _ptr(wins), _ptr(first), k, opt(r), opt(sd), opt(s),
                                     len(totals) if reqs is not None else 0, _ptr(health), _ptr(status))
    assert rc == 0, L.bnflac_last_error()
    assert (health[k * 32:] == CANARY).all() and status[4] == 0xA5A5A5A5
    h = libflac.health_array(health[: k * 32])
    return [[int(x[f]) for f in HEALTH_FIELDS] for x in h], status[:4].tolist()


def both(sel, sel_cap, wins, first, reqs=None, totals=None, ss=None):
    got = call_host_health(sel, sel_cap, wins, first, reqs, totals, ss)
    want = ref_health(sel, sel_cap, wins, first, reqs, totals, ss)
    assert got[1] == want[1]
    for w, (g, x) in enumerate(zip(got[0], want[0])):
        assert g == x, (w, g, x)
    assert len(got[0]) == len(want[0])
    return got


# ------------------------------------------------------------------ tables
def damage(sel, nrecords, rng, share=0.25):
    """Every record below nrecords good, then a share of them CRC-failed, in error, truncated or
    skipped.  A good record's crc_ok is any value but 0."""
    sel = sel.copy()
    sel["status"][:nrecords] = 0
    sel["crc_ok"][:nrecords] = rng.choice(np.array([1, 2, U32], np.uint32), nrecords)
    for p in np.flatnonzero(rng.random(nrecords) < share):
        kind = int(rng.integers(0, 4))
        sel["status"][p] = (0, 1, 2, 3)[kind]
        sel["crc_ok"][p] = 0 if kind == 0 else rng.integers(0, 2)
    return sel


def crop_requests(ss, rng, count):
    """Overlapping crops, empty ones, ids that name no stream and crops to the end of their stream"""
    n = len(ss) - 1
    reqs = []
    for _ in range(count):
        t = int(rng.integers(0, n + 2))
        T = int(ss[t + 1]) - int(ss[t]) if t < n else 5000
        kind = int(rng.integers(0, 8))
        lo = int(rng.integers(0, T + 50))
        want = (0, U64, 1)[kind] if kind < 3 else int(rng.integers(1, 9000))
        reqs.append((t, lo, want))
    return reqs


def carry_tables(sel_cap=2051, nwindows=2049, seed=5):
    """Records, windows, first positions and requests no selection wrote, at the sizes where the
    device scans carry: random statuses and blocksizes (0 and 2^32 - 1 among them), random runs with
    f up to sel_cap + 2 and n up to 40, and pinned runs at the workgroup boundaries and at sel_cap.
    -> (sel, sel_cap, wins, first, reqs, totals, ss)"""
    rng = np.random.default_rng(seed)
    sel = np.frombuffer(rng.bytes(128 * sel_cap), dtype=libflac.FRAME_INFO_DTYPE).copy()
    sel["status"] = rng.choice(np.array([0, 0, 0, 0, 1, 2, 3, 7, U32], np.uint32), sel_cap)
    sel["crc_ok"] = rng.choice(np.array([1, 1, 1, 0, U32], np.uint32), sel_cap)
    sel["blocksize"] = rng.choice(np.array([0, 1, 16, 4096, 4608, 65535, U32], np.uint32), sel_cap)
    wins = np.frombuffer(rng.bytes(32 * nwindows), dtype=libflac.WINDOW_DTYPE).copy()
    wins["nframes"] = rng.integers(0, 41, nwindows)
    wins["skip"] = rng.integers(0, 5000, nwindows)
    wins["nsamples"] = rng.integers(0, 200000, nwindows)
    first = rng.integers(0, sel_cap + 3, nwindows).astype(np.uint32)
    near = rng.random(nwindows) < 0.05  # some more runs that end around sel_cap
    first[near] = np.maximum(sel_cap - rng.integers(0, 40, int(near.sum())), 0)
    pinned = [(0, 5), (1020, 9), (2040, 12), (sel_cap - 4, 4), (sel_cap - 4, 5), (0, sel_cap), (U32, U32),
              (1023, 1), (1024, 1), (sel_cap, 0), (sel_cap, 3), (sel_cap - 1, 1)]
    for w, (f, n) in enumerate(pinned):
        if w * 7 < nwindows:
            first[w * 7], wins["nframes"][w * 7] = f, n
    n = 6
    totals = [0, 10000, 50000, 7, 1 << 40, U64]
    ss = np.array([0, 9000, 9000 + 10000, 40000, 40007, 90000, 100000], np.uint64)
    wants = (0, 1, 5000, 70000, U64)
    reqs = [(int(rng.integers(0, n + 3)), int(rng.integers(0, 60000)), wants[int(rng.integers(0, 5))]) for _ in range(nwindows)]
    reqs[3] = (U64, U64, U64)
    reqs[4] = (1 << 32, 0, 5)  # the low word alone would name stream 0
    return sel, sel_cap, wins, first, reqs, totals, ss


# ------------------------------------------------------------------ 1. the twin against the marks
@pytest.mark.parametrize("shared", [False, True])
def test_selections_with_damage(shared):
    info, sf, ss = fabricate(MIXED, seed=1, sample_base=0)
    cap = len(info)
    rng = np.random.default_rng(31 + shared)
    reqs = crop_requests(ss, rng, 300)
    reqs += [reqs[7], reqs[7], (3, 100, 3000), (3, 1100, 3000), (3, 2100, 3000)]
    if shared:
        sel, wins, first, totals, status = libflac.select_windows_shared_host(info, cap, sf, ss, reqs, cap + 3)
        nrecords, pcm_samples, sel_cap = int(totals[0]), int(totals[1]), cap + 3
    else:
        sel_cap = 4000
        sel, sel_f, sel_s, wins, status = libflac.select_windows_host(info, cap, sf, ss, reqs, sel_cap)
        nrecords, pcm_samples, first = int(sel_f[-1]), int(sel_s[-1]), sel_f
    assert status[0] == 4 and nrecords <= sel_cap, "every window's records were provided"
    sel = damage(sel, nrecords, rng)
    totals_si = [int(ss[t + 1] - ss[t]) for t in range(len(sf) - 1)]
    got, st = both(sel, sel_cap, wins, first, reqs, totals_si, ss)
    assert [g[4] for g in got] == marks_reference(sel, nrecords, pcm_samples, wins)
    assert st[0] == DAMAGED and st[1] > 20 and st[2] == st[3] == 0
    some_empty = [w for w in range(len(reqs)) if int(wins["flags"][w]) & WIN_EMPTY]
    assert some_empty and all(got[w][0] & EMPTY and got[w][1] == got[w][4] == 0 for w in some_empty)
    assert all(bool(got[w][0] & NO_STREAM) == (reqs[w][0] >= len(sf) - 1) for w in range(len(reqs)))
    whole = [w for w in range(len(reqs)) if got[w][1] == int(wins["nframes"][w]) > 0]
    assert whole and all(got[w][4] == int(wins["nsamples"][w]) for w in whole), "all frames bad: the whole window"
    assert any(0 < g[2] < g[1] for g in got) and all(g[3] == 0 for g in got)
    # without the request tables: the same records apart from NO_STREAM
    bare, st2 = both(sel, sel_cap, wins, first)
    assert st2 == st and all(b[:5] == [g[0] & ~NO_STREAM] + g[1:5] for b, g in zip(bare, got))


# ------------------------------------------------------------------ 2. missing, SHORT and NO_STREAM
def test_missing_against_the_formula():
    ss = np.array([100, 100 + 24576, 100 + 24576 + 5000, 40000, 40000, 60000], np.uint64)
    totals = [49152, 0, 10000 - 1, 700, 20000]  # cut short; unknown; a last frame passes the total; no frames; intact
    reqs = [(0, 0, 6000), (0, 22000, 6000), (0, 24576, 1), (0, 30000, 6000), (0, 47000, 6000), (0, 49152, 10), (0, 60000, 5),
            (0, 49151, U64), (0, U64, U64), (0, U64 - 3, 9), (0, 24575, 1), (0, 0, U64),
            (1, 0, 6000), (1, 4000, U64), (1, 9000, 1),
            (2, 9990, 100), (2, 0, U64), (2, 9999, 1),
            (3, 0, 100), (3, 650, 100), (3, 700, 1), (3, 0, U64),
            (4, 19000, 6000), (4, 20000, 1), (4, 0, U64),
            (5, 0, 1), (U64, 0, U64), (1 << 32, 22000, 6000)]
    k = len(reqs)
    wins = np.zeros(k, dtype=libflac.WINDOW_DTYPE)
    sel = np.zeros(1, dtype=libflac.FRAME_INFO_DTYPE)
    sel["crc_ok"] = 1
    got, st = both(sel, 1, wins, np.zeros(k, np.uint32), reqs, totals, ss)
    by = {r: (g[0], g[5]) for r, g in zip(reqs, got)}
    assert by[(0, 0, 6000)] == (0, 0) and by[(0, 22000, 6000)] == (SHORT, 3424) and by[(0, 24576, 1)] == (SHORT, 1)
    assert by[(0, 30000, 6000)] == (SHORT, 6000) and by[(0, 47000, 6000)] == (SHORT, 2152)
    assert by[(0, 49152, 10)] == (0, 0) and by[(0, 60000, 5)] == (0, 0) and by[(0, 24575, 1)] == (0, 0)
    assert by[(0, 49151, U64)] == (SHORT, 1) and by[(0, U64, U64)] == (0, 0) and by[(0, U64 - 3, 9)] == (0, 0)
    assert by[(0, 0, U64)] == (SHORT, 24576)
    assert all(by[r] == (0, 0) for r in reqs if r[0] in (1, 2, 4)), "total 0, total below T, total == T"
    assert by[(3, 0, 100)] == (SHORT, 100) and by[(3, 650, 100)] == (SHORT, 50) and by[(3, 700, 1)] == (0, 0)
    assert by[(3, 0, U64)] == (SHORT, 700)
    assert by[(5, 0, 1)] == by[(U64, 0, U64)] == by[(1 << 32, 22000, 6000)] == (NO_STREAM, 0)
    assert st == [SHORT, 0, sum(1 for g in got if g[0] & SHORT), 0] and st[2] == 9
    # nstreams == 0: every request names no stream and neither table is read (one-entry tables)
    got, st = both(sel, 1, wins[:3], np.zeros(3, np.uint32), reqs[:3], [], np.zeros(1, np.uint64))
    assert [g[0] for g in got] == [NO_STREAM] * 3 and st == [0, 0, 0, 0]


# ------------------------------------------------------------------ 3. edges
def _records(status, crc_ok, blocksize):
    sel = np.frombuffer(np.random.default_rng(9).bytes(128 * len(status)), dtype=libflac.FRAME_INFO_DTYPE).copy()
    sel["status"], sel["crc_ok"], sel["blocksize"] = status, crc_ok, blocksize
    return sel


def _windows(rows):
    """[(nframes, skip, nsamples, flags)] -> WINDOW_DTYPE; pcm_first and first_frame are never read"""
    w = np.zeros(len(rows), dtype=libflac.WINDOW_DTYPE)
    w["pcm_first"], w["first_frame"] = 0x1234567890, 77
    for k, (n, skip, want, flags) in enumerate(rows):
        w[k] = (w["pcm_first"][k], want, skip, 77, n, flags)
    return w


def test_run_edges():
    #                  0     1     2     3     4     5
    sel = _records([0, 0, 1, 0, 0, 3], [1, 0, 1, 1, 1, 0], [100, 200, 300, 400, 500, 600])
    cap = 6
    rows = [(0, 0, 0, WIN_EMPTY), (0, 9, 9, 0), (1, 10, 50, 0), (1, 10, 50, 0), (3, 20, 500, 0), (2, 30, 1000, 0),
            (1, 5, 7, 0), (2, 0, 1100, 0), (2, 0, 1100, 0), (U32, 0, 0, 0), (6, 0, 2100, 1), (7, 0, 2100, 0), (4, 0, 1, 0)]
    first = [3, 1, 0, 1, 0, 4, cap, 4, 5, U32, 0, 0, cap - 1]
    got, st = both(sel, cap, _windows(rows), first)
    assert got[0] == [EMPTY, 0, 0, 0, 0, 0] and got[1] == [0, 0, 0, 0, 0, 0], "n = 0: nothing, whatever f"
    assert got[2] == [0, 0, 0, 0, 0, 0] and got[3] == [DAMAGED, 1, 1, 0, 50, 0], "one frame: W.nsamples when it is bad"
    assert got[4] == [DAMAGED, 2, 1, 0, 500 - 80, 0], "head good, tail bad: 600 - 20 - 500 trimmed off 500"
    assert got[5] == [DAMAGED, 1, 0, 0, 600 - (1100 - 30 - 1000), 0], "f + n = sel_cap: the tail is taken"
    assert got[6] == [UNKNOWN, 0, 0, 0, 0, 0], "f = sel_cap"
    assert got[7][:5] == [DAMAGED, 1, 0, 0, 600] and got[8] == [DAMAGED | UNKNOWN, 1, 0, 0, 600, 0], "f + n = sel_cap + 1: no tail"
    assert got[9] == [UNKNOWN, 0, 0, 0, 0, 0], "f = n = 2^32 - 1 does not wrap"
    assert got[10] == [DAMAGED, 3, 1, 0, 1100, 0] and got[11] == [DAMAGED | UNKNOWN, 3, 1, 0, 1100, 0]
    assert got[12] == [DAMAGED | UNKNOWN, 1, 0, 0, 600, 0], "a bad first record below sel_cap: head = skip = 0"
    assert st == [DAMAGED | UNKNOWN, 8, 0, 5]
    # sel_cap = 0: no record is read (a one-entry allocation that is never touched would do)
    got, st = both(sel[:0], 0, _windows(rows), first)
    assert all(g[1:] == [0, 0, 0, 0, 0] for g in got) and st == [UNKNOWN, 0, 0, sum(1 for r in rows if r[0])]
    # nwindows = 0: a zero status
    assert both(sel, cap, _windows([]), []) == ([], [0, 0, 0, 0])
    # sample sums are modulo 2^64
    wide = _records([1, 1, 1], [0, 0, 0], [U32, U32, U32])
    got, _ = both(wide, 3, _windows([(3, U32, U64, 0), (2, 7, 5, 0)]), [0, 1])
    assert got[0][4] == (3 * U32 - U32 - (3 * U32 - U32 - U64)) & U64 == U64 and got[1][4] == 5


def test_tables_no_selection_wrote():
    """Random runs, statuses and blocksizes (the device test's tables): the twin is the rule."""
    sel, sel_cap, wins, first, reqs, totals, ss = carry_tables()
    got, st = both(sel, sel_cap, wins, first, reqs, totals, ss)
    assert st[0] == DAMAGED | SHORT | UNKNOWN and min(st[1:]) > 20
    assert got[6 * 7] == [UNKNOWN | (got[6 * 7][0] & (EMPTY | SHORT | NO_STREAM)), 0, 0, 0, 0, got[6 * 7][5]]
    assert got[5 * 7][1] == sum(1 for p in range(sel_cap) if is_bad(sel[p])) > 500


def test_wrapper_matches_the_raw_call():
    sel, sel_cap, wins, first, reqs, totals, ss = carry_tables(sel_cap=300, nwindows=90)
    want = call_host_health(sel, sel_cap, wins, first, reqs, totals, ss)
    health, status = libflac.window_health_host(sel, sel_cap, wins, first, reqs, stream_descs(totals), ss)
    assert [[int(x[f]) for f in HEALTH_FIELDS] for x in health] == want[0] and status.tolist() == want[1]
    again = libflac.window_health_host(sel, sel_cap, wins, first, libflac.window_requests(reqs), stream_descs(totals), ss)
    assert again[0].tobytes() == health.tobytes() and again[1].tolist() == want[1]
    bare = call_host_health(sel, sel_cap, wins, first)
    health, status = libflac.window_health_host(sel, sel_cap, wins, first)
    assert [[int(x[f]) for f in HEALTH_FIELDS] for x in health] == bare[0] and status.tolist() == bare[1]
    with pytest.raises(ValueError):
        libflac.window_health_host(sel, sel_cap, wins, first, reqs)
    assert libflac.WindowHealth.bad_samples.offset == 16 and libflac.WindowHealth.missing.offset == 24
    assert "bnflac_window_health" in libflac.BATCH_SYMBOLS and "bnflac_window_health_host" in libflac.BATCH_SYMBOLS
    assert (libflac.HEALTH_DAMAGED, libflac.HEALTH_SHORT, libflac.HEALTH_UNKNOWN, libflac.HEALTH_EMPTY,
            libflac.HEALTH_NO_STREAM) == (DAMAGED, SHORT, UNKNOWN, EMPTY, NO_STREAM)


def test_refusals():
    L = libflac.load()
    sel, sel_cap, wins, first, reqs, totals, ss = carry_tables(sel_cap=20, nwindows=8)
    r, sd = libflac.window_requests(reqs), stream_descs(totals)
    health, status = np.full(8 * 32, CANARY, np.uint8), np.full(4, 0xA5A5A5A5, np.uint32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    args = lambda **kw: [kw.get(k, v) for k, v in (("sel", vp(sel)), ("sel_cap", sel_cap), ("win", vp(wins)), ("first", vp(first)),
                                                  ("k", 8), ("r", vp(r)), ("sd", vp(sd)), ("ss", vp(ss)), ("n", len(totals)),
                                                  ("health", vp(health)), ("status", vp(status)))]
    for kw, word in (({"health": None}, b"null output"), ({"status": None}, b"null output"), ({"sel": None}, b"null table"),
                     ({"win": None}, b"null table"), ({"first": None}, b"null table"), ({"r": None}, b"all given or all null"),
                     ({"sd": None}, b"all given or all null"), ({"ss": None}, b"all given or all null"),
                     ({"r": None, "ss": None}, b"all given or all null"), ({"k": 1 << 30}, b"too many windows")):
        assert L.bnflac_window_health_host(*args(**kw)) < 0, kw
        assert word in L.bnflac_last_error(), (kw, L.bnflac_last_error())
        assert (health == CANARY).all() and (status == 0xA5A5A5A5).all(), kw
    assert L.bnflac_window_health_host(*args()) == 0 and (status != 0xA5A5A5A5).all()
    assert L.bnflac_window_health_host(*args(r=None, sd=None, ss=None)) == 0


# ------------------------------------------------------------------ 4. the rule under the sanitizers
@pytest.mark.skipif(_cxx() is None, reason="no C++ compiler")
def test_rule_under_asan_ubsan(tmp_path):
    """A program of its own (tools/window_health_sanitize.cpp), run directly: nothing is loaded
    into Python."""
    exe = str(tmp_path / "window_health_sanitize")
    subprocess.check_call([_cxx(), "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "birdnest", "audio_amd", "csrc"),
                           os.path.join(ROOT, "tools", "window_health_sanitize.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "window_health_sanitize: ok" in r.stdout
