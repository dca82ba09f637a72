"""The rule of bnflac_select_windows_shared on the host (bnflac_select_windows_shared_host, no GPU).

The reference is `ref_shared` below: `ref_select` of tests/test_select_ranges_host.py (the rule
restated in Python frame by frame) run per request on the one-stream slice the request names, then
the union of the runs by index position, and rank and pos of every member with Python integers,
independent of the library.  Every comparison is exact.  The tables are the fabricated ones of that
file.  `ref_select` is defined over tables whose frames tile their streams; over out_sample values
no index wrote, the run of each window is taken from bnflac_select_windows_host (whose own tests pin
it there) and the union, ranks and positions are still Python's.
tests/test_gpu_select_shared.py runs the device call over the same cases (`all_cases`).

The last part builds tools/select_shared_sanitize.cpp (the same rule, csrc/bnf_select.h, in a
program of its own) with AddressSanitizer and UBSan and runs it.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from birdnest.audio_amd import libflac
from tests.test_select_ranges_host import (BAD_TABLES, CANARY, EMPTY, MIXED, OVERFLOW, ROOT, U64, WINDOW_FIELDS, _cxx,
                                           fabricate, filler, ref_select)
from tests.test_select_windows_host import NO_STREAM, bad_slice_tables, call_host_windows

W, HOP = 3000, 1000  # a window and a third of it, in samples: blocksizes are 1 .. 4608


# ------------------------------------------------------------------ the reference
def runs_by_ref_select(info, cap, sf, ss, reqs):
    """-> ([(skip, nsamples, skip, a, n, flags) or None for a request without a stream], bad)"""
    n = len(sf) - 1
    memo, bad, out = {}, False, []
    for t, first, want in reqs:
        if t >= n:
            out.append(None)
            continue
        if (t, first, want) not in memo:
            f0, f1 = int(sf[t]), int(sf[t + 1])
            one = ref_select(info, cap, [f0, f1], [int(ss[t]), int(ss[t + 1])], [(first, want)], 0)
            memo[(t, first, want)] = one
            bad = bad or one[4][0] == BAD_TABLES
        out.append(memo[(t, first, want)][3][0])
    return out, bad


def runs_by_select_windows_host(info, cap, sf, ss, reqs):
    """The same from bnflac_select_windows_host, for tables ref_select is not defined over."""
    _, _, sel_s, wins, status = call_host_windows(info, cap, sf, ss, reqs, 0)
    n = len(sf) - 1
    out = [None if t >= n else ((w[0] - sel_s[k]) & U64,) + w[1:] for k, ((t, _, _), w) in enumerate(zip(reqs, wins))]
    return out, bool(status[0] & BAD_TABLES)


def ref_shared(info, cap, sf, ss, reqs, sel_cap, runs=runs_by_ref_select):
    """-> (sel records [sel_cap], windows [(WINDOW_FIELDS)], win_sel_first [k], totals [F, S], status [4])"""
    n, k = len(sf) - 1, len(reqs)
    per, bad = runs(info, cap, sf, ss, reqs)
    none = NO_STREAM if any(p is None for p in per) else 0
    sel = filler(sel_cap)
    if bad:
        wins = [(0, 0, 0, int(sf[t]), 0, EMPTY) if t < n else (0, 0, 0, 0, 0, EMPTY | NO_STREAM) for t, _, _ in reqs]
        return sel, wins, [0] * k, [0, 0], [BAD_TABLES | none, 0, 0, 0]
    members = sorted({i for p in per if p is not None for i in range(p[3], p[3] + p[4])})
    rank, pos, S = {}, {}, 0
    for r, i in enumerate(members):
        rank[i], pos[i] = r, S
        S = (S + int(info["blocksize"][i])) & U64
        if r < sel_cap:
            sel[r] = info[i]
            sel["out_sample"][r] = pos[i]
    wins, first, nonempty, clipped = [], [], 0, 0
    for p in per:
        if p is None:
            wins.append((0, 0, 0, 0, 0, EMPTY | NO_STREAM))
            first.append(0)
            continue
        skip, nsamples, _, a, nfr, flags = p
        wins.append((((pos[a] + skip) & U64) if nfr else 0, nsamples, skip, a, nfr, flags))
        first.append(rank[a] if nfr else 0)
        nonempty += 0 if flags & EMPTY else 1
        clipped += flags & 1
    F = len(members)
    return sel, wins, first, [F, S], [(OVERFLOW if F > sel_cap else 0) | none, F, nonempty, clipped]


# ------------------------------------------------------------------ the call, with canaries
def call_host_shared(info, cap, sf, ss, reqs, sel_cap):
    """bnflac_select_windows_shared_host itself on outputs one entry longer than the contract says,
    the extra entry a canary -> the outputs in ref_shared's shape"""
    n, k = len(sf) - 1, len(reqs)
    L = libflac.load()
    r = libflac.window_requests(reqs)
    info = np.ascontiguousarray(info)
    sf, ss = np.ascontiguousarray(sf, np.uint32), np.ascontiguousarray(ss, np.uint64)
    sel = np.full((sel_cap + 1) * 128, CANARY, np.uint8)
    win = np.full((k + 1) * 32, CANARY, np.uint8)
    first = np.full(k + 1, 0xA5A5A5A5, np.uint32)
    totals = np.full(3, 0xA5A5A5A5A5A5A5A5, np.uint64)
    status = np.full(5, 0xA5A5A5A5, np.uint32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a.size else None
    rc = L.bnflac_select_windows_shared_host(vp(info), cap, vp(sf), vp(ss), n, vp(r), k, vp(sel), sel_cap, vp(win), vp(first),
                                             vp(totals), vp(status))
    assert rc == 0, L.bnflac_last_error()
    assert (sel[sel_cap * 128:] == CANARY).all(), "a record was written at sel_cap"
    assert (win[k * 32:] == CANARY).all() and first[k] == 0xA5A5A5A5
    assert totals[2] == 0xA5A5A5A5A5A5A5A5 and status[4] == 0xA5A5A5A5
    w = libflac.window_array(win[: k * 32])
    return (libflac.info_array(sel[: sel_cap * 128]), [tuple(int(x[f]) for f in WINDOW_FIELDS) for x in w],
            first[:k].tolist(), totals[:2].tolist(), status[:4].tolist())


def assert_same_shared(got, want):
    g_sel, g_w, g_first, g_tot, g_st = got
    w_sel, w_w, w_first, w_tot, w_st = want
    assert g_st == [int(x) for x in w_st] and g_tot == [int(x) for x in w_tot]
    assert g_w == [tuple(int(v) for v in x) for x in w_w]
    assert g_first == [int(x) for x in w_first]
    if g_sel.tobytes() != w_sel.tobytes():
        for p in range(len(w_sel)):
            for f in libflac.FRAME_INFO_DTYPE.names:
                assert np.array_equal(g_sel[f][p], w_sel[f][p]), (p, f)
    return got


def both(info, cap, sf, ss, reqs, sel_cap, runs=runs_by_ref_select):
    return assert_same_shared(call_host_shared(info, cap, sf, ss, reqs, sel_cap), ref_shared(info, cap, sf, ss, reqs, sel_cap, runs))


# ------------------------------------------------------------------ the request sets (shared with the GPU file)
def sliding(ss, window=W, hop=HOP):
    """Windows of `window` samples every `hop` over every whole stream, stream-major; a stream
    without samples gets its one (empty) window at 0.  The last windows of a stream are clipped."""
    reqs = []
    for s in range(len(ss) - 1):
        T = int(ss[s + 1]) - int(ss[s])
        reqs += [(s, first, window) for first in range(0, max(T, 1), hop)]
    return reqs


def disjoint_ascending(info, sf, ss):
    """Two requests per stream of two or more frames, its first half of frames (from sample 1, so
    skip is not 0 where the first frame is longer) and the rest; one per stream of one frame."""
    reqs = []
    for s in range(len(sf) - 1):
        f0, f1 = int(sf[s]), int(sf[s + 1])
        T = int(ss[s + 1]) - int(ss[s])
        if f1 - f0 == 1:
            reqs.append((s, 0, T))
        elif f1 - f0 > 1:
            Lk = int(info["out_sample"][f0 + (f1 - f0) // 2]) - int(ss[s])
            if Lk > 1 and int(info["blocksize"][f0]) > 1:
                reqs.append((s, 1, Lk - 1))
            reqs.append((s, Lk, U64))
    return reqs


def garbage_tables(seed):
    rng = np.random.default_rng(500 + seed)
    info, sf, ss = fabricate((9, 1, 30, 0, 5, 64), seed=600 + seed)
    cap, n = len(info), len(sf) - 1
    info["out_sample"] = rng.integers(0, 1 << 63, cap, dtype=np.uint64) * 2 if seed & 1 else rng.integers(0, 20000, cap, dtype=np.uint64)
    if seed & 2:
        info["blocksize"] = rng.integers(0, 1 << 32, cap, dtype=np.uint64).astype(np.uint32)
    reqs = [(int(rng.integers(0, n + 1)), int(rng.integers(0, 9000)), U64 if seed & 4 else int(rng.integers(0, 9000)))
            for _ in range(40)]
    return info, sf, ss, reqs


def all_cases():
    """name -> (info, cap, sf, ss, reqs, sel_cap, runs): every case of this file, for the device call too"""
    info, sf, ss = fabricate(MIXED, seed=1, sample_base=0)
    cap = len(info)
    rng = np.random.default_rng(11)
    slide = sliding(ss)
    shuffled = [slide[i] for i in rng.permutation(len(slide))]
    F = ref_shared(info, cap, sf, ss, slide, 0)[3][0]
    sf2, ss2 = bad_slice_tables(info, sf, ss)
    good = sliding(ss[:5]) + [(99, 0, 1)]  # streams 0 .. 3 keep their slices' sense
    none, _, _ = fabricate((), seed=5)
    ref = runs_by_ref_select
    cases = {
        "sliding": (info, cap, sf, ss, slide, cap + 3, ref),
        "sliding_reversed": (info, cap, sf, ss, slide[::-1], cap + 3, ref),
        "sliding_shuffled": (info, cap, sf, ss, shuffled, cap + 3, ref),
        "sliding_duplicates": (info, cap, sf, ss, slide + slide[::7] + slide[:3], cap + 3, ref),
        "identity": (info, cap, sf, ss, disjoint_ascending(info, sf, ss), cap + 3, ref),
        "one_short": (info, cap, sf, ss, slide, F - 1, ref),
        "sel_cap_zero": (info, cap, sf, ss, slide, 0, ref),
        "exact": (info, cap, sf, ss, slide, F, ref),
        "bad_slice_unnamed": (info, cap, sf2, ss2, good, cap, ref),
        "no_windows": (info, cap, sf, ss, [], 5, ref),
        "no_streams": (none, 0, np.zeros(1, np.uint32), np.zeros(1, np.uint64),
                       [(0, 0, 5), (1, 2, 3), (U64, U64, U64), (0, 0, 0), (7, 7, 7)], 3, ref),
    }
    for t in (5, 9, 13):
        cases[f"bad_slice_{t}"] = (info, cap, sf2, ss2, good[:2] + [(t, 0, U64)] + good[2:], 24, ref)
    for seed in range(6):
        g_info, g_sf, g_ss, g_reqs = garbage_tables(seed)
        cases[f"garbage_{seed}"] = (g_info, len(g_info), g_sf, g_ss, g_reqs, len(g_info) + 2, runs_by_select_windows_host)
    return cases


CASES = all_cases()


@pytest.fixture(scope="module")
def mixed():
    return fabricate(MIXED, seed=1, sample_base=0)


# ------------------------------------------------------------------ the cases
@pytest.mark.parametrize("name", sorted(CASES))
def test_host_equals_the_reference(name):
    both(*CASES[name])


def test_sliding_windows_share_their_frames(mixed):
    """Hop = W / 3: the union is far smaller than the sum, the windows of a stream overlap in the
    shared PCM, and records, totals and each request's outputs do not depend on the request order."""
    info, sf, ss = mixed
    cap = len(info)
    reqs = CASES["sliding"][4]
    sel, wins, first, totals, status = both(info, cap, sf, ss, reqs, cap + 3)
    unshared = call_host_windows(info, cap, sf, ss, reqs, 0)[4][1]
    # every frame of every stream is in some window: the union is the whole index, each frame once
    assert status[0] == 0 and status[1] == totals[0] == cap and totals[1] == int(ss[-1]) and unshared > 2 * cap
    assert status[3] > 0 and status[2] == len(reqs) - MIXED.count(0)
    assert sel[:cap].tobytes() == info.tobytes() and sel[cap:].tobytes() == filler(3).tobytes()
    for (t, lo, _), w in zip(reqs, wins):  # sample_base 0: a window's place in the PCM is its place in the corpus
        assert w[4] == 0 or w[0] == int(ss[t]) + lo
    for order in (np.arange(len(reqs))[::-1], np.random.default_rng(3).permutation(len(reqs))):
        again = both(info, cap, sf, ss, [reqs[i] for i in order], cap + 3)
        assert again[0].tobytes() == sel.tobytes() and again[3] == totals and again[4] == status
        assert again[1] == [wins[i] for i in order] and again[2] == [first[i] for i in order]
    dup = both(info, cap, sf, ss, reqs + reqs, cap + 3)
    assert dup[0].tobytes() == sel.tobytes() and dup[3] == totals and dup[1] == wins + wins and dup[2] == first + first
    assert dup[4] == [0, cap, 2 * status[2], 2 * status[3]]


def test_disjoint_ascending_requests_equal_select_windows(mixed):
    """Nothing to share: records, window table and status byte-identical to bnflac_select_windows_host,
    win_sel_first its frame prefixes and the totals its last prefix entries."""
    info, sf, ss = mixed
    cap = len(info)
    reqs = CASES["identity"][4]
    assert len(reqs) > len(MIXED)
    for sel_cap in (cap + 3, 9):
        sel, wins, first, totals, status = both(info, cap, sf, ss, reqs, sel_cap)
        o_sel, o_f, o_s, o_wins, o_status = call_host_windows(info, cap, sf, ss, reqs, sel_cap)
        assert all(w[4] > 0 for w in wins) and any(w[2] > 0 for w in wins)
        assert sel.tobytes() == o_sel.tobytes() and wins == o_wins and status == o_status
        assert first == o_f[:-1] and totals == [o_f[-1], o_s[-1]]


def test_sel_cap_one_short_and_zero(mixed):
    info, sf, ss = mixed
    cap = len(info)
    reqs = CASES["sliding"][4]
    full = both(info, cap, sf, ss, reqs, cap)
    F = full[3][0]
    short = both(info, cap, sf, ss, reqs, F - 1)
    assert short[4] == [OVERFLOW] + full[4][1:] and short[3] == full[3]
    assert short[0].tobytes() == full[0][: F - 1].tobytes() and short[1] == full[1] and short[2] == full[2]
    zero = both(info, cap, sf, ss, reqs, 0)
    assert zero[4][0] == OVERFLOW and zero[1] == full[1] and zero[3] == full[3]


def test_bad_slices_count_only_when_named(mixed):
    info, sf, ss = mixed
    cap = len(info)
    _, _, sf2, ss2, good, _, _ = CASES["bad_slice_unnamed"]
    got = both(info, cap, sf2, ss2, good, cap)
    assert got[4][0] == NO_STREAM and got[4][1] == int(sf[4])
    assert_same_shared(got, ref_shared(info, cap, sf, ss, good, cap))  # as over the tables nobody damaged
    for t in (5, 9, 13):
        reqs = CASES[f"bad_slice_{t}"][4]
        bad = both(info, cap, sf2, ss2, reqs, 24)
        assert bad[4] == [BAD_TABLES | NO_STREAM, 0, 0, 0] and bad[3] == [0, 0] and not any(bad[2])
        assert bad[0].tobytes() == filler(24).tobytes()
        assert bad[1][2] == (0, 0, 0, int(sf2[t]), 0, EMPTY) and bad[1][0] == (0, 0, 0, int(sf2[0]), 0, EMPTY)
        assert bad[1][-1] == (0, 0, 0, 0, 0, EMPTY | NO_STREAM)
    assert both(info, cap, sf2, ss2, [(5, 0, 1)], 4)[4] == [BAD_TABLES, 0, 0, 0]  # bit 2 is its own


def test_no_windows_and_no_streams(mixed):
    info, sf, ss = mixed
    got = both(info, len(info), sf, ss, [], 5)
    assert got[4] == [0, 0, 0, 0] and got[3] == [0, 0] and got[1] == [] and got[0].tobytes() == filler(5).tobytes()
    got = both(*CASES["no_streams"])
    assert got[4] == [NO_STREAM, 0, 0, 0] and got[3] == [0, 0]
    assert all(w == (0, 0, 0, 0, 0, EMPTY | NO_STREAM) for w in got[1]) and not any(got[2])
    L = libflac.load()
    out = [np.zeros(32, np.uint64) for _ in range(4)]
    r = libflac.window_requests(CASES["no_streams"][4])
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.bnflac_select_windows_shared_host(None, 0, None, None, 0, vp(r), 5, None, 0, vp(out[0]), vp(out[1]), vp(out[2]),
                                               vp(out[3])) == 0  # the tables may be null pointers then
    assert L.bnflac_select_windows_shared_host(None, 0, None, None, 0, vp(r), 5, None, 0, vp(out[0]), None, vp(out[2]),
                                               vp(out[3])) == 0  # and so may win_sel_first always


@pytest.mark.parametrize("seed", range(6))
def test_out_sample_values_no_index_wrote(seed):
    """Non-monotone and wide out_sample values: the call returns, equals the reference, and every
    record below the total is the record of a position some window's run covers, in position order."""
    info, cap, sf, ss, reqs, sel_cap, runs = CASES[f"garbage_{seed}"]
    sel, wins, first, totals, status = both(info, cap, sf, ss, reqs, sel_cap, runs)
    members = sorted({i for w in wins for i in range(w[3], w[3] + w[4])})
    assert status[0] in (0, NO_STREAM) and status[1] == totals[0] == len(members) <= cap
    got, want = sel[: len(members)].copy(), info[members].copy()
    got["out_sample"] = want["out_sample"] = 0
    assert got.tobytes() == want.tobytes()
    for (t, _, _), w in zip(reqs, wins):
        if t < len(sf) - 1:
            assert int(sf[t]) <= w[3] <= int(sf[t + 1]) and w[3] + w[4] <= int(sf[t + 1])


def test_wrapper_matches_the_raw_call(mixed):
    info, sf, ss = mixed
    cap = len(info)
    reqs = CASES["sliding"][4][:50] + [(77, 0, 1)]
    sel, win, first, totals, status = libflac.select_windows_shared_host(info, cap, sf, ss, reqs, cap)
    want = ref_shared(info, cap, sf, ss, reqs, cap)
    assert sel.tobytes() == want[0].tobytes() and first.tolist() == want[2] and totals.tolist() == want[3]
    assert [tuple(int(x[f]) for f in WINDOW_FIELDS) for x in win] == want[1] and status.tolist() == want[4]
    again = libflac.select_windows_shared_host(info, cap, sf, ss, libflac.window_requests(reqs), cap)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (sel, win, first, totals, status)))
    assert "bnflac_select_windows_shared" in libflac.BATCH_SYMBOLS and "bnflac_select_windows_shared_host" in libflac.BATCH_SYMBOLS


def test_refusals(mixed):
    info, sf, ss = mixed
    cap, n = len(info), len(sf) - 1
    L = libflac.load()
    r = libflac.window_requests([(0, 0, 1)])
    sel = np.full(128, CANARY, np.uint8)
    win, first = np.full(32, CANARY, np.uint8), np.full(1, 0xA5A5A5A5, np.uint32)
    totals, status = np.full(2, 0xA5A5A5A5A5A5A5A5, np.uint64), np.full(4, 0xA5A5A5A5, np.uint32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    args = lambda **kw: [kw.get(k, v) for k, v in (("info", vp(info)), ("cap", cap), ("sf", vp(sf)), ("ss", vp(ss)), ("n", n),
                                                  ("r", vp(r)), ("k", 1), ("sel", vp(sel)), ("sel_cap", 1), ("win", vp(win)),
                                                  ("first", vp(first)), ("totals", vp(totals)), ("status", vp(status)))]
    for kw, word in (({"status": None}, b"null output"), ({"totals": None}, b"null output"), ({"sel": None}, b"null output"),
                     ({"r": None}, b"null table"), ({"win": None}, b"null table"), ({"sf": None}, b"null table"),
                     ({"ss": None}, b"null table"), ({"info": None}, b"null info"), ({"k": 1 << 30}, b"too many windows")):
        assert L.bnflac_select_windows_shared_host(*args(**kw)) < 0, kw
        assert word in L.bnflac_last_error(), (kw, L.bnflac_last_error())
        assert (status == 0xA5A5A5A5).all() and (sel == CANARY).all() and (win == CANARY).all()
        assert (first == 0xA5A5A5A5).all() and (totals == 0xA5A5A5A5A5A5A5A5).all()
    assert L.bnflac_select_windows_shared_host(*args()) == 0 and status.tolist() == [0, 1, 1, 0] and totals[0] == 1


# ------------------------------------------------------------------ the rule under the sanitizers
@pytest.mark.skipif(_cxx() is None, reason="no C++ compiler")
def test_rule_under_asan_ubsan(tmp_path):
    """A program of its own (tools/select_shared_sanitize.cpp), run directly: nothing is loaded
    into Python."""
    exe = str(tmp_path / "select_shared_sanitize")
    subprocess.check_call([_cxx(), "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "birdnest", "audio_amd", "csrc"),
                           os.path.join(ROOT, "tools", "select_shared_sanitize.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "select_shared_sanitize: ok" in r.stdout
