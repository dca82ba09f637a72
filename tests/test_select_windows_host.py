"""The rule of bnflac_select_windows on the host (bnflac_select_windows_host, no GPU).

The reference is `ref_windows` below: `ref_select` of tests/test_select_ranges_host.py (the rule
restated in Python frame by frame) run per request on the one-stream slice the request names, then
the per-window prefixes and their saturation, all in Python integers and independent of the
library.  Every comparison is exact.  The tables are the fabricated ones of that file.
tests/test_gpu_select_windows.py uses the same tables, requests and reference for the device call.

The last part builds tools/select_windows_sanitize.cpp (the same rule, csrc/bnf_select.h, in a
program of its own) with AddressSanitizer and UBSan and runs it.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from birdnest.audio_amd import libflac
from tests.test_select_ranges_host import (BAD_TABLES, CANARY, EMPTY, KINDS, MIXED, OVERFLOW, ROOT, U64,
                                           WINDOW_FIELDS, _cxx, assert_same, call_host, fabricate, filler, ref_select,
                                           window_of, windows_by_kind)

NO_STREAM = 4      # window flags bit 2 and status word 0 bit 2
U32 = (1 << 32) - 1


# ------------------------------------------------------------------ the reference
def ref_windows(info, cap, sf, ss, reqs, sel_cap):
    """-> ref_select's shape for the requests [(stream, first_sample, nsamples)], in their order.
    Each distinct request is evaluated once, by ref_select on its stream alone."""
    n = len(sf) - 1
    memo, bad, no_stream = {}, False, False
    for t, first, want in reqs:
        if t >= n:
            no_stream = True
        elif (t, first, want) not in memo:
            f0, f1 = int(sf[t]), int(sf[t + 1])
            one = ref_select(info, cap, [f0, f1], [int(ss[t]), int(ss[t + 1])], [(first, want)], max(f1 - f0, 0))
            memo[(t, first, want)] = one
            bad = bad or one[4][0] == BAD_TABLES
    sel = filler(sel_cap)
    k = len(reqs)
    if bad:
        wins = [(0, 0, 0, int(sf[t]), 0, EMPTY) if t < n else (0, 0, 0, 0, 0, EMPTY | NO_STREAM) for t, _, _ in reqs]
        return sel, [0] * (k + 1), [0] * (k + 1), wins, [BAD_TABLES | (NO_STREAM if no_stream else 0), 0, 0, 0]
    nf, ns, sel_f, sel_s, wins, nonempty, clipped = 0, 0, [0], [0], [], 0, 0
    for t, first, want in reqs:
        if t >= n:
            wins.append((ns, 0, 0, 0, 0, EMPTY | NO_STREAM))
        else:
            o_sel, o_f, o_s, o_w, o_st = memo[(t, first, want)]
            _, nsamples, skip, a, nfr, flags = o_w[0]
            wins.append(((ns + skip) & U64, nsamples, skip, a, nfr, flags))
            for j in range(min(nfr, max(sel_cap - nf, 0))):
                sel[nf + j] = o_sel[j]
                sel["out_sample"][nf + j] = (ns + int(o_sel["out_sample"][j])) & U64
            nf += nfr
            ns = (ns + int(o_s[1])) & U64
            nonempty += o_st[2]
            clipped += o_st[3]
        sel_f.append(min(nf, U32))
        sel_s.append(ns)
    return sel, sel_f, sel_s, wins, [(OVERFLOW if nf > sel_cap else 0) | (NO_STREAM if no_stream else 0), min(nf, U32),
                                     nonempty, clipped]


# ------------------------------------------------------------------ the call, with canaries
def call_host_windows(info, cap, sf, ss, reqs, sel_cap):
    """bnflac_select_windows_host itself on outputs one entry longer than the contract says, the
    extra entry a canary -> the outputs in ref_select's shape"""
    n, k = len(sf) - 1, len(reqs)
    L = libflac.load()
    r = libflac.window_requests(reqs)
    info = np.ascontiguousarray(info)
    sf, ss = np.ascontiguousarray(sf, np.uint32), np.ascontiguousarray(ss, np.uint64)
    sel = np.full((sel_cap + 1) * 128, CANARY, np.uint8)
    sel_f = np.full(k + 2, 0xA5A5A5A5, np.uint32)
    sel_s = np.full(k + 2, 0xA5A5A5A5A5A5A5A5, np.uint64)
    win = np.full((k + 1) * 32, CANARY, np.uint8)
    status = np.full(5, 0xA5A5A5A5, np.uint32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a.size else None
    rc = L.bnflac_select_windows_host(vp(info), cap, vp(sf), vp(ss), n, vp(r), k, vp(sel), sel_cap, vp(sel_f), vp(sel_s),
                                      vp(win), vp(status))
    assert rc == 0, L.bnflac_last_error()
    assert (sel[sel_cap * 128:] == CANARY).all(), "a record was written at sel_cap"
    assert sel_f[k + 1] == 0xA5A5A5A5 and sel_s[k + 1] == 0xA5A5A5A5A5A5A5A5 and status[4] == 0xA5A5A5A5
    assert (win[k * 32:] == CANARY).all()
    w = libflac.window_array(win[: k * 32])
    return (libflac.info_array(sel[: sel_cap * 128]), sel_f[: k + 1].tolist(), sel_s[: k + 1].tolist(),
            [tuple(int(x[f]) for f in WINDOW_FIELDS) for x in w], status[:4].tolist())


def both(info, cap, sf, ss, reqs, sel_cap):
    return assert_same(call_host_windows(info, cap, sf, ss, reqs, sel_cap), ref_windows(info, cap, sf, ss, reqs, sel_cap))


# ------------------------------------------------------------------ the request sets (shared with the GPU file)
@pytest.fixture(scope="module")
def mixed():
    return fabricate(MIXED, seed=1, sample_base=0)


def stream_shape(info, sf, ss, s):
    sl = slice(int(sf[s]), int(sf[s + 1]))
    return ([int(x) - int(ss[s]) for x in info["out_sample"][sl]], [int(x) for x in info["blocksize"][sl]],
            int(ss[s + 1]) - int(ss[s]))


def every_kind_on_every_stream(info, sf, ss):
    """len(KINDS) requests per stream, stream-major"""
    return [(s,) + tuple(window_of(kind, *stream_shape(info, sf, ss, s))) for s in range(len(sf) - 1) for kind in KINDS]


def three_on_the_long_stream(info, sf, ss):
    """Stream 3 of MIXED (40 frames): two overlapping windows and the first one again, then one
    each on streams 0 and 11; the other 13 streams are never named."""
    L, bs, T = stream_shape(info, sf, ss, 3)
    a = (3, L[10] + 1, L[14] - L[10])
    b = (3, L[12] - 1, L[20] - L[12] + 5)
    return [a, b, a, (0, 0, U64), (11, 7, 1000)]


def bad_ids(info, sf, ss):
    n = len(sf) - 1
    return [(1, 0, U64), (n, 0, 5), (U32, 1, 5), (U32 + 1, 0, U64), (1 << 63, 3, 3), (4, 2, 9)]


# ------------------------------------------------------------------ the cases
@pytest.mark.parametrize("shift", range(len(KINDS)))
def test_identity_requests_equal_select_ranges(mixed, shift):
    """Request s = (s, ranges[s]): every output byte-equal to bnflac_select_ranges_host."""
    info, sf, ss = mixed
    cap = len(info)
    ranges = windows_by_kind(info, sf, ss, shift)
    reqs = [(s,) + tuple(r) for s, r in enumerate(ranges)]
    for sel_cap in (cap + 3, 9):
        got = call_host_windows(info, cap, sf, ss, reqs, sel_cap)
        assert_same(got, call_host(info, cap, sf, ss, ranges, sel_cap))
        assert_same(got, ref_windows(info, cap, sf, ss, reqs, sel_cap))


def test_every_kind_on_every_stream_shape_and_reversed(mixed):
    info, sf, ss = mixed
    cap = len(info)
    reqs = every_kind_on_every_stream(info, sf, ss)
    assert len(reqs) == len(KINDS) * len(MIXED)
    got = both(info, cap, sf, ss, reqs, 4 * cap)
    assert got[4][0] == 0 and got[4][1] > cap  # more frames than the index holds: windows share them
    rev = both(info, cap, sf, ss, reqs[::-1], 4 * cap)
    assert rev[4] == got[4]
    assert [w[1:] for w in rev[3]] == [w[1:] for w in got[3][::-1]]  # all but pcm_first follows the request


def test_three_windows_on_one_stream(mixed):
    """Overlapping and identical windows each get their own copy of the frames they need."""
    info, sf, ss = mixed
    cap = len(info)
    reqs = three_on_the_long_stream(info, sf, ss)
    sel, sel_f, sel_s, wins, status = both(info, cap, sf, ss, reqs, cap)
    assert status[0] == 0 and status[2] == 5
    assert wins[0][2:] == wins[2][2:] and wins[0][0] != wins[2][0]
    a, b = wins[0], wins[1]
    assert a[3] < b[3] < a[3] + a[4], "the first two windows share frames"
    r0, r2 = sel[sel_f[0]:sel_f[1]].copy(), sel[sel_f[2]:sel_f[3]].copy()
    assert np.array_equal(r2["out_sample"] - r0["out_sample"], np.full(len(r0), sel_s[2] - sel_s[0], np.uint64))
    r0["out_sample"] = r2["out_sample"] = 0
    assert len(r0) == a[4] and r0.tobytes() == r2.tobytes()


def test_requests_that_name_no_stream(mixed):
    info, sf, ss = mixed
    cap, n = len(info), len(sf) - 1
    reqs = bad_ids(info, sf, ss)
    sel, sel_f, sel_s, wins, status = both(info, cap, sf, ss, reqs, cap)
    assert status[0] == NO_STREAM and status[2] == 2
    for w in wins[1:5]:
        assert w[1:] == (0, 0, 0, 0, EMPTY | NO_STREAM)
    assert sel_f[1] == sel_f[2] == sel_f[5] and sel_s[1] == sel_s[5]
    # no table entry is read for such a request: with tables of a single stream, entries [2, n] do not exist
    one = both(info, cap, sf[:2], ss[:2], [(1, 0, U64), (0, 0, U64), (n, 0, 1)], cap)
    assert one[4][0] == NO_STREAM and one[4][2] == 1


@pytest.mark.parametrize("nwindows", [0, 1, 1023, 1024, 1025])
def test_window_counts_around_the_scan_block(nwindows):
    rng = np.random.default_rng(nwindows)
    info, sf, ss = fabricate((5, 0, 3), seed=40)
    cap = len(info)
    reqs = []
    for _ in range(nwindows):
        t = int(rng.integers(0, 3))
        T = int(ss[t + 1]) - int(ss[t])
        reqs.append((t, int(rng.integers(0, T + 3)), int(rng.integers(0, T + 3))))
    got = both(info, cap, sf, ss, reqs, 5 * nwindows + 2)
    if nwindows == 0:
        assert got[4] == [0, 0, 0, 0] and got[1] == [0] and got[2] == [0] and got[3] == []
        assert got[0].tobytes() == filler(2).tobytes()
    if nwindows == 1025:
        assert got[4][0] == 0 and got[1][1025] >= got[1][1024] > 8


def test_no_streams_at_all():
    """nstreams == 0 with requests: every window names no stream, no table is read (none exists)."""
    info, sf, ss = fabricate((), seed=5)
    reqs = [(0, 0, 5), (1, 2, 3), (U64, U64, U64), (0, 0, 0), (7, 7, 7)]
    got = both(info, 0, sf, ss, reqs, 3)
    assert got[4] == [NO_STREAM, 0, 0, 0] and got[1] == [0] * 6 and got[2] == [0] * 6
    assert all(w == (0, 0, 0, 0, 0, EMPTY | NO_STREAM) for w in got[3])
    L = libflac.load()
    out = [np.zeros(32, np.uint64) for _ in range(4)]
    r = libflac.window_requests(reqs)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.bnflac_select_windows_host(None, 0, None, None, 0, vp(r), 5, None, 0, vp(out[0]), vp(out[1]), vp(out[2]),
                                        vp(out[3])) == 0  # the tables may be null pointers then


def test_sel_cap_one_short_and_zero(mixed):
    info, sf, ss = mixed
    cap = len(info)
    reqs = three_on_the_long_stream(info, sf, ss) + every_kind_on_every_stream(info, sf, ss)[:40]
    full = ref_windows(info, cap, sf, ss, reqs, 4 * cap)
    total = full[4][1]
    assert 8 < total < 4 * cap
    got = both(info, cap, sf, ss, reqs, total - 1)
    assert got[4][0] == OVERFLOW and got[4][1] == total and got[1] == full[1] and got[2] == full[2]
    assert got[0].tobytes() == full[0][: total - 1].tobytes()
    both(info, cap, sf, ss, reqs, total)
    zero = both(info, cap, sf, ss, reqs, 0)
    assert zero[4][0] == OVERFLOW and zero[1] == full[1]


def test_filler_field_by_field(mixed):
    info, sf, ss = mixed
    cap = len(info)
    reqs = three_on_the_long_stream(info, sf, ss)
    sel, sel_f, _, _, status = call_host_windows(info, cap, sf, ss, reqs, cap + 40)
    total = status[1]
    assert sel_f[-1] == total and 0 < total < cap
    fill = sel[total:]
    assert len(fill) >= 40
    for f in libflac.FRAME_INFO_DTYPE.names:
        want = 3 if f == "status" else -1 if f == "err" else 0
        assert (fill[f] == want).all(), f


def bad_slice_tables(info, sf, ss):
    """MIXED with stream 5's slice descending (sf[5] > sf[6]), stream 9's samples descending and
    stream 13's slice passing cap (sf[14] > cap while sf[13] is fine); streams 4 and 6 .. 8, 10 .. 12
    and 14, 15 lose their slices' sense with them, streams 0 .. 3 keep theirs."""
    cap = len(info)
    sf2, ss2 = sf.copy(), ss.copy()
    sf2[5], sf2[6] = sf[6], sf[5]
    ss2[10] = ss[9] - 1
    sf2[14] = cap + 7
    assert sf2[5] > sf2[6] and sf2[13] <= cap < sf2[14]
    return sf2, ss2


def test_bad_slices_count_only_when_named(mixed):
    info, sf, ss = mixed
    cap = len(info)
    sf2, ss2 = bad_slice_tables(info, sf, ss)
    good = [(3, 100, 5000), (0, 0, U64), (3, 100, 5000), (2, 0, 1), (1, 0, U64), (99, 0, 1)]
    got = both(info, cap, sf2, ss2, good, cap)
    assert got[4][0] == NO_STREAM and got[4][2] == 4
    assert_same(got, ref_windows(info, cap, sf, ss, good, cap))  # as over the tables nobody damaged
    for t in (5, 9, 13):
        reqs = good[:2] + [(t, 0, U64)] + good[2:]
        bad = both(info, cap, sf2, ss2, reqs, 24)
        assert bad[4] == [BAD_TABLES | NO_STREAM, 0, 0, 0]
        assert not any(bad[1]) and not any(bad[2]) and bad[0].tobytes() == filler(24).tobytes()
        assert bad[3][2] == (0, 0, 0, int(sf2[t]), 0, EMPTY) and bad[3][0] == (0, 0, 0, int(sf2[3]), 0, EMPTY)
        assert bad[3][-1] == (0, 0, 0, 0, 0, EMPTY | NO_STREAM)
    assert both(info, cap, sf2, ss2, [(5, 0, 1)], 4)[4] == [BAD_TABLES, 0, 0, 0]  # bit 2 is its own


def saturation_case():
    """One stream of 65,536 frames of blocksize 1, 65,537 requests for all of it."""
    rng = np.random.default_rng(77)
    nf = 65536
    info = np.frombuffer(rng.bytes(128 * nf), dtype=libflac.FRAME_INFO_DTYPE).copy()
    info["blocksize"] = 1
    info["out_sample"] = np.arange(nf, dtype=np.uint64)
    return info, np.array([0, nf], np.uint32), np.array([0, nf], np.uint64), [(0, 0, nf)] * (nf + 1)


def assert_saturated(info, got):
    sel, sel_f, sel_s, wins, status = got
    assert status == [OVERFLOW, 0xFFFFFFFF, 65537, 0]
    assert sel_f == [min(65536 * k, U32) for k in range(65538)] and sel_f[-1] == sel_f[-2] == U32
    assert sel_s == [65536 * k for k in range(65538)]
    assert sel["out_sample"].tolist() == list(range(8))
    want = info[:8].copy()
    assert sel.tobytes() == want.tobytes()  # the stream's first 8 records: its out_sample values are 0 .. 7 already
    assert wins[65536] == (65536 * 65536, 65536, 0, 0, 65536, 0)


def test_frame_prefixes_saturate():
    info, sf, ss, reqs = saturation_case()
    got = call_host_windows(info, len(info), sf, ss, reqs, 8)
    assert_saturated(info, got)
    assert_same(got, ref_windows(info, len(info), sf, ss, reqs, 8))


@pytest.mark.parametrize("seed", range(6))
def test_out_sample_values_no_index_wrote(seed):
    """Non-monotone out_sample inside the streams: the call returns, and whatever a window selects
    lies inside the slice of the stream it names and is copied from there."""
    rng = np.random.default_rng(300 + seed)
    info, sf, ss = fabricate((9, 1, 30, 0, 5, 64), seed=400 + seed)
    cap, n = len(info), len(sf) - 1
    info["out_sample"] = rng.integers(0, 1 << 63, cap, dtype=np.uint64) * 2 if seed & 1 else rng.integers(0, 20000, cap, dtype=np.uint64)
    if seed & 2:
        info["blocksize"] = rng.integers(0, 1 << 32, cap, dtype=np.uint64).astype(np.uint32)
    reqs = [(int(rng.integers(0, n)), int(rng.integers(0, 9000)), U64 if seed & 4 else int(rng.integers(0, 9000)))
            for _ in range(40)]
    sel_cap = 40 * 64
    sel, sel_f, sel_s, wins, status = call_host_windows(info, cap, sf, ss, reqs, sel_cap)
    assert status[0] == 0 and status[1] == sel_f[-1] <= sel_cap
    for (t, _, _), w, k in zip(reqs, wins, range(40)):
        assert int(sf[t]) <= w[3] <= int(sf[t + 1]) and w[3] + w[4] <= int(sf[t + 1])
        assert sel_f[k + 1] - sel_f[k] == w[4]
        got = sel[sel_f[k]:sel_f[k + 1]].copy()
        want = info[w[3]:w[3] + w[4]].copy()
        got["out_sample"] = want["out_sample"] = 0
        assert got.tobytes() == want.tobytes()


def test_wrapper_matches_the_raw_call(mixed):
    info, sf, ss = mixed
    cap = len(info)
    reqs = three_on_the_long_stream(info, sf, ss) + bad_ids(info, sf, ss)
    sel, sel_f, sel_s, win, status = libflac.select_windows_host(info, cap, sf, ss, reqs, cap)
    want = ref_windows(info, cap, sf, ss, reqs, cap)
    assert sel.tobytes() == want[0].tobytes() and sel_f.tolist() == want[1] and sel_s.tolist() == want[2]
    assert [tuple(int(x[f]) for f in WINDOW_FIELDS) for x in win] == want[3] and status.tolist() == want[4]
    table = libflac.window_requests(reqs)
    again = libflac.select_windows_host(info, cap, sf, ss, table, cap)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (sel, sel_f, sel_s, win, status)))
    assert libflac.window_requests([(2, 5)])[0].tolist() == (2, 5, U64)  # nsamples left out: to the end
    with pytest.raises(ValueError):
        libflac.window_requests([(0, -1, 3)])


def test_refusals(mixed):
    info, sf, ss = mixed
    cap, n = len(info), len(sf) - 1
    L = libflac.load()
    r = libflac.window_requests([(0, 0, 1)])
    sel = np.full(128, CANARY, np.uint8)
    sel_f, sel_s = np.full(2, 0xA5A5A5A5, np.uint32), np.full(2, 0xA5A5A5A5A5A5A5A5, np.uint64)
    win, status = np.full(32, CANARY, np.uint8), np.full(4, 0xA5A5A5A5, np.uint32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    args = lambda **kw: [kw.get(k, v) for k, v in (("info", vp(info)), ("cap", cap), ("sf", vp(sf)), ("ss", vp(ss)), ("n", n),
                                                  ("r", vp(r)), ("k", 1), ("sel", vp(sel)), ("sel_cap", 1),
                                                  ("sel_f", vp(sel_f)), ("sel_s", vp(sel_s)), ("win", vp(win)),
                                                  ("status", vp(status)))]
    for kw, word in (({"status": None}, b"null output"), ({"sel_f": None}, b"null output"), ({"sel": None}, b"null output"),
                     ({"r": None}, b"null table"), ({"win": None}, b"null table"), ({"sf": None}, b"null table"),
                     ({"info": None}, b"null info"), ({"k": 1 << 30}, b"too many windows")):
        assert L.bnflac_select_windows_host(*args(**kw)) < 0, kw
        assert word in L.bnflac_last_error(), (kw, L.bnflac_last_error())
        assert (status == 0xA5A5A5A5).all() and (sel == CANARY).all() and (win == CANARY).all()
        assert (sel_f == 0xA5A5A5A5).all() and (sel_s == 0xA5A5A5A5A5A5A5A5).all()
    assert L.bnflac_select_windows_host(*args()) == 0 and status[1] == 1


# ------------------------------------------------------------------ the rule under the sanitizers
@pytest.mark.skipif(_cxx() is None, reason="no C++ compiler")
def test_rule_under_asan_ubsan(tmp_path):
    """A program of its own (tools/select_windows_sanitize.cpp), run directly: nothing is loaded
    into Python."""
    exe = str(tmp_path / "select_windows_sanitize")
    subprocess.check_call([_cxx(), "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "birdnest", "audio_amd", "csrc"),
                           os.path.join(ROOT, "tools", "select_windows_sanitize.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "select_windows_sanitize: ok" in r.stdout
