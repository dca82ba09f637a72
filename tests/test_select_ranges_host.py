"""The rule of bnflac_select_ranges on the host (bnflac_select_ranges_host, no GPU).

The reference is `ref_select` below: the rule of include/bnflac.h restated in Python frame by frame
(no binary search), independent of the library.  Every comparison is exact.  The tables are
fabricated: records of random bytes in the `info_array` dtype with only blocksize and out_sample
set, so "copied byte for byte" is tested on every field.  tests/test_gpu_select_ranges.py uses the
same tables, windows and reference for the device call.

The second part builds tools/select_ranges_sanitize.cpp (the same rule, csrc/bnf_select.h, in a
program of its own) with AddressSanitizer and UBSan and runs it.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from birdnest.audio_amd import libflac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = (1 << 64) - 1
CLIPPED, EMPTY = 1, 2
OVERFLOW, BAD_TABLES = 1, 2
CANARY = 0xA5
WINDOW_FIELDS = ("pcm_first", "nsamples", "skip", "first_frame", "nframes", "flags")


# ------------------------------------------------------------------ the reference
def filler(n):
    f = np.zeros(n, dtype=libflac.FRAME_INFO_DTYPE)
    f["status"] = 3
    f["err"] = -1
    return f


def ref_select(info, cap, sf, ss, ranges, sel_cap):
    """-> (sel records [sel_cap], sel_frames [n+1], sel_samples [n+1], windows [(WINDOW_FIELDS)], status [4]).
    Valid for tables as bnflac_index_streams writes them (frames tile each stream) and for
    unusable ones (status bit 1)."""
    n = len(sf) - 1
    sel = filler(sel_cap)
    if n and (int(sf[n]) > cap or any(sf[s] > sf[s + 1] or ss[s] > ss[s + 1] for s in range(n))):
        return sel, [0] * (n + 1), [0] * (n + 1), [(0, 0, 0, int(sf[s]), 0, EMPTY) for s in range(n)], [BAD_TABLES, 0, 0, 0]
    sel_f, sel_s, wins, nonempty, clipped = [0], [0], [], 0, 0
    for s in range(n):
        first, want = (int(x) for x in ranges[s])
        f0, f1, s0 = int(sf[s]), int(sf[s + 1]), int(ss[s])
        T = int(ss[s + 1]) - s0
        lo = min(first, T)
        hi = min(min(lo + want, U64), T)
        flags = CLIPPED if min(first + want, U64) > T else 0
        clipped += flags
        nf, ns = sel_f[-1], sel_s[-1]
        chosen = [i for i in range(f0, f1)
                  if hi > lo and int(info["out_sample"][i]) - s0 < hi and int(info["out_sample"][i]) - s0 + int(info["blocksize"][i]) > lo]
        if not chosen:
            wins.append((ns, 0, 0, f0, 0, flags | EMPTY))
            sel_f.append(nf)
            sel_s.append(ns)
            continue
        a, b = chosen[0], chosen[-1] + 1
        assert chosen == list(range(a, b))
        La = int(info["out_sample"][a]) - s0
        skip = lo - La
        assert 0 <= skip < int(info["blocksize"][a])
        wins.append((ns + skip, hi - lo, skip, a, b - a, flags))
        for i in chosen:
            p = nf + (i - a)
            if p < sel_cap:
                sel[p] = info[i]
                sel["out_sample"][p] = ns + (int(info["out_sample"][i]) - s0 - La)
        nonempty += 1
        sel_f.append(nf + b - a)
        sel_s.append(ns + int(info["out_sample"][b - 1]) + int(info["blocksize"][b - 1]) - int(info["out_sample"][a]))
    return sel, sel_f, sel_s, wins, [OVERFLOW if sel_f[-1] > sel_cap else 0, sel_f[-1], nonempty, clipped]


# ------------------------------------------------------------------ fabricated tables
def fabricate(nframes, seed, sample_base=0):
    """Streams of the given frame counts: blocksizes 1..4608 with a short last frame, records of
    random bytes -> (info, stream_frames uint32[n+1], stream_samples uint64[n+1])"""
    rng = np.random.default_rng(seed)
    total = int(sum(nframes))
    info = np.frombuffer(rng.bytes(128 * total), dtype=libflac.FRAME_INFO_DTYPE).copy()
    sf, ss, f, smp = [0], [sample_base], 0, sample_base
    for nf in nframes:
        for k in range(nf):
            bs = int(rng.integers(1, 100)) if k + 1 == nf and nf > 1 else int(rng.integers(1, 4609))
            info["blocksize"][f] = bs
            info["out_sample"][f] = smp
            smp += bs
            f += 1
        sf.append(f)
        ss.append(smp)
    return info, np.array(sf, np.uint32), np.array(ss, np.uint64)


KINDS = ("inside", "across", "lo_on_start", "hi_on_start", "last_sample", "at_T", "past_T", "zero", "to_end", "wraps",
         "whole", "clipped_by_one")


def window_of(kind, L, bs, T):
    """One window of a kind for a stream with local frame starts L, blocksizes bs and T samples."""
    nf = len(L)
    k = nf // 2
    if kind == "inside":  # strictly inside frame k where it is long enough
        return (L[k] + bs[k] // 3, max(1, bs[k] // 3)) if nf else (0, 1)
    if kind == "across":  # the last sample of frame k - 1 and the first of frame k, or wider
        return (L[k] - 1, 2) if nf > 1 else (0, max(T, 1))
    if kind == "lo_on_start":  # skip 0, the previous frame not selected
        return (L[k], 3) if nf else (0, 3)
    if kind == "hi_on_start":  # ends where frame k starts: frame k not selected
        return (max(L[k] - 5, 0), L[k] - max(L[k] - 5, 0)) if nf > 1 else (0, T)
    if kind == "last_sample":
        return (T - 1, 1) if T else (0, 1)
    if kind == "at_T":
        return (T, 4)
    if kind == "past_T":
        return (T + 9, 4)
    if kind == "zero":
        return (min(3, T), 0)
    if kind == "to_end":
        return (T // 2, U64)
    if kind == "wraps":  # first_sample + nsamples passes 2^64
        return (5, U64 - 2)
    if kind == "whole":
        return (0, T)
    if kind == "clipped_by_one":
        return (T - 1, 2) if T else (0, 1)
    raise KeyError(kind)


def windows_by_kind(info, sf, ss, shift=0):
    """Stream s gets the window of kind (s + shift) mod len(KINDS)."""
    out = []
    for s in range(len(sf) - 1):
        sl = slice(int(sf[s]), int(sf[s + 1]))
        L = [int(x) - int(ss[s]) for x in info["out_sample"][sl]]
        out.append(window_of(KINDS[(s + shift) % len(KINDS)], L, [int(x) for x in info["blocksize"][sl]],
                             int(ss[s + 1]) - int(ss[s])))
    return out


# ------------------------------------------------------------------ the call, with canaries
def call_host(info, cap, sf, ss, ranges, sel_cap):
    """bnflac_select_ranges_host itself on outputs one entry longer than the contract says, the
    extra entry a canary -> the outputs in ref_select's shape"""
    n = len(sf) - 1
    L = libflac.load()
    r = libflac.sample_ranges(ranges)
    info = np.ascontiguousarray(info)
    sf, ss = np.ascontiguousarray(sf, np.uint32), np.ascontiguousarray(ss, np.uint64)
    sel = np.full((sel_cap + 1) * 128, CANARY, np.uint8)
    sel_f = np.full(n + 2, 0xA5A5A5A5, np.uint32)
    sel_s = np.full(n + 2, 0xA5A5A5A5A5A5A5A5, np.uint64)
    win = np.full((n + 1) * 32, CANARY, np.uint8)
    status = np.full(5, 0xA5A5A5A5, np.uint32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a.size else None
    rc = L.bnflac_select_ranges_host(vp(info), cap, vp(sf), vp(ss), n, vp(r), vp(sel), sel_cap, vp(sel_f), vp(sel_s), vp(win),
                                     vp(status))
    assert rc == 0, L.bnflac_last_error()
    assert (sel[sel_cap * 128:] == CANARY).all(), "a record was written at sel_cap"
    assert sel_f[n + 1] == 0xA5A5A5A5 and sel_s[n + 1] == 0xA5A5A5A5A5A5A5A5 and status[4] == 0xA5A5A5A5
    assert (win[n * 32:] == CANARY).all()
    w = libflac.window_array(win[: n * 32])
    return (libflac.info_array(sel[: sel_cap * 128]), sel_f[: n + 1].tolist(), sel_s[: n + 1].tolist(),
            [tuple(int(x[f]) for f in WINDOW_FIELDS) for x in w], status[:4].tolist())


def assert_same(got, want):
    g_sel, g_f, g_s, g_w, g_st = got
    w_sel, w_f, w_s, w_w, w_st = want
    assert g_st == list(w_st)
    assert g_f == [int(x) for x in w_f] and g_s == [int(x) for x in w_s]
    assert g_w == [tuple(int(v) for v in x) for x in w_w]
    if g_sel.tobytes() != w_sel.tobytes():
        for p in range(len(w_sel)):
            for f in libflac.FRAME_INFO_DTYPE.names:
                assert np.array_equal(g_sel[f][p], w_sel[f][p]), (p, f)
    return got


MIXED = (12, 1, 0, 40, 7, 3, 1, 25, 9, 2, 2, 30, 5, 1, 0, 17)


@pytest.fixture(scope="module")
def mixed():
    return fabricate(MIXED, seed=1, sample_base=0)


# ------------------------------------------------------------------ the cases
@pytest.mark.parametrize("shift", range(len(KINDS)))
def test_every_kind_of_window_on_every_stream_shape(mixed, shift):
    """Streams of 0, 1 and many frames; each pass gives every stream another kind of window."""
    info, sf, ss = mixed
    cap = len(info)
    ranges = windows_by_kind(info, sf, ss, shift)
    got = assert_same(call_host(info, cap, sf, ss, ranges, cap + 3), ref_select(info, cap, sf, ss, ranges, cap + 3))
    assert got[4][0] == 0


def test_the_kinds_are_what_they_say(mixed):
    """The windows above really hit the edges they are named after (stream 3: 40 frames)."""
    info, sf, ss = mixed
    cap, s = len(info), 3
    f0, k = int(sf[s]), 20
    L = [int(x) - int(ss[s]) for x in info["out_sample"][f0:int(sf[s + 1])]]
    T = int(ss[s + 1]) - int(ss[s])
    for kind, check in (("lo_on_start", lambda w: w[2] == 0 and w[3] == f0 + k),
                        ("hi_on_start", lambda w: w[3] + w[4] == f0 + k),
                        ("across", lambda w: w[3] == f0 + k - 1 and w[4] == 2),
                        ("last_sample", lambda w: w[3] == int(sf[s + 1]) - 1 and w[4] == 1 and w[1] == 1 and not w[5]),
                        ("at_T", lambda w: w[5] == CLIPPED | EMPTY), ("past_T", lambda w: w[5] == CLIPPED | EMPTY),
                        ("zero", lambda w: w[5] == EMPTY), ("to_end", lambda w: w[5] == CLIPPED and w[1] == T - T // 2),
                        ("wraps", lambda w: w[5] == CLIPPED and w[1] == T - 5),
                        ("whole", lambda w: w[5] == 0 and w[4] == 40 and w[1] == T),
                        ("clipped_by_one", lambda w: w[5] == CLIPPED and w[1] == 1)):
        ranges = [(0, 0)] * (len(sf) - 1)
        ranges[s] = window_of(kind, L, [int(x) for x in info["blocksize"][f0:int(sf[s + 1])]], T)
        got = assert_same(call_host(info, cap, sf, ss, ranges, cap), ref_select(info, cap, sf, ss, ranges, cap))
        assert check(got[3][s]), (kind, got[3][s])


def test_sample_base_and_inside_one_frame():
    """Prefixes that do not start at 0, and a window strictly inside one long frame."""
    info, sf, ss = fabricate((3, 5), seed=2, sample_base=1000)
    info["blocksize"][4] = 4096
    for i in range(5, 8):
        info["out_sample"][i] = info["out_sample"][i - 1] + info["blocksize"][i - 1]
    ss[2] = info["out_sample"][7] + info["blocksize"][7]
    L4 = int(info["out_sample"][4]) - int(ss[1])
    ranges = [(0, 1), (L4 + 100, 50)]
    got = assert_same(call_host(info, 8, sf, ss, ranges, 8), ref_select(info, 8, sf, ss, ranges, 8))
    assert got[3][1][2:5] == (100, 4, 1)


@pytest.mark.parametrize("nstreams", [0, 1, 1025])
def test_stream_counts_around_the_scan_block(nstreams):
    rng = np.random.default_rng(nstreams)
    info, sf, ss = fabricate([int(x) for x in rng.integers(0, 6, nstreams)], seed=3 + nstreams)
    cap = len(info)
    ranges = []
    for s in range(nstreams):
        T = int(ss[s + 1]) - int(ss[s])
        ranges.append((int(rng.integers(0, T + 3)), int(rng.integers(0, T + 3))))
    got = assert_same(call_host(info, cap, sf, ss, ranges, cap + 2), ref_select(info, cap, sf, ss, ranges, cap + 2))
    if nstreams == 0:
        assert got[4] == [0, 0, 0, 0] and got[1] == [0] and got[2] == [0]
        assert got[0].tobytes() == filler(2).tobytes()


def test_sel_cap_one_short(mixed):
    """Bit 0, the true prefixes, the records below sel_cap, nothing at sel_cap (call_host's canary)."""
    info, sf, ss = mixed
    cap = len(info)
    ranges = windows_by_kind(info, sf, ss, 10)
    full = ref_select(info, cap, sf, ss, ranges, cap)
    total = full[4][1]
    assert total > 8
    got = assert_same(call_host(info, cap, sf, ss, ranges, total - 1), ref_select(info, cap, sf, ss, ranges, total - 1))
    assert got[4][0] == OVERFLOW and got[4][1] == total and got[1] == [int(x) for x in full[1]]
    assert got[0].tobytes() == full[0][: total - 1].tobytes()
    assert_same(call_host(info, cap, sf, ss, ranges, 0), ref_select(info, cap, sf, ss, ranges, 0))


def test_filler_field_by_field(mixed):
    info, sf, ss = mixed
    cap = len(info)
    ranges = windows_by_kind(info, sf, ss, 0)
    sel, sel_f, _, _, status = call_host(info, cap, sf, ss, ranges, cap + 40)
    total = status[1]
    assert sel_f[-1] == total and total < cap
    fill = sel[total:]
    assert len(fill) >= 40
    for f in libflac.FRAME_INFO_DTYPE.names:
        want = 3 if f == "status" else -1 if f == "err" else 0
        assert (fill[f] == want).all(), f


def test_unusable_tables(mixed):
    info, sf, ss = mixed
    cap, n = len(info), len(sf) - 1
    ranges = [(0, U64)] * n

    def check(cap, sf, ss):
        got = assert_same(call_host(info, cap, sf, ss, ranges, 24), ref_select(info, cap, sf, ss, ranges, 24))
        assert got[4] == [BAD_TABLES, 0, 0, 0]
        assert not any(got[1]) and not any(got[2])
        assert all(w[1] == 0 and w[4] == 0 and w[5] == EMPTY for w in got[3])
        assert got[0].tobytes() == filler(24).tobytes()

    check(cap - 1, sf, ss)  # d_stream_frames[nstreams] > cap: the index overflowed
    bad = sf.copy()
    bad[5], bad[6] = sf[6], sf[5]
    assert bad[5] > bad[6]
    check(cap, bad, ss)  # the frame prefixes descend
    bad = ss.copy()
    bad[9] = ss[8] - 1
    check(cap, sf, bad)  # the sample prefixes descend
    bad = sf.copy()
    bad[4] = cap + 7  # one entry past cap although the last one is not
    check(cap, bad, ss)


@pytest.mark.parametrize("seed", range(6))
def test_out_sample_values_no_index_wrote(seed):
    """Non-monotone out_sample inside the streams: the call returns, and whatever it selects lies
    inside the stream's frames and below sel_cap."""
    rng = np.random.default_rng(100 + seed)
    info, sf, ss = fabricate((9, 1, 30, 0, 5, 64), seed=200 + seed)
    cap = len(info)
    info["out_sample"] = rng.integers(0, 1 << 63, cap, dtype=np.uint64) * 2 if seed & 1 else rng.integers(0, 20000, cap, dtype=np.uint64)
    if seed & 2:
        info["blocksize"] = rng.integers(0, 1 << 32, cap, dtype=np.uint64).astype(np.uint32)
    ranges = [(int(rng.integers(0, 9000)), U64 if seed & 4 else int(rng.integers(0, 9000))) for _ in range(len(sf) - 1)]
    sel, sel_f, sel_s, wins, status = call_host(info, cap, sf, ss, ranges, cap)
    assert status[0] == 0 and status[1] == sel_f[-1] <= cap
    for s, w in enumerate(wins):
        assert int(sf[s]) <= w[3] <= int(sf[s + 1]) and w[3] + w[4] <= int(sf[s + 1])
        assert sel_f[s + 1] - sel_f[s] == w[4]
        got = sel[sel_f[s]:sel_f[s + 1]].copy()
        want = info[w[3]:w[3] + w[4]].copy()
        got["out_sample"] = want["out_sample"] = 0
        assert got.tobytes() == want.tobytes()


def test_wrapper_matches_the_raw_call(mixed):
    info, sf, ss = mixed
    cap = len(info)
    ranges = windows_by_kind(info, sf, ss, 4)
    sel, sel_f, sel_s, win, status = libflac.select_ranges_host(info, cap, sf, ss, ranges, cap)
    want = ref_select(info, cap, sf, ss, ranges, cap)
    assert sel.tobytes() == want[0].tobytes() and sel_f.tolist() == want[1] and sel_s.tolist() == want[2]
    assert [tuple(int(x[f]) for f in WINDOW_FIELDS) for x in win] == want[3] and status.tolist() == want[4]


# ------------------------------------------------------------------ the rule under the sanitizers
def _cxx():
    for c in ("c++", "g++", "clang++"):
        if shutil.which(c):
            return shutil.which(c)
    return None


@pytest.mark.skipif(_cxx() is None, reason="no C++ compiler")
def test_rule_under_asan_ubsan(tmp_path):
    """A program of its own (tools/select_ranges_sanitize.cpp), run directly: nothing is loaded
    into Python."""
    exe = str(tmp_path / "select_ranges_sanitize")
    subprocess.check_call([_cxx(), "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "birdnest", "audio_amd", "csrc"),
                           os.path.join(ROOT, "tools", "select_ranges_sanitize.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "select_ranges_sanitize: ok" in r.stdout
