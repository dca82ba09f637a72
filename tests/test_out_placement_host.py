"""The host side of the output-placement tests (tests/out_placement.py), without a GPU.

What tests/test_gpu_out_placement.py relies on is proved here: the frame builder is deterministic;
the exact reference (frame_pcm) agrees with the CPU oracle on every frame, under both numbering
forms, with and without STREAMINFO; every frame reaches the kernel its carrier is built for and is
one that kernel keeps; the placement plans meet their conditions on every leg; every batch the GPU
module launches stays inside its guarded allocation, also under the wrapping arithmetic the range
rule replaces; and the rule itself (csrc/bnf_out_range.h, in a program of its own) gives the
verdicts of the contract in unbounded integers."""
import math
import os
import shutil
import subprocess

import pytest

import oracle
from birdnest.audio_amd import libflac
from tests import flac_frames as F
from tests import out_placement as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_builder_is_deterministic():
    for carrier in F.CARRIERS:
        for bs, copy in ((P.blocksizes(carrier)[0], 0), (97, 3), (192, 7)):
            a, b = P.Frame(carrier, bs, copy), P.Frame(carrier, bs, copy)
            assert a.pcm == b.pcm and a.data(5) == b.data(5) and a.data(P.HEADER_BASE + 9, True) == b.data(P.HEADER_BASE + 9, True)
            assert a.data(5) == P.pick(carrier, bs, copy).data(5)
    assert [len(P.frames(c)) for c in F.CARRIERS] == [168, 168, 168, 168, 144]  # W32: the 18 blocksizes from 32 up
    assert P.plan("S16", "OUT_FLACDECODER", "mixed") == P.plan("S16", "OUT_FLACDECODER", "mixed")


def test_copies_differ_and_assignments_are_used():
    for carrier, (channels, _, _, _) in F.CARRIERS.items():
        frs = P.frames(carrier)
        assert len({f.data() for f in frs}) == len(frs)
        if channels == 2:
            assert {f.assignment for f in frs} == {1, F.LEFT_SIDE, F.RIGHT_SIDE, F.MID_SIDE}


def test_reference_agrees_with_the_oracle():
    """frame_pcm (RFC 9639 in unbounded integers) against the oracle's decode of the frame's bytes:
    every frame, the numbering form and STREAMINFO alternating over them"""
    seen = set()
    for carrier, (channels, bps, _, _) in F.CARRIERS.items():
        for i, fr in enumerate(P.frames(carrier)):
            variable, si = bool(i & 1), bool(i & 2)
            number = P.HEADER_BASE + 77 * i if variable else i
            sp = oracle.StreamParams(1, F.SI_BLOCKSIZE, F.SI_BLOCKSIZE, F.SI_RATE, channels, bps, 0) if si else None
            data = fr.data(number, variable)
            rc, res, planar = oracle.decode_frame_at(data, 0, sp)
            assert rc == 0 and res.crc_ok == 1 and res.error == -1, (carrier, fr.blocksize, fr.copy, rc)
            assert res.end_off == len(data) and res.blocksize == fr.blocksize and res.channels == channels
            assert res.bps == bps and res.number == number and res.number_type == int(variable)
            assert res.assignment == fr.record_assignment
            got = planar[: channels * fr.blocksize].reshape(channels, fr.blocksize).tolist()
            assert got == fr.pcm, (carrier, fr.blocksize, fr.copy)
            seen.add((carrier, fr.blocksize, variable, si))
    for carrier in F.CARRIERS:
        assert {b for c, b, _, _ in seen if c == carrier} == set(P.blocksizes(carrier))
        assert {(v, s) for c, _, v, s in seen if c == carrier} == {(False, False), (True, False), (False, True), (True, True)}


def test_frames_reach_their_kernel_and_are_kept():
    """no hand-back may hide a broken store path: every frame is one its carrier's kernel keeps"""
    for carrier, (channels, bps, _, kernel) in F.CARRIERS.items():
        for fr in P.frames(carrier):
            assert F.lane_kernel(fr.subs, channels, bps) == kernel, (carrier, fr.blocksize)
            samples = [[v >> s.get("wasted", 0) for v in c] for s, c in zip(fr.subs, fr.samples)]
            assert kernel != "k_decode_st" or F.st_keeps(fr.subs, bps, fr.assignment, samples)
            assert kernel != "k_decode_sw" or F.sw_keeps(fr.subs, bps, fr.assignment)
            assert F.sys_keeps(fr.subs, bps, fr.assignment, samples)
            assert 16 <= fr.blocksize <= 192 and all(s["order"] <= fr.blocksize for s in fr.subs)
            assert all(s["porder"] in (0, 1) for s in fr.subs)
        assert any(s["porder"] == 1 for fr in P.frames(carrier) for s in fr.subs)


def test_strides_are_the_library_s():
    for carrier, layout in P.LEGS:
        channels, bps = F.CARRIERS[carrier][:2]
        sp = libflac.StreamParams(1, 4096, 4096, 44100, channels, bps, 0)
        assert libflac.out_stride(P.LAYOUT_CODE[layout], sp) == P.stride_of(layout, channels, bps)
        assert getattr(libflac, layout) == P.LAYOUT_CODE[layout]
    assert {P.stride_of(l, *F.CARRIERS[c][:2]) for c, l in P.LEGS} == {2, 4, 6, 8, 9, 12}
    assert {P.stride_of(l, *F.CARRIERS[c][:2]) for c, l in P.WRAP_LEGS} == {2, 4, 6, 8, 9, 12}
    assert {F.CARRIERS[c][3] for c, _ in P.WRAP_LEGS} == {k for _, _, _, k in F.CARRIERS.values()}


@pytest.mark.parametrize("carrier,layout", P.LEGS)
def test_plan_conditions(carrier, layout):
    channels, bps, _, kernel = F.CARRIERS[carrier]
    stride, M, chunk = P.stride_of(layout, channels, bps), P.line_of(carrier, layout), P.CHUNK[kernel]
    frs = P.frames(carrier)
    for kind in P.PLANS:
        pos = P.plan(carrier, layout, kind)
        assert len(pos) == len(frs) and pos[0] >= 0
        gaps = [q - (p + f.blocksize) for p, q, f in zip(pos, pos[1:], frs)]
        assert min(gaps) >= 0
        starts = [p * stride for p in pos]
        by_bs = {}
        for f, s in zip(frs, starts):
            by_bs.setdefault(f.blocksize, set()).add(s % max(M, 64))
        if kind == "line":
            assert all(s % max(M, 64) == 0 for s in starts)
        elif kind == "al16":
            assert all(s % 16 == 0 for s in starts) and {s % 64 for s in starts} == {0, 16, 32, 48}
            assert all(len(r) > 1 for r in by_bs.values())  # the copies of a blocksize do not share a residue
        else:
            reach = set(range(0, M, math.gcd(stride, M)))
            whole = {s % M for f, s in zip(frs, starts) if f.blocksize % chunk == 0}
            ragged = {s % M for f, s in zip(frs, starts) if f.blocksize % chunk != 0}
            assert whole == reach and ragged == reach, (sorted(reach - whole), sorted(reach - ragged))
            assert min(gaps) >= 1 and min(gaps) * stride < 16
            assert all(len({s % M for f, s in zip(frs, starts) if f.blocksize == b}) > 1 for b in by_bs)
            assert (pos[-1] + frs[-1].blocksize) * stride < 200 * 1024
    g = P.guard_bytes(carrier, layout)
    assert g % 256 == 0 and g >= 4096 and g >= 2 * max(f.blocksize for f in frs) * stride


def test_blocksizes_cover_whole_ragged_and_single_chunks():
    for chunk in (16, 32):
        assert {b % chunk for b in P.B} >= {0, 1, chunk - 1}
        assert any(b < 2 * chunk for b in P.B) and any(b > 4 * chunk for b in P.B)
    assert len(P.B) == 21 and P.COPIES == 8


# ------------------------------------------------------------------ the wrap model
def _wrapped_check_passes(x, bs, stride, out_bytes):
    """(out_sample + blocksize) * stride <= out_bytes in 64-bit arithmetic"""
    return (((x + bs) % P.U64) * stride) % P.U64 <= out_bytes


@pytest.mark.parametrize("stride", [2, 4, 6, 8, 9, 12])
def test_wrap_model(stride):
    """Case A and case B: the wrapping check lets them through, and the address it then forms lies
    inside the guarded allocation (the front guard for A, the view's first bytes for B) -- while
    the contract calls both out of range."""
    bs, out_bytes, front = 129, 100000, 4608
    for d in (1, 60, bs):
        x = (-d) % P.U64
        assert _wrapped_check_passes(x, bs, stride, out_bytes)
        assert P.parent_store_range(P.case_a(d), bs, stride, out_bytes) == (-d * stride, (bs - d) * stride)
        assert -front <= -d * stride
        assert not P.in_range(P.case_a(d), bs, stride, out_bytes)
    assert not _wrapped_check_passes((-(bs + 1)) % P.U64, bs, stride, out_bytes)  # d > blocksize: the check holds
    x = P.case_b(stride)
    assert x == (P.U64 + stride - 1) // stride and x < P.U64
    r = x * stride - P.U64
    assert 0 <= r < stride and _wrapped_check_passes(x, bs, stride, out_bytes)
    assert P.parent_store_range(x, bs, stride, out_bytes) == (r, r + bs * stride)
    assert P.parent_fill_range(x, bs, stride, out_bytes) == (r, r + bs * stride)
    assert not P.in_range(x, bs, stride, out_bytes)
    assert P.parent_store_range(5, bs, stride, out_bytes) == (5 * stride, (5 + bs) * stride) and P.in_range(5, bs, stride, out_bytes)


def test_every_batch_stays_inside_its_allocation():
    """What the GPU module asserts before each launch, for every batch it builds: the contract's
    range and the wrapping arithmetic's range both lie inside the guarded allocation."""
    batches = P.all_batches()
    assert len(batches) == 5 * len(P.LEGS) + 2 * len(P.FIXED_LEGS) + 2 * len(P.WRAP_LEGS)
    for name, b in batches.items():
        assert len(b.items) <= 168 + 8 and b.front % 256 == 0 and b.front >= 4096, name
        assert b.unsafe() == [], name
        _, verdicts = b.expected()
        kind = name[0]
        if kind in "ab":
            assert set(verdicts) == {"pcm"}, name
        elif kind == "c":
            assert verdicts[-6:] == ["pcm", "out", "out", "out", "zeros", "out"] and set(verdicts[:-6]) == {"pcm"}, name
            x, limit = b.items[-6], b.out_bytes // b.stride
            assert x.p + x.frame.blocksize == limit and b.out_bytes % b.stride == b.stride - 1, name
            assert b.items[-5].p + b.items[-5].frame.blocksize == limit + 1 and b.items[-4].p == limit + 1 and b.items[-3].p == limit
        elif name.endswith("table"):
            assert verdicts[-5:] == ["out"] * 5 and set(verdicts[:-5]) == {"pcm"}, name
            olds = [P.parent_store_range(it.p, it.frame.blocksize, b.stride, b.out_bytes) for it in b.items[-5:-1]]
            assert all(o is not None for o in olds) and all(o[0] < 0 for o in olds[:3]) and 0 <= olds[3][0] < b.stride, name
            assert P.parent_fill_range(b.items[-1].p, b.items[-1].frame.blocksize, b.stride, b.out_bytes) is not None, name
        else:
            assert verdicts[-2:] == ["out"] * 2 and set(verdicts[:-2]) == {"pcm"}, name
            assert [b.header_sample(it) - b.base_sample for it in b.items[-2:]] == [-1, -b.items[-1].frame.blocksize], name
        if not b.table:  # the position the contract reads from the header is the item's
            assert all(b.header_sample(it) - b.base_sample == it.p for it in b.items), name
            assert all(0 <= it.number < 1 << 36 for it in b.items), name
        if kind == "b" and name.endswith("variable"):
            assert all(len(F.utf8(it.number)) == 7 for it in b.items), name


def test_truncation_cut_is_inside_the_subframes():
    for carrier in F.CARRIERS:
        t = P.pick(carrier, 97, 0)
        for number in (204, 172):
            data = t.data(number)
            head = 6 + len(F.utf8(number))  # 97 samples: an 8-bit blocksize field
            assert F.crc8(data[:head - 1]) == data[head - 1]
            first, last = P.truncation_cut(t, number, "first"), P.truncation_cut(t, number, "last")
            assert head < first <= last < len(data) - 2 and (first == last) == (t.channels == 1)
            # the oracle agrees: the header parses, the frame does not end inside the kept bytes
            for cut in (first, last):
                rc, res, _ = oracle.decode_frame_at(data[:cut], 0, None)
                assert rc != 0 and res.blocksize == 97, (carrier, cut, rc)


# ------------------------------------------------------------------ the rule, in a program of its own
def _cxx():
    for c in ("c++", "g++", "clang++"):
        if shutil.which(c):
            return shutil.which(c)
    return None


def _rule_rows():
    rows = []
    for stride in (2, 4, 6, 8, 9, 12):
        for out_bytes in (0, 1, stride - 1, stride, 1000 * stride, 1000 * stride + stride - 1, 1000 * stride + 1,
                          (1 << 32) + 5, (1 << 63) + 11, P.U64 - 1):
            limit = out_bytes // stride
            for bs in (1, 16, 192, 4096, 65535, (1 << 32) - 1):
                ps = {0, 1, limit, limit + 1, max(limit - 1, 0), max(limit - bs, 0), max(limit - bs + 1, 0),
                      max(limit - bs - 1, 0), 1 << 63, P.U64 - 1, P.U64 - bs, P.U64 - bs - 1, P.U64 - 1 - bs // 2,
                      P.case_b(stride), P.case_b(stride) + 1, P.case_b(stride) - 1}
                rows += [(p % P.U64, bs, stride, out_bytes) for p in sorted(ps)]
    rows += [(7, 16, 0, 1000), (0, 1, 0, 0)]  # no layout has stride 0: it holds nothing
    return rows


@pytest.mark.skipif(_cxx() is None, reason="no C++ compiler")
def test_rule_verdicts(tmp_path):
    """tools/out_range_table.cpp (csrc/bnf_out_range.h under UBSan, run directly: nothing is loaded
    into Python) against the rule in Python integers, at 0, 1, limit, limit +- 1, 2^63, 2^64 - 1,
    2^64 - blocksize, ceil(2^64 / stride), and out_bytes that no stride divides."""
    exe = str(tmp_path / "out_range_table")
    subprocess.check_call([_cxx(), "-std=c++17", "-g", "-O1", "-fsanitize=undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "birdnest", "audio_amd", "csrc"),
                           os.path.join(ROOT, "tools", "out_range_table.cpp"), "-o", exe])
    rows = _rule_rows()
    text = "".join("%d %d %d %d\n" % r for r in rows)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    lines = r.stdout.split("\n")
    assert lines[len(rows)] == "out_range_table: %d rows" % len(rows)
    verdicts = set()
    for (p, bs, stride, out_bytes), line in zip(rows, lines):
        limit = out_bytes // stride if stride else 0
        want = p <= limit and bs <= limit - p
        if stride:
            assert want == P.in_range(p, bs, stride, out_bytes)
            assert want == ((p + bs) * stride <= out_bytes)  # the contract's plain reading, nothing wrapping
        assert line == "%d %d" % (limit, want), (p, bs, stride, out_bytes, line)
        verdicts.add(want)
    assert verdicts == {True, False}
    # the rows include positions the wrapping form accepted
    assert any(_wrapped_check_passes(p, bs, s, ob) and not P.in_range(p, bs, s, ob) for p, bs, s, ob in rows if s)
