"""The rule of bnflac_gather_ranges_f32 on the host (bnflac_gather_ranges_f32_host, no GPU).

The reference is `ref_f32` below: the formulas of include/bnflac.h in numpy, sample by sample out
of the PCM bytes, independent of the library (no tiles, no blocks).  Every comparison of floats is
on the bit pattern.  tests/test_gpu_gather_f32.py uses the same layouts, reference and raw call
for the device.

The last part builds tools/gather_f32_sanitize.cpp (the same rule, csrc/bnf_pcm_f32.h, in a
program of its own) with AddressSanitizer and UBSan and runs it.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from birdnest.audio_amd import libflac
from tests.test_select_ranges_host import ROOT, U64, _cxx

MONO = 1
CANARY = 0x7FC5A5A5  # a NaN no conversion yields
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31

# (layout, channels, bps): every accepted layout, units of 2, 3 and 4 bytes, 1 to 8 channels
LAYOUTS = [("OUT_FLACDECODER", 1, 16), ("OUT_FLACDECODER", 2, 16), ("OUT_FILEREADER", 1, 24), ("OUT_FILEREADER", 2, 24),
           ("OUT_FILEREADER", 3, 16), ("OUT_FILEREADER", 8, 24), ("OUT_INTERLEAVED32", 1, 8), ("OUT_INTERLEAVED32", 2, 16),
           ("OUT_INTERLEAVED32", 3, 20), ("OUT_INTERLEAVED32", 8, 32)]
LAYOUT_IDS = ["%s-%dch-%d" % (f[4:], c, b) for f, c, b in LAYOUTS]
# 32-bit inputs whose conversion tells round-to-nearest-even from truncation, and the float they give before scaling
CHOSEN_32 = [(2 ** 24 + 1, 2 ** 24), (2 ** 24 + 3, 2 ** 24 + 4), (-(2 ** 24 + 1), -2 ** 24), (2 ** 25 + 2, 2 ** 25),
             (2 ** 25 + 6, 2 ** 25 + 8), (INT32_MAX, 2 ** 31), (INT32_MIN, -2 ** 31)]


def params(channels, bps):
    return libflac.StreamParams(1, 4096, 4096, 44100, channels, bps, 0)


def layout(name, channels, bps):
    """-> (fmt, sp, stride, unit), the stride worked out here and checked against the library's"""
    fmt, sp = getattr(libflac, name), params(channels, bps)
    unit = 4 if name == "OUT_INTERLEAVED32" else 2 if name == "OUT_FLACDECODER" else bps // 8
    assert libflac.out_stride(fmt, sp) == unit * channels and libflac.md5_layout(fmt, sp) == (bps + 7) // 8
    return fmt, sp, unit * channels, unit


def samples_of(pcm, stride, unit):
    """The whole sample frames of the PCM bytes as int64[frames, channels]."""
    pcm = np.asarray(pcm, np.uint8)
    n = len(pcm) // stride
    b = pcm[: n * stride].reshape(n, stride // unit, unit).astype(np.int64)
    v = sum(b[:, :, k] << (8 * k) for k in range(unit))
    return v - ((v >> (8 * unit - 1)) << (8 * unit))  # sign-extended from 8 * unit bits


def ref_f32(pcm, fmt, sp, windows, R, pitch, flags):
    """-> (the bits of every float from d_out on, uint32[(n * planes - 1) * pitch + R] with CANARY where
    nothing is written; status [4]).  pcm: uint8[pcm_bytes]."""
    unit = 4 if fmt == libflac.OUT_INTERLEAVED32 else 2 if fmt == libflac.OUT_FLACDECODER else sp.bps // 8
    stride = unit * sp.channels
    smp = samples_of(pcm, stride, unit)
    limit = len(smp)
    planes = 1 if flags & MONO else sp.channels
    n = len(windows)
    want = np.full(max((n * planes - 1) * pitch + R, 0), CANARY, np.uint32)
    nbad = ncut = 0
    for s, w in enumerate(windows):
        first, ns = int(w["pcm_first"]), int(w["nsamples"])
        bad = ns != 0 and (first > limit or ns > limit - first)
        nbad += bad
        ncut += (not bad) and ns > R
        ncopy = 0 if bad else min(ns, R)
        x = smp[first: first + ncopy] if ncopy else smp[:0]
        if flags & MONO:
            f = (x.sum(axis=1).astype(np.float64) * 2.0 ** -(sp.bps - 1) / sp.channels).astype(np.float32)[None, :]
        else:
            f = x.T.astype(np.int32).astype(np.float32) * np.float32(2.0 ** -(sp.bps - 1))
        for c in range(planes):
            at = (s * planes + c) * pitch
            want[at: at + ncopy] = np.ascontiguousarray(f[c]).view(np.uint32)
            want[at + ncopy: at + R] = 0
    return want, [1 if nbad else 0, nbad, ncut, 0]


def window_table(pairs):
    win = np.zeros(len(pairs), dtype=libflac.WINDOW_DTYPE)
    for k, (first, n) in enumerate(pairs):
        win[k] = (first, n, 0, 0, 0, 0)
    return win


def padded(pcm):
    """The allocation the contract asks for: round_up(pcm_bytes, 16) bytes, the tail not zero."""
    buf = np.full((len(pcm) + 15) // 16 * 16, 0xEE, np.uint8)
    buf[: len(pcm)] = pcm
    return buf


def call_host(pcm, fmt, sp, win, R, pitch, flags, tail=7):
    """bnflac_gather_ranges_f32_host itself on an output of the contract's size plus `tail` canaries
    -> (rc, the output's bits with the tail checked and cut off, status[4] with its canary checked)"""
    n = len(win)
    planes = 1 if flags & MONO else max(sp.channels, 1)
    size = max((n * planes - 1) * pitch + R, 0)
    buf, win = padded(pcm), np.ascontiguousarray(win)
    out = np.full(size + tail, CANARY, np.uint32)
    status = np.full(5, 0xA5A5A5A5, np.uint32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a.size else None
    rc = libflac.load().bnflac_gather_ranges_f32_host(vp(buf), len(pcm), fmt, ctypes.byref(sp), vp(win), n, R, pitch, flags,
                                                      vp(out), vp(status))
    assert (out[size:] == CANARY).all() and status[4] == 0xA5A5A5A5
    return rc, out[:size], status[:4].tolist()


def assert_bits(got, want, what=""):
    if not np.array_equal(got, want):
        bad = int(np.flatnonzero(got != want)[0])
        raise AssertionError("%s: float %d is %08x, want %08x" % (what, bad, got[bad], want[bad]))


def random_pcm(rng, nbytes, unit, bps):
    """Random bytes; unit 4: random int32 over the full range with the chosen values mixed in."""
    pcm = rng.integers(0, 256, nbytes, dtype=np.uint8)
    if unit == 4:
        v = pcm[: nbytes // 4 * 4].view("<i4")
        picks = np.array([x for x, _ in CHOSEN_32], np.int64).astype(np.int32)
        v[:: 5] = picks[np.arange(len(v[:: 5])) % len(picks)]
    return pcm


# ------------------------------------------------------------------ the host twin against ref_f32
@pytest.mark.parametrize("name,channels,bps", LAYOUTS, ids=LAYOUT_IDS)
def test_host_twin_against_the_formulas(name, channels, bps):
    fmt, sp, stride, unit = layout(name, channels, bps)
    rng = np.random.default_rng(channels * 100 + bps)
    R, nsmp = 50, 140
    pcm = random_pcm(rng, nsmp * stride + 1, unit, bps)  # a partial sample frame at the end
    pairs = [(first, n) for n in (0, 1, 3, 4, 5, R - 1, R, R + 3) for first in (0, 1, 2, 3, 7)]
    pairs += [(nsmp - R, R), (nsmp - 1, 1), (nsmp, 0)]
    win = window_table(pairs)
    for flags in (0, MONO):
        for pitch in (R, R + 5):
            rc, got, st = call_host(pcm, fmt, sp, win, R, pitch, flags)
            want, want_st = ref_f32(pcm, fmt, sp, win, R, pitch, flags)
            assert rc == 0, libflac.load().bnflac_last_error()
            assert_bits(got, want, "%s flags %d pitch %d" % (name, flags, pitch))
            assert st == want_st == [0, 0, 5, 0]


@pytest.mark.parametrize("name,channels,bps", [LAYOUTS[1], LAYOUTS[5], LAYOUTS[8]], ids=[LAYOUT_IDS[k] for k in (1, 5, 8)])
def test_host_twin_across_tiles(name, channels, bps):
    """Rows longer than two of the rule's tiles (at most 2,048 sample frames each)."""
    fmt, sp, stride, unit = layout(name, channels, bps)
    rng = np.random.default_rng(7)
    R = 2 * 2048 + 3
    pcm = random_pcm(rng, (R + 20) * stride, unit, bps)
    win = window_table([(1, R), (3, R + 9), (5, 2048), (0, 2049)])
    for flags in (0, MONO):
        rc, got, st = call_host(pcm, fmt, sp, win, R, R + 5, flags)
        want, want_st = ref_f32(pcm, fmt, sp, win, R, R + 5, flags)
        assert rc == 0 and st == want_st == [0, 0, 1, 0]
        assert_bits(got, want, name)


# ------------------------------------------------------------------ chosen values
def _one_window(values, name, channels, bps, flags=0):
    """The floats of one window over the given sample frames (int, [frames, channels])."""
    fmt, sp, stride, unit = layout(name, channels, bps)
    v = np.asarray(values, np.int64).reshape(-1, channels)
    pcm = np.zeros(len(v) * stride, np.uint8)
    for k in range(unit):
        pcm.reshape(len(v), channels, unit)[:, :, k] = (v >> (8 * k)) & 0xFF
    rc, got, st = call_host(pcm, fmt, sp, window_table([(0, len(v))]), len(v), len(v), flags)
    assert rc == 0 and st == [0, 0, 0, 0]
    return got.view(np.float32)


def test_int_to_float_rounds_to_nearest_even():
    got = _one_window([x for x, _ in CHOSEN_32], "OUT_INTERLEAVED32", 1, 32)
    want = np.array([float(y) * 2.0 ** -31 for _, y in CHOSEN_32], np.float32)  # exact: a power of two times a float
    assert [float(y) for _, y in CHOSEN_32] == [float(np.float32(y)) for _, y in CHOSEN_32]
    assert_bits(got.view(np.uint32), want.view(np.uint32))
    assert got[5] == 1.0 and got[6] == -1.0
    truncated = [2 ** 24, 2 ** 24 + 2, -2 ** 24, 2 ** 25, 2 ** 25 + 4]  # what a conversion towards zero gives
    assert sum(t != y for t, (_, y) in zip(truncated, CHOSEN_32)) == 2, "the values tell rounding from truncation"


def test_24_bit_packed_extremes():
    fmt, sp, stride, unit = layout("OUT_FILEREADER", 1, 24)
    pcm = np.array([0x00, 0x00, 0x80, 0xFF, 0xFF, 0x7F], np.uint8)
    rc, got, st = call_host(pcm, fmt, sp, window_table([(0, 2)]), 2, 2, 0)
    assert rc == 0 and got.view(np.float32).tolist() == [-1.0, 1.0 - 2.0 ** -23]


def test_mono_chosen_values():
    assert _one_window([[INT32_MAX] * 8], "OUT_INTERLEAVED32", 8, 32, MONO).tolist() == [1.0]
    rng = np.random.default_rng(3)
    v = rng.integers(INT32_MIN, INT32_MAX + 1, 500)
    for name, bps in (("OUT_INTERLEAVED32", 32), ("OUT_INTERLEAVED32", 12)):
        a = _one_window(v, name, 1, bps, 0)
        b = _one_window(v, name, 1, bps, MONO)
        assert_bits(a.view(np.uint32), b.view(np.uint32), "mono of one channel")


def test_mono_is_the_formula_not_a_sum_of_floats():
    rng = np.random.default_rng(11)
    v = rng.integers(INT32_MIN, INT32_MAX + 1, (4000, 3))
    got = _one_window(v, "OUT_INTERLEAVED32", 3, 32, MONO)
    formula = (v.sum(axis=1).astype(np.float64) * 2.0 ** -31 / 3).astype(np.float32)
    assert_bits(got.view(np.uint32), formula.view(np.uint32), "mono, 3 channels, 32 bits")
    k = np.float32(2.0 ** -31)
    f = v.astype(np.int32).astype(np.float32) * k
    shortcut = (f[:, 0] + f[:, 1] + f[:, 2]) / np.float32(3)
    differing = int((shortcut.view(np.uint32) != formula.view(np.uint32)).sum())
    assert differing > 400, "the data does not tell the formula from a sum of floats (%d of 4000 differ)" % differing


# ------------------------------------------------------------------ status and refusals
def _edge_case():
    """FILEREADER 2 x 24: 50 whole sample frames and 2 bytes; pcm_bytes is no multiple of 6 or 16."""
    fmt, sp, stride, unit = layout("OUT_FILEREADER", 2, 24)
    nsmp, R = 50, 20
    pcm = np.random.default_rng(4).integers(1, 256, nsmp * stride + 2, dtype=np.uint8)
    assert len(pcm) % stride and len(pcm) % 16
    win = window_table([(nsmp - 10, 10),  # ends exactly at the last whole sample frame
                        (nsmp - 10, 11),  # one sample past it
                        (U64, 1),
                        (U64, 0)])        # empty: nothing is read, whatever pcm_first says
    return fmt, sp, stride, pcm, win, R, nsmp


def test_windows_at_and_past_the_end():
    fmt, sp, stride, pcm, win, R, nsmp = _edge_case()
    for flags in (0, MONO):
        rc, got, st = call_host(pcm, fmt, sp, win, R, R + 1, flags)
        want, want_st = ref_f32(pcm, fmt, sp, win, R, R + 1, flags)
        assert rc == 0 and st == want_st == [1, 2, 0, 0]
        assert_bits(got, want)
        planes = 1 if flags else 2
        assert got[:10].any() and not got[(R + 1) * planes: (R + 1) * planes + R].any()


def test_no_streams_and_no_samples():
    fmt, sp, stride, pcm, win, R, nsmp = _edge_case()
    rc, got, st = call_host(pcm, fmt, sp, win[:0], R, R, 0)
    assert rc == 0 and st == [0, 0, 0, 0] and got.size == 0
    rc, got, st = call_host(pcm, fmt, sp, win, 0, 3, 0)  # row_samples 0: nothing written, the windows still counted
    assert rc == 0 and st == [1, 2, 1, 0]
    assert (got == CANARY).all()


def test_refusals():
    fmt, sp, stride, pcm, win, R, nsmp = _edge_case()
    L = libflac.load()

    def refused(word, fmt=fmt, sp=sp, R=R, pitch=R, flags=0, win=win, n=len(win)):
        planes = 1 if flags & MONO else sp.channels
        out = np.full(max(len(win) * planes * max(pitch, R), 1), CANARY, np.uint32)
        status = np.full(4, 0xA5A5A5A5, np.uint32)
        buf = padded(pcm)
        rc = L.bnflac_gather_ranges_f32_host(buf.ctypes.data_as(ctypes.c_void_p), len(pcm), fmt, ctypes.byref(sp),
                                             win.ctypes.data_as(ctypes.c_void_p), n, R, pitch, flags,
                                             out.ctypes.data_as(ctypes.c_void_p), status.ctypes.data_as(ctypes.c_void_p))
        assert rc == -1 and word in L.bnflac_last_error(), (word, rc, L.bnflac_last_error())
        assert (out == CANARY).all() and (status == 0xA5A5A5A5).all()

    refused(b"PLANAR32", fmt=libflac.OUT_PLANAR32)
    refused(b"bnflac_md5_layout", fmt=libflac.OUT_FLACDECODER)                    # 24-bit FLACDECODER bytes are not the samples
    refused(b"bnflac_md5_layout", fmt=libflac.OUT_FILEREADER, sp=params(2, 20))
    refused(b"bnflac_md5_layout", fmt=libflac.OUT_FLACDECODER, sp=params(3, 16))
    refused(b"bnflac_md5_layout", fmt=libflac.OUT_INTERLEAVED32, sp=params(2, 3))
    refused(b"out_format", fmt=7)
    refused(b"channels", sp=params(0, 24))
    refused(b"channels", fmt=libflac.OUT_INTERLEAVED32, sp=params(9, 24))
    refused(b"flags", flags=2)
    refused(b"flags", flags=MONO | 0x80000000)
    refused(b"plane_pitch", pitch=R - 1)
    refused(b"too many streams", n=1 << 30)
    # null arguments, by the rules of bnflac_gather_ranges
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    out, status, buf = np.zeros(4 * 2 * R, np.float32), np.zeros(4, np.uint32), padded(pcm)
    args = lambda **kw: [kw.get("pcm", vp(buf)), len(pcm), fmt, kw.get("sp", ctypes.byref(sp)), kw.get("win", vp(win)), len(win), R, R,
                         0, kw.get("out", vp(out)), kw.get("status", vp(status))]
    for kw in ({"pcm": None}, {"sp": None}, {"win": None}, {"out": None}, {"status": None}):
        assert L.bnflac_gather_ranges_f32_host(*args(**kw)) == -1 and b"null" in L.bnflac_last_error(), kw
    assert L.bnflac_gather_ranges_f32_host(*args()) == 0


def test_wrapper_matches_the_raw_call():
    fmt, sp, stride, pcm, win, R, nsmp = _edge_case()
    for mono in (False, True):
        planes, status = libflac.gather_ranges_f32_host(pcm, fmt, sp, win, R, mono=mono, plane_pitch=R + 3)
        want, want_st = ref_f32(pcm, fmt, sp, win, R, R, MONO if mono else 0)
        assert planes.dtype == np.float32 and planes.shape == (4, 1 if mono else 2, R)
        assert_bits(np.ascontiguousarray(planes).view(np.uint32).reshape(-1), want)
        assert status.tolist() == want_st
    assert libflac.f32_layout(params(2, 16)) == libflac.OUT_FLACDECODER and libflac.f32_layout(params(3, 16)) == libflac.OUT_FILEREADER
    assert libflac.f32_layout(params(2, 24)) == libflac.OUT_FILEREADER and libflac.f32_layout(params(2, 20)) == libflac.OUT_INTERLEAVED32
    assert libflac.F32_MONO == MONO


# ------------------------------------------------------------------ the rule under the sanitizers
@pytest.mark.skipif(_cxx() is None, reason="no C++ compiler")
def test_rule_under_asan_ubsan(tmp_path):
    """A program of its own (tools/gather_f32_sanitize.cpp), run directly: nothing is loaded into
    Python."""
    exe = str(tmp_path / "gather_f32_sanitize")
    cmd = [_cxx(), "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "birdnest", "audio_amd", "csrc"), os.path.join(ROOT, "tools", "gather_f32_sanitize.cpp"),
           "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and re.search(r"cannot find .*(asan|ubsan)|lib(clang_rt\.)?(asan|ubsan)[^ ]*: No such file", built.stderr):
        pytest.skip("the compiler lacks the sanitizer runtimes")
    assert built.returncode == 0, built.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "gather_f32_sanitize: ok" in r.stdout
