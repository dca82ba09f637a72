"""The rule of bnflac_gather_ranges_f32_rs on the host (bnflac_gather_ranges_f32_rs_host, no GPU),
bnflac_resample_design and bnflac_resample_request.

The yardstick is `ref_rs` below: the formula of include/bnflac.h in numpy float64 over the float32
taps and the float32 x values, gathered with an index matrix, independent of the library (no
tiles, no steps, no blocks).  A value y of the code under test must lie within
    |y - y64| <= gamma * sum_k |h_k x_k|,  gamma = n u / (1 - n u),  n = K / 4 + 2,  u = 2^-24:
each of the four accumulators takes K / 4 fused multiply-adds (one rounding each) and the two levels
of the final sum add two more, the standard bound for this order of accumulation.  It is derived,
not measured.  Everything that the contract gives bit for bit (zeros, identity, crops against the
whole, canaries) is compared on the bit pattern.  tests/test_gpu_gather_rs.py uses the same
yardstick and raw call for the device.

The last part builds tools/gather_rs_sanitize.cpp (the same rule, csrc/bnf_resample.h, in a program
of its own) with AddressSanitizer and UBSan and runs it.
"""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from birdnest.audio_amd import libflac
from tests.test_gather_f32_host import (CANARY, MONO, assert_bits, layout, padded, params, random_pcm, samples_of,
                                        window_table)
from tests.test_select_ranges_host import ROOT, U64, _cxx

TILE = libflac.RS_TILE
U = 2.0 ** -24
RATES = [(44100, 48000), (48000, 44100), (96000, 48000), (22050, 48000), (44100, 32000), (32000, 48000)]
_DESIGNS = {}


def design(rate_in, rate_out, **kw):
    key = (rate_in, rate_out, tuple(sorted(kw.items())))
    if key not in _DESIGNS:
        _DESIGNS[key] = libflac.resample_design(rate_in, rate_out, **kw)
    spec, taps = _DESIGNS[key]
    return libflac.ResampleSpec(spec.up, spec.down, spec.taps, 0), taps


def random_taps(rng, up, K):
    """A table that is no design: the contract is about the float32 values, whoever made them."""
    return (rng.standard_normal((up, K)) / K).astype(np.float32)


def gamma(K):
    n = K // 4 + 2
    return n * U / (1 - n * U)


def x_of(pcm, fmt, sp, flags):
    """The float32 x values of the whole PCM: [planes, frames] (the formulas of bnflac_gather_ranges_f32)."""
    unit = 4 if fmt == libflac.OUT_INTERLEAVED32 else 2 if fmt == libflac.OUT_FLACDECODER else sp.bps // 8
    smp = samples_of(pcm, unit * sp.channels, unit)
    if flags & MONO:
        return (smp.sum(axis=1).astype(np.float64) * 2.0 ** -(sp.bps - 1) / sp.channels).astype(np.float32)[None, :]
    return np.ascontiguousarray(smp.T.astype(np.int32).astype(np.float32) * np.float32(2.0 ** -(sp.bps - 1)))


def fir64(x, spec, taps, out_first, count):
    """Outputs out_first .. out_first + count - 1 of one plane x (float32[n]) -> (y64, sum |h x|), float64."""
    L, M, K = spec.up, spec.down, spec.taps
    c0 = K // 2 - 1
    j = np.arange(out_first, out_first + count, dtype=np.int64)
    q, ph = j * M // L, j * M % L
    xp = np.concatenate([np.zeros(K, np.float64), x.astype(np.float64), np.zeros(K + 1, np.float64)])
    idx = q[:, None] + np.arange(K)[None, :] - c0 + K
    prod = np.asarray(taps, np.float32).reshape(L, K)[ph].astype(np.float64) * xp[idx]
    return prod.sum(axis=1), np.abs(prod).sum(axis=1)


def ref_rs(pcm, fmt, sp, windows, spec, taps, R, pitch, flags):
    """-> (y64, bound, fixed, status): float64 arrays over every float from d_out on,
    (n * planes - 1) * pitch + R of them; fixed: 1 where the contract gives +0.0f, 2 where nothing is
    written, 0 where y64 and bound hold."""
    L, M = spec.up, spec.down
    X = x_of(pcm, fmt, sp, flags)
    limit = X.shape[1]
    planes = X.shape[0]
    n = len(windows)
    size = max((n * planes - 1) * pitch + R, 0)
    y, bound, fixed = np.zeros(size), np.zeros(size), np.full(size, 2, np.uint8)
    nbad = ncut = 0
    for s, w in enumerate(windows):
        first, ns = int(w["pcm_first"]), int(w["nsamples"])
        bad = ns != 0 and (first > limit or ns > limit - first)
        nbad += bad
        n_out = 0 if bad else max(0, -(-ns * L // M) - spec.out_first)
        ncut += n_out > R
        ncopy = min(n_out, R)
        for c in range(planes):
            at = (s * planes + c) * pitch
            fixed[at: at + R] = 1
            if ncopy:
                y[at: at + ncopy], bound[at: at + ncopy] = fir64(X[c, first: first + ns], spec, taps, spec.out_first, ncopy)
                bound[at: at + ncopy] *= gamma(spec.taps)
                fixed[at: at + ncopy] = 0
    return y, bound, fixed, [1 if nbad else 0, nbad, ncut, 0]


def assert_within(got_bits, ref, what=""):
    """got_bits: uint32 view of the floats; ref: (y64, bound, fixed, ...)"""
    y, bound, fixed = ref[:3]
    assert len(got_bits) == len(y), what
    assert_bits(got_bits[fixed == 2], np.full(int((fixed == 2).sum()), CANARY, np.uint32), what + ": not to be written")
    assert_bits(got_bits[fixed == 1], np.zeros(int((fixed == 1).sum()), np.uint32), what + ": +0.0f")
    v = got_bits.view(np.float32).astype(np.float64)[fixed == 0]
    err, lim = np.abs(v - y[fixed == 0]), bound[fixed == 0]
    assert np.isfinite(v).all(), what
    if (err > lim).any():
        k = int(np.flatnonzero(err > lim)[0])
        raise AssertionError("%s: value %d is %r off the float64 yardstick, the bound is %r" % (what, k, err[k], lim[k]))


def call_rs_host(pcm, fmt, sp, win, spec, taps, R, pitch, flags, tail=7):
    """bnflac_gather_ranges_f32_rs_host itself on an output of the contract's size plus `tail` canaries
    -> (rc, the output's bits with the tail checked and cut off, status[4] with its canary checked)"""
    n = len(win)
    planes = 1 if flags & MONO else max(sp.channels, 1)
    size = max((n * planes - 1) * pitch + R, 0)
    buf, win = padded(pcm), np.ascontiguousarray(win)
    tab = np.ascontiguousarray(taps, np.float32).reshape(-1)
    out = np.full(size + tail, CANARY, np.uint32)
    status = np.full(5, 0xA5A5A5A5, np.uint32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a.size else None
    rc = libflac.load().bnflac_gather_ranges_f32_rs_host(vp(buf), len(pcm), fmt, ctypes.byref(sp), vp(win), n,
                                                         ctypes.byref(spec), vp(tab), R, pitch, flags, vp(out), vp(status))
    assert (out[size:] == CANARY).all() and status[4] == 0xA5A5A5A5
    return rc, out[:size], status[:4].tolist()


def frames_for(R, spec):
    """Sample frames of a PCM that holds every window of windows_for."""
    full = -(-(R + spec.out_first) * spec.down // spec.up)
    return 17 + max(full + 2 * spec.down // spec.up + 3, spec.taps // 2) + 8


def windows_for(nsmp, R, spec):
    """Windows of every length class for rows of R outputs: empty, tiny, shorter than the filter, one
    that fills the row exactly, one that is cut, at source positions of every phase."""
    L, M = spec.up, spec.down
    full = -(-(R + spec.out_first) * M // L)  # the fewest sample frames that give R outputs behind out_first
    lens = sorted({0, 1, 3, spec.taps // 2, max(full - 2, 0), full, full + 2 * M // L + 3})
    pairs = [((3 * k + 1) % 17, n) for k, n in enumerate(lens)]
    assert all(f + n <= nsmp for f, n in pairs)
    return window_table(pairs)


# ------------------------------------------------------------------ the host twin against the float64 yardstick
@pytest.mark.parametrize("rate_in,rate_out", RATES, ids=["%d-%d" % r for r in RATES])
def test_host_twin_against_float64(rate_in, rate_out):
    spec, taps = design(rate_in, rate_out)
    rng = np.random.default_rng(rate_in % 1000 + rate_out % 777)
    R = 300
    for (name, channels, bps), out_first in ((("OUT_FLACDECODER", 2, 16), 0), (("OUT_FILEREADER", 3, 24), 5),
                                             (("OUT_INTERLEAVED32", 1, 32), 0)):
        fmt, sp, stride, unit = layout(name, channels, bps)
        sf = spec.with_out_first(out_first)
        nsmp = 17 + (R + out_first) * sf.down // sf.up + 2 * sf.down // sf.up + 8
        pcm = random_pcm(rng, nsmp * stride + 1, unit, bps)
        win = windows_for(nsmp, R, sf)
        for flags in (0, MONO):
            for pitch in (R, R + 5):
                rc, got, st = call_rs_host(pcm, fmt, sp, win, sf, taps, R, pitch, flags)
                ref = ref_rs(pcm, fmt, sp, win, sf, taps, R, pitch, flags)
                assert rc == 0, libflac.load().bnflac_last_error()
                assert st == ref[3] and st[2] >= 1  # at least the longest window is cut
                assert_within(got, ref, "%s flags %d pitch %d" % (name, flags, pitch))


def test_host_twin_across_tiles_and_steps():
    """Rows longer than two tiles; 1/8 takes several steps per tile, and a table that is no design."""
    rng = np.random.default_rng(12)
    fmt, sp, stride, unit = layout("OUT_FILEREADER", 2, 24)
    for up, down, K in ((160, 147, 32), (1, 8, 64), (3, 2, 4)):
        spec = libflac.ResampleSpec(up, down, K, 3)
        taps = random_taps(rng, up, K)
        R = 2 * TILE + 3
        nsmp = 17 + (R + 3) * down // up + 40
        pcm = random_pcm(rng, nsmp * stride, unit, 24)
        win = windows_for(nsmp, R, spec)
        for flags in (0, MONO):
            rc, got, st = call_rs_host(pcm, fmt, sp, win, spec, taps, R, R + 1, flags)
            ref = ref_rs(pcm, fmt, sp, win, spec, taps, R, R + 1, flags)
            assert rc == 0 and st == ref[3]
            assert_within(got, ref, "%d/%d flags %d" % (up, down, flags))


# ------------------------------------------------------------------ identity
@pytest.mark.parametrize("name,channels,bps", [("OUT_FLACDECODER", 2, 16), ("OUT_FILEREADER", 8, 24), ("OUT_INTERLEAVED32", 3, 20)])
def test_equal_rates_are_the_plain_gather(name, channels, bps):
    spec, taps = design(44100, 44100)
    assert (spec.up, spec.down, spec.taps, spec.out_first) == (1, 1, 4, 0) and taps.tolist() == [[0.0, 1.0, 0.0, 0.0]]
    fmt, sp, stride, unit = layout(name, channels, bps)
    rng = np.random.default_rng(channels)
    R = TILE + 9
    pcm = random_pcm(rng, (R + 30) * stride + 1, unit, bps)
    win = window_table([(0, 0), (1, 5), (2, R), (7, R + 9), (R + 29, 1), (U64, 1)])
    for mono in (False, True):
        got, st = libflac.gather_ranges_f32_rs_host(pcm, fmt, sp, win, spec, taps, R, mono=mono)
        want, want_st = libflac.gather_ranges_f32_host(pcm, fmt, sp, win, R, mono=mono)
        assert st.tolist() == want_st.tolist() == [1, 1, 1, 0]
        assert_bits(np.ascontiguousarray(got).view(np.uint32).reshape(-1), np.ascontiguousarray(want).view(np.uint32).reshape(-1))


# ------------------------------------------------------------------ crops tile the whole
@pytest.mark.parametrize("rate_in,rate_out", [(147, 160), (160, 147), (2, 1), (2, 3), (1, 6)],
                         ids=["160/147", "147/160", "1/2", "3/2", "6/1"])
def test_crops_tile_the_whole(rate_in, rate_out):
    spec, taps = design(rate_in, rate_out)
    L, M, K = spec.up, spec.down, spec.taps
    fmt, sp, stride, unit = layout("OUT_FLACDECODER", 2, 16)
    T, N = 1500, 200
    pcm = random_pcm(np.random.default_rng(L * 7 + M), T * stride, unit, 16)
    total = -(-T * L // M)
    whole, st = libflac.gather_ranges_f32_rs_host(pcm, fmt, sp, window_table([(0, T)]), spec, taps, total + N)
    assert st.tolist() == [0, 0, 0, 0] and not whole[0, :, total:].any() and whole[0, :, total - 1].any()
    whole = np.ascontiguousarray(whole[0]).view(np.uint32)
    for j0 in (0, 1, L, 777, total - N // 2, total - 1, total, total + 50):
        first, n, out_first = libflac.resample_request(spec, j0, N)
        c0 = K // 2 - 1
        b = max(0, j0 * M // L - c0) // M
        assert (first, out_first) == (M * b, j0 - L * b) and n == (j0 + N - 1) * M // L + K // 2 + 1 - first
        lo = min(first, T)
        hi = min(lo + n, T)  # the selection's clipping
        crop, st = libflac.gather_ranges_f32_rs_host(pcm, fmt, sp, window_table([(lo, hi - lo)]), spec.with_out_first(out_first),
                                                     taps, N)
        want = np.zeros((2, N), np.uint32)
        k = max(0, min(N, total + N - j0))
        want[:, :k] = whole[:, j0: j0 + k]
        assert_bits(np.ascontiguousarray(crop[0]).view(np.uint32).reshape(-1), want.reshape(-1), "outputs from %d" % j0)
        assert st.tolist()[:2] == [0, 0]
    assert libflac.resample_request(spec, 5, 0)[1] == 0


# ------------------------------------------------------------------ the design
def design_numpy(rate_in, rate_out, zeros=16.0, rolloff=0.945, beta=9.0):
    g = math.gcd(rate_in, rate_out)
    L, M = rate_out // g, rate_in // g
    s = min(1.0, L / M)
    fc = rolloff * s
    K = (2 * math.ceil(zeros / s) + 3) // 4 * 4
    c0 = K // 2 - 1
    tau = (np.arange(K)[None, :] - c0) - np.arange(L)[:, None] / L
    inside = np.abs(tau) < K / 2
    w = np.where(inside, np.i0(beta * np.sqrt(np.where(inside, 1 - (tau / (K / 2)) ** 2, 0.0))) / np.i0(beta), 0.0)
    gk = fc * np.sinc(fc * tau) * w
    return L, M, K, gk / gk.sum(axis=1, keepdims=True)


@pytest.mark.parametrize("rate_in,rate_out", RATES + [(8000, 48000), (48000, 8000)], ids=lambda r: str(r))
def test_design_is_the_formula(rate_in, rate_out):
    spec, taps = design(rate_in, rate_out)
    L, M, K, h = design_numpy(rate_in, rate_out)
    assert (spec.up, spec.down, spec.taps, spec.out_first) == (L, M, K, 0) and taps.shape == (L, K) and taps.dtype == np.float32
    assert np.abs(taps.astype(np.float64) - h).max() <= 2.0 ** -24
    assert np.abs(taps.astype(np.float64).sum(axis=1) - 1).max() <= K * 2.0 ** -24


def test_design_parameters_and_refusals():
    spec, taps = design(44100, 48000, zeros=8.0, rolloff=0.9, beta=6.0)
    L, M, K, h = design_numpy(44100, 48000, 8.0, 0.9, 6.0)
    assert (spec.up, spec.down, spec.taps) == (160, 147, 16) == (L, M, K) and np.abs(taps - h).max() <= 2.0 ** -24
    spec, taps = design(48000, 44100, zeros=7.0)
    assert spec.taps == design_numpy(48000, 44100, 7.0)[2] == 16
    Lb = libflac.load()
    s = libflac.ResampleSpec()
    buf = np.full(16, CANARY, np.uint32)
    vp = buf.ctypes.data_as(ctypes.c_void_p)
    with pytest.raises(RuntimeError, match=r"up = 640 x taps = 32"):
        libflac.resample_design(11025, 48000)
    assert libflac.resample_design(11025, 48000, zeros=12.0)[0].taps == 24  # the message says what to lower
    assert Lb.bnflac_resample_design(0, 48000, 0, 0, 0, ctypes.byref(s), vp, 16) < 0 and b"zero" in Lb.bnflac_last_error()
    assert Lb.bnflac_resample_design(48000, 0, 0, 0, 0, ctypes.byref(s), vp, 16) < 0 and b"zero" in Lb.bnflac_last_error()
    assert Lb.bnflac_resample_design(1, 65537, 0, 0, 0, ctypes.byref(s), vp, 16) < 0
    assert Lb.bnflac_resample_design(2, 1, 200.0, 0, 0, ctypes.byref(s), vp, 16) < 0 and b"taps = 800" in Lb.bnflac_last_error()
    assert Lb.bnflac_resample_design(44100, 48000, 0, 0, 0, None, vp, 16) < 0
    # a short taps_cap: the size and the spec come back, the table is not written
    assert Lb.bnflac_resample_design(44100, 48000, 0, 0, 0, ctypes.byref(s), vp, 16) == 160 * 32
    assert (s.up, s.down, s.taps, s.out_first) == (160, 147, 32, 0) and (buf == CANARY).all()
    assert Lb.bnflac_resample_design(5, 5, 0, 0, 0, ctypes.byref(s), vp, 4) == 4 and (buf[4:] == CANARY).all()
    assert buf[:4].view(np.float32).tolist() == [0.0, 1.0, 0.0, 0.0]


# ------------------------------------------------------------------ refusals of the gather
def test_gather_refusals():
    fmt, sp, stride, unit = layout("OUT_FILEREADER", 2, 24)
    R, nsmp = 20, 50
    pcm = np.random.default_rng(4).integers(1, 256, nsmp * stride + 2, dtype=np.uint8)
    win = window_table([(0, 10), (5, 40), (U64, 1)])
    good, taps = design(3, 2)
    L = libflac.load()
    big = np.zeros(16384 + 64, np.float32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def refused(word, fmt=fmt, sp=sp, R=R, pitch=R, flags=0, n=len(win), spec=good):
        planes = 1 if flags & MONO else max(sp.channels, 1)
        out = np.full(max(len(win) * planes * min(max(pitch, R), 64), 1), CANARY, np.uint32)  # a refused call writes nothing
        status = np.full(4, 0xA5A5A5A5, np.uint32)
        rc = L.bnflac_gather_ranges_f32_rs_host(vp(padded(pcm)), len(pcm), fmt, ctypes.byref(sp), vp(win), n, ctypes.byref(spec),
                                                vp(big), R, pitch, flags, vp(out), vp(status))
        assert rc < 0 and word in L.bnflac_last_error(), (word, rc, L.bnflac_last_error())
        assert (out == CANARY).all() and (status == 0xA5A5A5A5).all()

    S = libflac.ResampleSpec
    refused(b"1..65535", spec=S(0, 1, 4, 0))
    refused(b"1..65535", spec=S(1, 0, 4, 0))
    refused(b"1..65535", spec=S(65536, 1, 4, 0))
    refused(b"1..65535", spec=S(1, 65537, 4, 0))
    refused(b"coprime", spec=S(4, 6, 4, 0))
    refused(b"multiple of 4", spec=S(3, 2, 0, 0))
    refused(b"multiple of 4", spec=S(3, 2, 6, 0))
    refused(b"multiple of 4", spec=S(3, 2, 516, 0))
    refused(b"16384", spec=S(4097, 2, 4, 0))
    refused(b"16384", spec=S(33, 2, 512, 0))
    refused(b"out_first", spec=S(3, 2, 4, 1 << 31))
    refused(b"row_out", R=1 << 31, pitch=1 << 31)
    refused(b"PLANAR32", fmt=libflac.OUT_PLANAR32)
    refused(b"bnflac_md5_layout", fmt=libflac.OUT_FLACDECODER)
    refused(b"bnflac_md5_layout", fmt=libflac.OUT_FILEREADER, sp=params(2, 20))
    refused(b"out_format", fmt=7)
    refused(b"channels", sp=params(0, 24))
    refused(b"channels", fmt=libflac.OUT_INTERLEAVED32, sp=params(9, 24))
    refused(b"flags", flags=2)
    refused(b"flags", flags=MONO | 0x80000000)
    refused(b"plane_pitch", pitch=R - 1)
    refused(b"too many streams", n=1 << 30)
    out, status, buf = np.zeros(3 * 2 * R, np.float32), np.zeros(4, np.uint32), padded(pcm)
    args = lambda **kw: [kw.get("pcm", vp(buf)), len(pcm), fmt, kw.get("sp", ctypes.byref(sp)), kw.get("win", vp(win)), len(win),
                         kw.get("spec", ctypes.byref(good)), kw.get("taps", vp(big)), R, R, 0, kw.get("out", vp(out)),
                         kw.get("status", vp(status))]
    for kw in ({"pcm": None}, {"sp": None}, {"win": None}, {"out": None}, {"status": None}, {"spec": None}, {"taps": None}):
        assert L.bnflac_gather_ranges_f32_rs_host(*args(**kw)) == -1 and b"null" in L.bnflac_last_error(), kw
    assert L.bnflac_gather_ranges_f32_rs_host(*args()) == 0 and status.tolist() == [1, 1, 1, 0]
    # the largest tables are taken: up * taps = 16384 both ways, and no streams
    for spec in (S(32, 1, 512, 0), S(4096, 1, 4, 0)):
        assert L.bnflac_gather_ranges_f32_rs_host(*args(spec=ctypes.byref(spec))) == 0
    rc, got, st = call_rs_host(pcm, fmt, sp, win[:0], good, taps, R, R, 0)
    assert rc == 0 and st == [0, 0, 0, 0] and got.size == 0
    rc, got, st = call_rs_host(pcm, fmt, sp, win, good, taps, 0, 3, 0)  # row_out 0: nothing written, the windows still counted
    assert rc == 0 and st == [1, 1, 2, 0] and (got == CANARY).all()
    for bad in (S(0, 1, 4, 0), S(3, 2, 6, 0)):
        with pytest.raises(RuntimeError):
            libflac.resample_request(bad, 0, 10)


# ------------------------------------------------------------------ a tone
TONE_MEASURED = 1.94e-5  # the float64 yardstick's own error for this input (1.933e-05, rounded up), see DESIGN.md "Windows at another rate"
TONE_TOLERANCE = 2 * TONE_MEASURED  # a factor 2 for the float32 accumulation


def test_tone_44100_to_48000():
    """A 1 kHz sine at 0.9 of 24-bit full scale through the default 44100 -> 48000 design against the
    analytic sine, away from the edges.  The error is the design's (stopband and passband ripple) and
    the input's quantisation; the float64 yardstick has it too, and its measured value sets the
    tolerance: twice that, for the float32 accumulation."""
    spec, taps = design(44100, 48000)
    fmt, sp, stride, unit = layout("OUT_FILEREADER", 1, 24)
    T = 4410
    v = np.round(0.9 * (2 ** 23 - 1) * np.sin(2 * np.pi * 1000.0 * np.arange(T) / 44100.0)).astype(np.int64)
    pcm = np.zeros(T * 3, np.uint8)
    for k in range(3):
        pcm[k::3] = (v >> (8 * k)) & 0xFF
    n_out = T * 160 // 147
    got, st = libflac.gather_ranges_f32_rs_host(pcm, fmt, sp, window_table([(0, T)]), spec, taps, n_out)
    assert st.tolist() == [0, 0, 0, 0]
    edge = spec.taps
    j = np.arange(edge, n_out - edge)
    want = 0.9 * (2 ** 23 - 1) / 2.0 ** 23 * np.sin(2 * np.pi * 1000.0 * j / 48000.0)
    y64, _ = fir64(x_of(pcm, fmt, sp, 0)[0], spec, taps, 0, n_out)
    err64 = np.abs(y64[j] - want).max()
    err = np.abs(got[0, 0, j].astype(np.float64) - want).max()
    print("tone: float64 yardstick %.3e, host twin %.3e, tolerance %.3e" % (err64, err, TONE_TOLERANCE))
    assert err64 <= TONE_MEASURED, "the yardstick's own error is what the tolerance was taken from"
    assert err <= TONE_TOLERANCE


# ------------------------------------------------------------------ the rule under the sanitizers
@pytest.mark.skipif(_cxx() is None, reason="no C++ compiler")
def test_rule_under_asan_ubsan(tmp_path):
    """A program of its own (tools/gather_rs_sanitize.cpp), run directly: nothing is loaded into
    Python."""
    exe = str(tmp_path / "gather_rs_sanitize")
    cmd = [_cxx(), "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "birdnest", "audio_amd", "csrc"), os.path.join(ROOT, "tools", "gather_rs_sanitize.cpp"),
           "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and re.search(r"cannot find .*(asan|ubsan)|lib(clang_rt\.)?(asan|ubsan)[^ ]*: No such file", built.stderr):
        pytest.skip("the compiler lacks the sanitizer runtimes")
    assert built.returncode == 0, built.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "gather_rs_sanitize: ok" in r.stdout
