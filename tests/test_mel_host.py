"""The rule of bnflac_gather_ranges_mel on the host (bnflac_gather_ranges_mel_host, no GPU),
bnflac_mel_design and bnflac_mel_request.

The yardstick is `ref_mel` below: the definition of include/bnflac.h in numpy float64 over the float32
table values and the float32 x values (np.fft.rfft of w * x with exact twiddles, the square, the band
sums), independent of the library (no tiles, no steps, no bit reversal).  A value of the code under
test must lie within a bound that is derived, not measured (DESIGN.md "Windows as mel spectrograms"),
with u = 2^-24 and t = log2 N:
    eta   = mu + gamma_4 (sqrt 2 + mu), mu = u: a design's twiddles are cos and sin rounded to float32
    eps   = t eta / (1 - t eta) * (1 + u) + u     Higham, Accuracy and Stability, Theorem 24.2, on the
                                                  rounded products w * x (one more u)
    E     = eps * sqrt(N) * ||w x||_2             the norm-wise bound holds for every bin
    dP[k] = (2 |X[k]| E + E^2) (1 + gamma_2) + gamma_2 |X[k]|^2       the product and the fmaf of P
    row   : sum |w_i| dP_i + gamma_nb sum |w_i| (P_i + dP_i)          the chain of nb fmafs
          (n_mels == 0: dP[k]).
Everything that the contract gives bit for bit (zeros, crops against the whole, canaries) is compared
on the bit pattern.  tests/test_gpu_gather_mel.py uses the same raw call for the device.

The last part builds tools/gather_mel_sanitize.cpp (the same rule, csrc/bnf_mel.h, in a program of its
own) with AddressSanitizer and UBSan and runs it.
"""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from birdnest.audio_amd import libflac
from tests.test_gather_f32_host import CANARY, MONO, assert_bits, layout, padded, params, random_pcm, window_table
from tests.test_resample_host import assert_within, x_of
from tests.test_select_ranges_host import ROOT, U64, _cxx

TF = libflac.MEL_TILE
U = 2.0 ** -24
_DESIGNS = {}


def design(sample_rate, n_fft, hop, n_mels, **kw):
    key = (sample_rate, n_fft, hop, n_mels, tuple(sorted(kw.items())))
    if key not in _DESIGNS:
        _DESIGNS[key] = libflac.mel_design(sample_rate, n_fft, hop, n_mels, **kw)
    spec, tab, bands = _DESIGNS[key]
    return spec.with_origin(spec.origin), tab, bands


def gam(n):
    return n * U / (1 - n * U)


def checked_bands(spec, bands):
    """-> [(first, woff, nb)] with nb = 0 for a bad band, and how many are bad: the contract's check."""
    out, nbad = [], 0
    half = spec.n_fft // 2 + 1
    b = np.asarray(bands, np.uint32).reshape(-1, 2).astype(np.int64) if spec.n_mels else np.zeros((1, 2), np.int64)
    for m in range(spec.n_mels):
        f, w0, w1 = int(b[m, 0]), int(b[m, 1]), int(b[m + 1, 1])
        if w1 < w0 or w1 > spec.n_weights or f + (w1 - w0) > half:
            out.append((0, 0, 0))
            nbad += 1
        else:
            out.append((f, w0, w1 - w0))
    return out, nbad


def n_valid_of(n, spec):
    c = n - spec.n_fft // 2 - spec.origin
    return 0 if n == 0 or c < 0 else c // spec.hop + 1


def frames64(x, spec, tab, count):
    """Frames 0 .. count - 1 of one plane x (float32[n]) -> w * x in float64, [count, N]."""
    N = spec.n_fft
    w = np.asarray(tab[:N], np.float32).astype(np.float64)
    fr = np.zeros((count, N))
    for t in range(count):
        a = spec.origin + t * spec.hop
        lo, hi = max(a, 0), min(a + N, len(x))
        if hi > lo:
            fr[t, lo - a: hi - a] = x[lo:hi].astype(np.float64)
    return fr * w[None, :]


def rows64(x, spec, tab, bands, count):
    """-> (rows64, bound), float64[rows, count]: the definition and the derived bound."""
    N = spec.n_fft
    t = int(math.log2(N))
    fr = frames64(x, spec, tab, count)
    X = np.abs(np.fft.rfft(fr, axis=1))  # [count, N/2 + 1]
    P = X * X
    eta = U + gam(4) * (math.sqrt(2.0) + U)
    eps = t * eta / (1 - t * eta) * (1 + U) + U
    E = eps * math.sqrt(N) * np.sqrt((fr * fr).sum(axis=1))[:, None]
    dP = (2 * X * E + E * E) * (1 + gam(2)) + gam(2) * P
    if not spec.n_mels:
        return P.T, dP.T
    wt = np.asarray(tab[2 * N:], np.float32).astype(np.float64)
    y, bound = np.zeros((spec.n_mels, count)), np.zeros((spec.n_mels, count))
    for m, (f, w0, nb) in enumerate(checked_bands(spec, bands)[0]):
        if nb:
            aw = np.abs(wt[w0: w0 + nb])
            y[m] = P[:, f: f + nb] @ wt[w0: w0 + nb]
            bound[m] = dP[:, f: f + nb] @ aw + gam(nb) * ((P + dP)[:, f: f + nb] @ aw)
    return y, bound


def ref_mel(pcm, fmt, sp, windows, spec, tab, bands, R, pitch, flags):
    """-> (y64, bound, fixed, status): float64 arrays over every float from d_out on,
    (n * planes * rows - 1) * pitch + R of them; fixed: 1 where the contract gives +0.0f, 2 where
    nothing is written, 0 where y64 and bound hold."""
    X = x_of(pcm, fmt, sp, flags)
    limit, planes, rows = X.shape[1], X.shape[0], spec.rows
    n = len(windows)
    size = max((n * planes * rows - 1) * pitch + R, 0)
    y, bound, fixed = np.zeros(size), np.zeros(size), np.full(size, 2, np.uint8)
    nbad = ncut = 0
    for s, w in enumerate(windows):
        first, ns = int(w["pcm_first"]), int(w["nsamples"])
        bad = ns != 0 and (first > limit or ns > limit - first)
        nbad += bad
        nv = 0 if bad else n_valid_of(ns, spec)
        ncut += nv > R
        ncopy = min(nv, R)
        for c in range(planes):
            if ncopy:
                yy, bb = rows64(X[c, first: first + ns], spec, tab, bands, ncopy)
            for r in range(rows):
                at = ((s * planes + c) * rows + r) * pitch
                fixed[at: at + R] = 1
                if ncopy:
                    y[at: at + ncopy], bound[at: at + ncopy] = yy[r], bb[r]
                    fixed[at: at + ncopy] = 0
    nbb = checked_bands(spec, bands)[1] if n else 0
    return y, bound, fixed, [(1 if nbad else 0) | (2 if nbb else 0), nbad, ncut, nbb]


def call_mel_host(pcm, fmt, sp, win, spec, tab, bands, R, pitch, flags, tail=7):
    """bnflac_gather_ranges_mel_host itself on an output of the contract's size plus `tail` canaries
    -> (rc, the output's bits with the tail checked and cut off, status[4] with its canary checked)"""
    n = len(win)
    planes = 1 if flags & MONO else max(sp.channels, 1)
    size = max((n * planes * spec.rows - 1) * pitch + R, 0)
    buf, win = padded(pcm), np.ascontiguousarray(win)
    tab = np.ascontiguousarray(tab, np.float32).reshape(-1)
    bnd = np.zeros(0, np.uint32) if bands is None else np.ascontiguousarray(bands, np.uint32).reshape(-1)
    out = np.full(size + tail, CANARY, np.uint32)
    status = np.full(5, 0xA5A5A5A5, np.uint32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a.size else None
    rc = libflac.load().bnflac_gather_ranges_mel_host(vp(buf), len(pcm), fmt, ctypes.byref(sp), vp(win), n, ctypes.byref(spec),
                                                      vp(tab), vp(bnd), R, pitch, flags, vp(out), vp(status))
    assert (out[size:] == CANARY).all() and status[4] == 0xA5A5A5A5
    return rc, out[:size], status[:4].tolist()


def random_tables(rng, spec_design, tab, n_mels, n_weights):
    """Tables that are no design apart from the twiddles: a random window, random weights (some
    negative), bands at random places that may overlap.  -> (spec, tab, bands)"""
    N = spec_design.n_fft
    t = np.concatenate([rng.standard_normal(N).astype(np.float32), np.asarray(tab[N: 2 * N], np.float32),
                        rng.standard_normal(n_weights).astype(np.float32)])
    cuts = np.sort(rng.integers(0, n_weights + 1, n_mels - 1)) if n_mels > 1 else np.zeros(0, np.int64)
    woff = np.concatenate([[0], cuts, [n_weights]]).astype(np.int64)
    nb = np.minimum(np.diff(woff), N // 2 + 1)
    woff = np.concatenate([[0], np.cumsum(nb)])
    first = [int(rng.integers(0, N // 2 + 2 - k)) for k in nb] + [0]
    bands = np.stack([np.asarray(first, np.uint32), woff.astype(np.uint32)], axis=1)
    return libflac.MelSpec(N, spec_design.hop, n_mels, spec_design.origin, int(woff[-1])), t[: 2 * N + int(woff[-1])], bands


def windows_for(nsmp, R, spec):
    """Windows of every length class for rows of R frames: empty, one sample, shorter than a frame,
    one frame's worth, two hops short of the row, filling it, cut; at source positions of every phase."""
    N, hop = spec.n_fft, spec.hop
    full = max((R - 1) * hop + N // 2 + spec.origin, 1)  # the fewest sample frames that give R frames
    lens = sorted({0, 1, N - 1, N, max(full - 2 * hop, 0), full, full + 2 * hop + 3})
    pairs = [((3 * k + 1) % 17, n) for k, n in enumerate(lens)]
    assert all(f + n <= nsmp for f, n in pairs), (nsmp, pairs)
    return window_table(pairs)


def frames_needed(R, spec):
    return 17 + max((R - 1) * spec.hop + spec.n_fft // 2 + spec.origin, 1) + 2 * spec.hop + 3 + spec.n_fft


# ------------------------------------------------------------------ the host twin against the float64 yardstick
CASES = [(64, 16, 40, "OUT_FLACDECODER", 2, 16), (512, 100, 40, "OUT_FILEREADER", 2, 24), (2048, 512, 128, "OUT_INTERLEAVED32", 8, 24),
         (512, 128, 0, "OUT_FLACDECODER", 1, 16), (2048, 300, 0, "OUT_FILEREADER", 1, 24), (64, 1, 7, "OUT_INTERLEAVED32", 3, 20)]


@pytest.mark.parametrize("n_fft,hop,n_mels,name,channels,bps", CASES, ids=["N%d-h%d-m%d-%s-%dch" % (c[0], c[1], c[2], c[3][4:], c[4]) for c in CASES])
def test_host_twin_against_float64(n_fft, hop, n_mels, name, channels, bps):
    spec, tab, bands = design(48000, n_fft, hop, n_mels)
    fmt, sp, stride, unit = layout(name, channels, bps)
    rng = np.random.default_rng(n_fft + hop + channels)
    R = TF + 5 if n_fft < 2048 else 9
    nsmp = frames_needed(R, spec)
    pcm = random_pcm(rng, nsmp * stride + 1, unit, bps)
    win = windows_for(nsmp, R, spec)
    for flags in (0, MONO):
        for pitch in (R, R + 5):
            rc, got, st = call_mel_host(pcm, fmt, sp, win, spec, tab, bands if n_mels else None, R, pitch, flags)
            ref = ref_mel(pcm, fmt, sp, win, spec, tab, bands, R, pitch, flags)
            assert rc == 0, libflac.load().bnflac_last_error()
            assert st == ref[3] and st[2] >= 1 and st[0] == 0
            assert_within(got, ref, "%s flags %d pitch %d" % (name, flags, pitch))


def test_host_twin_with_tables_that_are_no_design():
    """The contract is about the tables' values: a random window, negative weights, overlapping bands."""
    rng = np.random.default_rng(5)
    fmt, sp, stride, unit = layout("OUT_FILEREADER", 2, 24)
    for n_fft, hop, n_mels, nw in ((256, 37, 40, 900), (64, 80, 1, 33), (1024, 256, 256, 8192)):
        d, dtab, _ = design(48000, n_fft, hop, 0)
        spec, tab, bands = random_tables(rng, d, dtab, n_mels, nw)
        R = 11
        nsmp = frames_needed(R, spec)
        pcm = random_pcm(rng, nsmp * stride, unit, 24)
        win = windows_for(nsmp, R, spec)
        rc, got, st = call_mel_host(pcm, fmt, sp, win, spec, tab, bands, R, R + 1, 0)
        ref = ref_mel(pcm, fmt, sp, win, spec, tab, bands, R, R + 1, 0)
        assert rc == 0 and st == ref[3] and st[3] == 0
        assert_within(got, ref, "N %d mels %d" % (n_fft, n_mels))


# ------------------------------------------------------------------ the definition
FOOT = 1e-9  # a weight below this is a triangle's foot: a bin that sits on a corner frequency up to rounding


def htk_dense(sample_rate, n_fft, n_mels, f_min=0.0, f_max=None):
    """The formula of include/bnflac.h in float64, operation by operation as it is written there (what
    torchaudio.functional.melscale_fbanks(n_fft // 2 + 1, f_min, f_max, n_mels, sample_rate, norm=None,
    mel_scale="htk") computes in float32): [n_fft // 2 + 1, n_mels]."""
    f_max = sample_rate / 2 if f_max is None else f_max
    mel = lambda f: 2595.0 * math.log10(1.0 + f / 700.0)
    m0, m1 = mel(f_min), mel(f_max)
    dm = (m1 - m0) / (n_mels + 1)
    pts = np.array([700.0 * (math.pow(10.0, (m0 + dm * j) / 2595.0) - 1.0) for j in range(n_mels + 2)])
    g = np.arange(n_fft // 2 + 1) * float(sample_rate) / n_fft
    up = (g[:, None] - pts[None, :-2]) / (pts[1:-1] - pts[:-2])[None, :]
    down = (pts[None, 2:] - g[:, None]) / (pts[2:] - pts[1:-1])[None, :]
    return np.maximum(0.0, np.minimum(up, down))


def assert_weights_are_htk(spec, tab, bands, sample_rate, f_min=0.0, f_max=None):
    """The table's weights against the formula rounded to float32.  A weight goes through log10 and pow
    (the corner frequencies) before its rounding to float32, and C's libm may differ from Python's in
    the last place of the double, so every weight above FOOT is allowed one float32 ulp, and it must be
    there.  Only the feet, where a bin sits on a corner frequency and the formula gives 0 up to the
    rounding of that corner (the Nyquist bin under the last triangle's end is one), may appear or
    vanish, and no other entry may: n_weights is the formula's count apart from them."""
    want64 = htk_dense(sample_rate, spec.n_fft, spec.n_mels, f_min, f_max)
    want, got = want64.astype(np.float32), dense_of(spec, tab, bands).astype(np.float32)
    body = want64 > FOOT
    assert (got[body] > 0).all() and ulps(got[body], want[body]).max() <= 1
    assert (got[~body] <= FOOT).all() and (got[~body] >= 0).all()
    assert spec.n_weights == int(body.sum()) + int(np.count_nonzero(got[~body]))


def dense_of(spec, tab, bands):
    fb = np.zeros((spec.n_fft // 2 + 1, spec.n_mels))
    wt = np.asarray(tab[2 * spec.n_fft:], np.float32).astype(np.float64)
    for m, (f, w0, nb) in enumerate(checked_bands(spec, bands)[0]):
        fb[f: f + nb, m] = wt[w0: w0 + nb]
    return fb


@pytest.mark.parametrize("n_fft,hop,n_mels", [(512, 128, 64), (1024, 100, 128), (64, 64, 0)])
def test_yardstick_is_torch_stft_times_the_htk_filterbank(n_fft, hop, n_mels):
    """origin = -N/2 is torch.stft(center=True, pad_mode="constant"); n_valid is 1 + n // hop."""
    import torch
    sr = 32000
    spec, tab, bands = design(sr, n_fft, hop, n_mels)
    assert spec.origin == -(n_fft // 2)
    rng = np.random.default_rng(n_fft)
    for n in (n_fft * 3 + 17, hop * 9, 5):
        x = rng.uniform(-1, 1, n).astype(np.float32)
        nv = n_valid_of(n, spec)
        assert nv == 1 + n // hop
        y, _ = rows64(x, spec, tab, bands, nv)
        w = torch.from_numpy(np.asarray(tab[:n_fft], np.float32).astype(np.float64))
        S = torch.stft(torch.from_numpy(x.astype(np.float64)), n_fft, hop_length=hop, window=w, center=True, pad_mode="constant",
                       return_complex=True)
        assert tuple(S.shape) == (n_fft // 2 + 1, nv)
        P = (S.abs() ** 2).numpy()
        want = dense_of(spec, tab, bands).T @ P if n_mels else P
        scale = max(np.abs(want).max(), 1e-30)
        assert np.abs(y - want).max() <= 1e-12 * scale
        if n_mels:  # and the table's weights are the dense HTK filterbank's, rounded to float32
            assert_weights_are_htk(spec, tab, bands, sr)


# ------------------------------------------------------------------ crops are columns of the whole
@pytest.mark.parametrize("n_fft,hop,n_mels", [(256, 100, 20), (64, 7, 0), (512, 700, 30)])
def test_crops_are_columns_of_the_whole(n_fft, hop, n_mels):
    spec, tab, bands = design(44100, n_fft, hop, n_mels)
    fmt, sp, stride, unit = layout("OUT_FLACDECODER", 2, 16)
    T, NF = 9000, 12
    assert 4096 % hop
    pcm = random_pcm(np.random.default_rng(n_fft + hop), T * stride, unit, 16)
    total = 1 + T // hop
    whole, st = libflac.gather_ranges_mel_host(pcm, fmt, sp, window_table([(0, T)]), spec, tab, bands, total + NF)
    assert st.tolist() == [0, 0, 0, 0] and not whole[0, :, :, total:].any() and whole[0, :, :, total - 1].any()
    whole = np.ascontiguousarray(whole[0]).view(np.uint32)
    for t0 in (0, 1, total // 2, total - NF, total - NF // 2, total - 1, total, total + 40):
        first, n, origin = libflac.mel_request(spec, t0, NF)
        start = spec.origin + t0 * hop
        assert first == max(0, start) and origin == start - first and n == max(0, start + (NF - 1) * hop + n_fft - first)
        lo = min(first, T)
        hi = min(lo + n, T)  # the selection's clipping
        crop, st = libflac.gather_ranges_mel_host(pcm, fmt, sp, window_table([(lo, hi - lo)]), spec.with_origin(origin), tab, bands, NF)
        want = np.zeros((2, spec.rows, NF), np.uint32)
        k = max(0, min(NF, total + NF - t0))
        want[:, :, :k] = whole[:, :, t0: t0 + k]
        assert_bits(np.ascontiguousarray(crop[0]).view(np.uint32).reshape(-1), want.reshape(-1), "frames from %d" % t0)
        assert st.tolist()[:2] == [0, 0]
    assert libflac.mel_request(spec, 5, 0)[1] == 0


# ------------------------------------------------------------------ the design
def ulps(a, b):
    """Distance in float32 steps between two float32 arrays of one sign pattern (or zeros)."""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


@pytest.mark.parametrize("sr,n_fft,n_mels,f_min,f_max", [(48000, 1024, 128, 0.0, 0.0), (16000, 512, 40, 20.0, 7600.0),
                                                         (44100, 2048, 256, 0.0, 0.0), (22050, 64, 10, 0.0, 0.0), (48000, 256, 0, 0.0, 0.0)])
def test_design_is_the_formula(sr, n_fft, n_mels, f_min, f_max):
    """Every entry goes through libm (cos, sin; log10 and pow for the weights) in double before its
    rounding to float32, and Python's may differ from C's in the last place of the double: every entry
    of the window, the twiddles and the weights is allowed one float32 ulp (assert_weights_are_htk says
    which weights may appear or vanish); the band layout and n_weights are exact."""
    spec, tab, bands = design(sr, n_fft, 160, n_mels, f_min=f_min, f_max=f_max)
    N = n_fft
    assert (spec.n_fft, spec.hop, spec.n_mels, spec.origin, list(spec.reserved)) == (N, 160, n_mels, -(N // 2), [0, 0, 0])
    assert tab.dtype == np.float32 and tab.size == 2 * N + spec.n_weights
    i = np.arange(N)
    assert ulps(tab[:N], (0.5 - 0.5 * np.cos(2 * np.pi * i / N)).astype(np.float32)).max() <= 1
    k = np.arange(N // 2)
    assert ulps(tab[N: 2 * N: 2], np.cos(2 * np.pi * k / N).astype(np.float32))[np.abs(np.cos(2 * np.pi * k / N)) > 1e-9].max() <= 1
    assert ulps(tab[N + 1: 2 * N: 2], np.sin(2 * np.pi * k / N).astype(np.float32)).max() <= 1
    assert tab[N] == 1.0 and tab[N + 1] == 0.0 and abs(float(tab[N + N // 2])) < 1e-16 and tab[N + N // 2 + 1] == 1.0
    if not n_mels:
        assert spec.n_weights == 0 and bands.shape == (0, 2)
        return
    assert bands.shape == (n_mels + 1, 2) and bands.dtype == np.uint32
    woff = bands[:, 1].astype(np.int64)
    nb = np.diff(woff)
    assert woff[0] == 0 and (nb >= 0).all() and woff[-1] == spec.n_weights and tuple(bands[-1]) == (0, spec.n_weights)
    assert (bands[:-1, 0].astype(np.int64) + nb <= N // 2 + 1).all() and checked_bands(spec, bands)[1] == 0
    assert (tab[2 * N:] > 0).all()  # the zero weights are dropped
    assert_weights_are_htk(spec, tab, bands, sr, f_min, f_max if f_max else None)


def test_design_sizing_and_refusals():
    L = libflac.load()
    s = libflac.MelSpec()
    tab = np.full(4096, CANARY, np.uint32)
    bnd = np.full(600, CANARY, np.uint32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    # zero caps size the tables and fill the spec; nothing is written
    need = L.bnflac_mel_design(48000, 1024, 256, 128, 0.0, 0.0, ctypes.byref(s), None, 0, None, 0)
    assert need == 2 * 1024 + s.n_weights and (s.n_fft, s.hop, s.n_mels, s.origin) == (1024, 256, 128, -512) and s.n_weights > 128
    # a short cap of either table: the size comes back, nothing is written
    assert L.bnflac_mel_design(48000, 1024, 256, 128, 0.0, 0.0, ctypes.byref(s), vp(tab), need - 1, vp(bnd), 600) == need
    assert L.bnflac_mel_design(48000, 1024, 256, 128, 0.0, 0.0, ctypes.byref(s), vp(tab), 4096, vp(bnd), 257) == need
    assert (tab == CANARY).all() and (bnd == CANARY).all()
    assert L.bnflac_mel_design(48000, 1024, 256, 128, 0.0, 0.0, ctypes.byref(s), vp(tab), 4096, vp(bnd), 258) == need
    assert (tab[:need] != CANARY).all() and (tab[need:] == CANARY).all() and (bnd[:258] != CANARY).all() and (bnd[258:] == CANARY).all()
    # n_mels 0 needs no bands
    assert L.bnflac_mel_design(48000, 64, 1, 0, 0.0, 0.0, ctypes.byref(s), vp(tab), 128, None, 0) == 128 and s.n_weights == 0
    with pytest.raises(RuntimeError, match=r"n_mels = 300 and n_weights = \d+ \(n_mels <= 256, n_weights <= 8192\)"):
        libflac.mel_design(48000, 1024, 256, 300)
    for args, word in (((0, 1024, 256, 40, 0.0, 0.0), b"sample_rate"), ((48000, 1000, 256, 40, 0.0, 0.0), b"power of two"),
                       ((48000, 32, 256, 40, 0.0, 0.0), b"power of two"), ((48000, 4096, 256, 40, 0.0, 0.0), b"power of two"),
                       ((48000, 1024, 0, 40, 0.0, 0.0), b"hop"), ((48000, 1024, 65536, 40, 0.0, 0.0), b"hop"),
                       ((48000, 1024, 256, 40, 100.0, 50.0), b"f_min"), ((48000, 1024, 256, 40, 0.0, 30000.0), b"f_min"),
                       ((48000, 1024, 256, 40, -1.0, 0.0), b"f_min")):
        assert L.bnflac_mel_design(*args, ctypes.byref(s), vp(tab), 4096, vp(bnd), 600) < 0 and word in L.bnflac_last_error(), args
    assert L.bnflac_mel_design(48000, 1024, 256, 40, 0.0, 0.0, None, vp(tab), 4096, vp(bnd), 600) < 0 and b"null" in L.bnflac_last_error()
    for bad in (libflac.MelSpec(100, 1, 0, 0, 0), libflac.MelSpec(64, 0, 0, 0, 0)):
        with pytest.raises(RuntimeError):
            libflac.mel_request(bad, 0, 10)
    with pytest.raises(RuntimeError, match="2\\^31"):
        libflac.mel_request(libflac.MelSpec(64, 1, 0, 0, 0), 1 << 31, 1)


# ------------------------------------------------------------------ edges
def test_edges_of_windows_origins_and_rows():
    """n < n_fft, n == 0, origin positive and past the window, origin below -n_fft; row_frames 0, 1,
    above and below n_valid; frame_pitch > row_frames (canaries); a bad window."""
    d, tab, bands = design(48000, 128, 48, 12)
    fmt, sp, stride, unit = layout("OUT_FILEREADER", 2, 24)
    nsmp = 700
    pcm = np.random.default_rng(4).integers(1, 256, nsmp * stride + 2, dtype=np.uint8)
    win = window_table([(3, 0), (5, 1), (0, 127), (9, 128), (1, 600), (U64, 1), (nsmp - 100, 100), (nsmp - 100, 101)])
    seen = set()
    for origin in (-64, 0, 31, 200, 650, -128, -129, -1000, 2 ** 31 - 1, -2 ** 31):
        spec = d.with_origin(origin)
        nvs = [n_valid_of(int(w["nsamples"]), spec) for w in win[[0, 1, 2, 3, 4, 6]]]
        for R in (0, 1, 5, 13, 40):
            for flags in (0, MONO):
                rc, got, st = call_mel_host(pcm, fmt, sp, win, spec, tab, bands, R, R + 3, flags)
                ref = ref_mel(pcm, fmt, sp, win, spec, tab, bands, R, R + 3, flags)
                assert rc == 0 and st == ref[3], (origin, R, st, ref[3])
                assert st[:2] == [1, 2] and st[2] == sum(nv > R for nv in nvs) and st[3] == 0
                assert_within(got, ref, "origin %d R %d flags %d" % (origin, R, flags))
                seen.add((st[2] > 0, any(0 < nv <= R for nv in nvs)))
    assert seen == {(True, False), (True, True), (False, True), (False, False)}  # rows cut, rows with zeros behind, neither


def test_bad_bands_are_empty_and_counted_once():
    """Bands that descend, run past n_weights or past the last bin: a +0.0f row, counted once per
    launch whatever the number of windows and frames, and nothing outside the tables is read (the
    tables are allocated exactly; the sanitizer program runs the same tables)."""
    d, tab, bands = design(48000, 128, 32, 8)
    fmt, sp, stride, unit = layout("OUT_FLACDECODER", 2, 16)
    pcm = random_pcm(np.random.default_rng(8), 900 * stride, unit, 16)
    win = window_table([(0, 500), (7, 800)])
    b = bands.copy()
    b[2, 1] = b[3, 1] + 1       # band 1's end (2's start) behind band 2's end: band 2 descends, band 1 overlaps (fine if inside)
    b[5, 0] = 65 - 1            # band 5 starts at the last bin: runs past N/2 + 1 if it has two bins or more
    b[8, 1] = d.n_weights + 1   # the last prefix past n_weights: band 7 is bad
    spec = libflac.MelSpec(128, 32, 8, -64, d.n_weights)
    chk, nbad = checked_bands(spec, b)
    assert nbad >= 3 and chk[2][2] == 0 and chk[5][2] == 0 and chk[7][2] == 0
    for R in (3, 40):
        rc, got, st = call_mel_host(pcm, fmt, sp, win, spec, tab, b, R, R, 0)
        ref = ref_mel(pcm, fmt, sp, win, spec, tab, b, R, R, 0)
        assert rc == 0 and st == ref[3] == [2, 0, st[2], nbad]
        assert_within(got, ref, "bad bands")
        rows = got.reshape(2, 2, 8, R)
        assert not rows[:, :, [2, 5, 7], :].any() and rows[:, :, 0, 0].all()
    huge = np.full_like(b, 0xFFFFFFFF)
    rc, got, st = call_mel_host(pcm, fmt, sp, win, spec, tab, huge, 5, 5, 0)
    assert rc == 0 and st == [2, 0, 2, 8] and not got.any()  # every prefix past n_weights
    huge[:, 1] = np.arange(9, dtype=np.uint32)[::-1] * 1000  # and descending
    rc, got, st = call_mel_host(pcm, fmt, sp, win, spec, tab, huge, 5, 5, 0)
    assert rc == 0 and st == [2, 0, 2, 8] and not got.any()
    rc, got, st = call_mel_host(pcm, fmt, sp, win[:0], spec, tab, huge, 5, 5, 0)  # no windows: zeros
    assert rc == 0 and st == [0, 0, 0, 0]


# ------------------------------------------------------------------ refusals of the gather
def test_gather_refusals():
    fmt, sp, stride, unit = layout("OUT_FILEREADER", 2, 24)
    R, nsmp = 20, 900
    pcm = np.random.default_rng(4).integers(1, 256, nsmp * stride + 2, dtype=np.uint8)
    win = window_table([(0, 10), (5, 800), (U64, 1)])
    good, tab, bands = design(48000, 64, 16, 8)
    L = libflac.load()
    big = np.zeros(2 * 2048 + 8192 + 64, np.float32)
    bigb = np.zeros(2 * 258, np.uint32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    S = lambda n_fft=64, hop=16, n_mels=8, origin=-32, n_weights=good.n_weights, reserved=(0, 0, 0): libflac.MelSpec(
        n_fft, hop, n_mels, origin, n_weights, (ctypes.c_uint32 * 3)(*reserved))

    def refused(word, fmt=fmt, sp=sp, R=R, pitch=R, flags=0, n=len(win), spec=good):
        out = np.full(4096, CANARY, np.uint32)  # a refused call writes nothing
        status = np.full(4, 0xA5A5A5A5, np.uint32)
        rc = L.bnflac_gather_ranges_mel_host(vp(padded(pcm)), len(pcm), fmt, ctypes.byref(sp), vp(win), n, ctypes.byref(spec),
                                             vp(big), vp(bigb), R, pitch, flags, vp(out), vp(status))
        assert rc < 0 and word in L.bnflac_last_error(), (word, rc, L.bnflac_last_error())
        assert (out == CANARY).all() and (status == 0xA5A5A5A5).all()

    for n_fft in (0, 32, 63, 96, 4096, 1 << 31):
        refused(b"power of two", spec=S(n_fft=n_fft))
    refused(b"hop", spec=S(hop=0))
    refused(b"hop", spec=S(hop=65536))
    refused(b"n_mels", spec=S(n_mels=257))
    refused(b"n_weights", spec=S(n_weights=8193))
    refused(b"n_weights", spec=S(n_mels=0, n_weights=1))
    for k in range(3):
        refused(b"reserved", spec=S(reserved=[1 if j == k else 0 for j in range(3)]))
    refused(b"row_frames", R=1 << 31, pitch=1 << 31)
    refused(b"frame_pitch", pitch=R - 1)
    refused(b"PLANAR32", fmt=libflac.OUT_PLANAR32)
    refused(b"bnflac_md5_layout", fmt=libflac.OUT_FLACDECODER)
    refused(b"bnflac_md5_layout", fmt=libflac.OUT_FILEREADER, sp=params(2, 20))
    refused(b"out_format", fmt=7)
    refused(b"channels", sp=params(0, 24))
    refused(b"channels", fmt=libflac.OUT_INTERLEAVED32, sp=params(9, 24))
    refused(b"flags", flags=2)
    refused(b"flags", flags=MONO | 0x80000000)
    refused(b"too many streams", n=1 << 30)
    out, status, buf = np.zeros(3 * 2 * 8 * R, np.float32), np.zeros(4, np.uint32), padded(pcm)
    args = lambda **kw: [kw.get("pcm", vp(buf)), len(pcm), fmt, kw.get("sp", ctypes.byref(sp)), kw.get("win", vp(win)), len(win),
                         kw.get("spec", ctypes.byref(good)), kw.get("tab", vp(big)), kw.get("bands", vp(bigb)), R, R, 0,
                         kw.get("out", vp(out)), kw.get("status", vp(status))]
    for kw in ({"pcm": None}, {"sp": None}, {"win": None}, {"out": None}, {"status": None}, {"spec": None}, {"tab": None},
               {"bands": None}):
        assert L.bnflac_gather_ranges_mel_host(*args(**kw)) == -1 and b"null" in L.bnflac_last_error(), kw
    assert L.bnflac_gather_ranges_mel_host(*args()) == 0 and status.tolist() == [1, 1, 1, 0]
    # null bands are taken with n_mels == 0; the limits themselves are taken
    nomel = S(n_mels=0, n_weights=0)
    out0 = np.zeros(3 * 2 * 33 * R, np.float32)
    assert L.bnflac_gather_ranges_mel_host(*args(spec=ctypes.byref(nomel), bands=None, out=vp(out0))) == 0
    for spec in (S(n_fft=2048, hop=65535, n_mels=256, n_weights=8192), S(n_fft=64, hop=1, n_mels=1, n_weights=0)):
        outb = np.zeros(3 * 2 * 256 * R, np.float32)
        assert L.bnflac_gather_ranges_mel_host(*args(spec=ctypes.byref(spec), out=vp(outb))) == 0, L.bnflac_last_error()
    rc, got, st = call_mel_host(pcm, fmt, sp, win[:0], good, tab, bands, R, R, 0)
    assert rc == 0 and st == [0, 0, 0, 0] and got.size == 0
    rc, got, st = call_mel_host(pcm, fmt, sp, win, good, tab, bands, 0, 3, 0)  # row_frames 0: nothing written, the windows still counted
    assert rc == 0 and st == [1, 1, 2, 0] and (got == CANARY).all()


# ------------------------------------------------------------------ the rule under the sanitizers
@pytest.mark.skipif(_cxx() is None, reason="no C++ compiler")
def test_rule_under_asan_ubsan(tmp_path):
    """A program of its own (tools/gather_mel_sanitize.cpp), run directly: nothing is loaded into
    Python."""
    exe = str(tmp_path / "gather_mel_sanitize")
    cmd = [_cxx(), "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "birdnest", "audio_amd", "csrc"), os.path.join(ROOT, "tools", "gather_mel_sanitize.cpp"),
           "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and re.search(r"cannot find .*(asan|ubsan)|lib(clang_rt\.)?(asan|ubsan)[^ ]*: No such file", built.stderr):
        pytest.skip("the compiler lacks the sanitizer runtimes")
    assert built.returncode == 0, built.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "gather_mel_sanitize: ok" in r.stdout
