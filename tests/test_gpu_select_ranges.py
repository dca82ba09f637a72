"""bnflac_select_ranges / bnflac_gather_ranges: one sample window per stream of a batch.

References, all independent of the code under test: `ref_select` (the rule in Python) and
bnflac_select_ranges_host on the fabricated tables of tests/test_select_ranges_host.py; the
generator's PCM for the whole chain; a whole-batch decode_parsed of the unselected index for the
packed layouts; numpy slicing for the gather alone.  Every comparison is exact.
"""
import ctypes
import math

import numpy as np
import pytest

from tests.conftest import gpu_available
from tests.test_gpu_index_streams import Batch, _first_frame_offset, _mixed, _pack, _stream_params, _upload
from tests.test_select_ranges_host import (BAD_TABLES, CANARY, KINDS, MIXED, OVERFLOW, U64, WINDOW_FIELDS, assert_same,
                                           call_host, fabricate, filler, ref_select, windows_by_kind)

pytestmark = pytest.mark.gpu

POISON = 0x5A
DEV = "cuda:0"


@pytest.fixture(scope="module")
def gpu():
    if not gpu_available():
        pytest.skip("no GPU")
    import torch
    from birdnest.audio_amd import libflac
    return torch, libflac, libflac.BatchDecoder(0)


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _dev(torch, a):
    """a numpy array's bytes on the device, 8-byte typed where it is"""
    a = np.ascontiguousarray(a)
    if a.size == 0:
        return torch.zeros(16, dtype=torch.uint8, device=DEV)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(DEV)


def call_device(gpu, info, cap, sf, ss, ranges, sel_cap, offsets=None):
    """bnflac_select_ranges itself on uploaded tables; every output one entry longer than the
    contract says, the extra entry a canary -> (call_host's shape, sel_offsets or None)"""
    torch, libflac, dec = gpu
    n = len(sf) - 1
    d_info = _dev(torch, info)
    d_sf, d_ss = _dev(torch, np.asarray(sf, np.uint32)), _dev(torch, np.asarray(ss, np.uint64))
    d_r = _dev(torch, libflac.sample_ranges(ranges))
    d_offs = _dev(torch, np.asarray(offsets, np.uint64)) if offsets is not None else None
    d_sel = torch.full(((sel_cap + 1) * 128,), CANARY, dtype=torch.uint8, device=DEV)
    d_sel_o = torch.full(((sel_cap + 1) * 8,), CANARY, dtype=torch.uint8, device=DEV)
    d_sel_f = torch.full(((n + 2) * 4,), CANARY, dtype=torch.uint8, device=DEV)
    d_sel_s = torch.full(((n + 2) * 8,), CANARY, dtype=torch.uint8, device=DEV)
    d_win = torch.full(((n + 1) * 32,), CANARY, dtype=torch.uint8, device=DEV)
    d_st = torch.full((5 * 4,), CANARY, dtype=torch.uint8, device=DEV)
    rc = dec.L.bnflac_select_ranges(dec.ctx, _vp(d_offs), _vp(d_info), cap, _vp(d_sf), _vp(d_ss), n, _vp(d_r),
                                    _vp(d_sel_o) if offsets is not None else None, _vp(d_sel), sel_cap, _vp(d_sel_f),
                                    _vp(d_sel_s), _vp(d_win), _vp(d_st),
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, dec.L.bnflac_last_error()
    torch.cuda.synchronize()
    sel, sel_o, sel_f, sel_s, win, st = (t.cpu().numpy() for t in (d_sel, d_sel_o, d_sel_f, d_sel_s, d_win, d_st))
    assert (sel[sel_cap * 128:] == CANARY).all(), "a record was written at sel_cap"
    assert (sel_o[sel_cap * 8:] == CANARY).all(), "an offset was written at sel_cap"
    assert (sel_f[(n + 1) * 4:] == CANARY).all() and (sel_s[(n + 1) * 8:] == CANARY).all()
    assert (win[n * 32:] == CANARY).all() and (st[16:] == CANARY).all()
    w = libflac.window_array(win[: n * 32])
    out = (libflac.info_array(sel[: sel_cap * 128]), sel_f[: (n + 1) * 4].view("<u4").tolist(),
           sel_s[: (n + 1) * 8].view("<u8").tolist(), [tuple(int(x[f]) for f in WINDOW_FIELDS) for x in w],
           st[:16].view("<u4").tolist())
    return out, (sel_o[: sel_cap * 8].view("<u8") if offsets is not None else None)


# ------------------------------------------------------------------ 1. device = host = Python
def _three_way(gpu, info, cap, sf, ss, ranges, sel_cap, offsets=None):
    want = ref_select(info, cap, sf, ss, ranges, sel_cap)
    assert_same(call_host(info, cap, sf, ss, ranges, sel_cap), want)
    got, sel_o = call_device(gpu, info, cap, sf, ss, ranges, sel_cap, offsets)
    assert_same(got, want)
    return got, sel_o


@pytest.mark.parametrize("shift", [0, 7])
def test_device_host_python_mixed(gpu, shift):
    """16 streams of 0, 1 and many frames; the two passes give each stream two kinds of window,
    and each pass holds every kind.  With offsets: d_sel_offsets follows the records."""
    info, sf, ss = fabricate(MIXED, seed=1)
    cap = len(info)
    assert len(MIXED) >= len(KINDS)
    ranges = windows_by_kind(info, sf, ss, shift)
    offsets = np.arange(cap, dtype=np.uint64) * 1000 + 7
    got, sel_o = _three_way(gpu, info, cap, sf, ss, ranges, cap + 3, offsets)
    want_o = np.zeros(cap + 3, np.uint64)
    for s, w in enumerate(got[3]):
        want_o[got[1][s]:got[1][s + 1]] = offsets[w[3]:w[3] + w[4]]
    assert np.array_equal(sel_o, want_o)


@pytest.mark.parametrize("nstreams", [0, 1, 1025])
def test_device_host_python_stream_counts(gpu, nstreams):
    """1025 streams: the prefixes cross the 1,024-stream workgroup of the scan."""
    rng = np.random.default_rng(nstreams)
    info, sf, ss = fabricate([int(x) for x in rng.integers(0, 6, nstreams)], seed=3 + nstreams)
    cap = len(info)
    ranges = []
    for s in range(nstreams):
        T = int(ss[s + 1]) - int(ss[s])
        ranges.append((int(rng.integers(0, T + 3)), int(rng.integers(0, T + 3))))
    got, _ = _three_way(gpu, info, cap, sf, ss, ranges, cap + 2)
    if nstreams == 1025:
        assert got[1][1024] > 0 and got[1][1025] >= got[1][1024]


def test_device_status_cases(gpu):
    """sel_cap one short (bit 0), the index's total above cap and descending tables (bit 1)."""
    info, sf, ss = fabricate(MIXED, seed=1)
    cap, n = len(info), len(MIXED)
    ranges = windows_by_kind(info, sf, ss, 10)
    total = ref_select(info, cap, sf, ss, ranges, cap)[4][1]
    got, _ = _three_way(gpu, info, cap, sf, ss, ranges, total - 1)
    assert got[4][0] == OVERFLOW and got[4][1] == total
    _three_way(gpu, info, cap, sf, ss, ranges, 0)
    everything = [(0, U64)] * n
    for cap2, sf2, ss2 in ((cap - 1, sf, ss),
                           (cap, np.concatenate([sf[:5], [sf[6], sf[5]], sf[7:]]).astype(np.uint32), ss),
                           (cap, sf, np.concatenate([ss[:9], [ss[8] - 1], ss[10:]]).astype(np.uint64))):
        got, _ = _three_way(gpu, info, cap2, sf2, ss2, everything, 24)
        assert got[4] == [BAD_TABLES, 0, 0, 0] and got[0].tobytes() == filler(24).tobytes()


def test_device_out_sample_values_no_index_wrote(gpu):
    """Non-monotone out_sample: the device call returns and agrees with the host twin."""
    rng = np.random.default_rng(9)
    info, sf, ss = fabricate((9, 1, 30, 0, 5, 64), seed=200)
    cap = len(info)
    info["out_sample"] = rng.integers(0, 20000, cap, dtype=np.uint64)
    ranges = [(int(rng.integers(0, 9000)), int(rng.integers(0, 9000))) for _ in range(len(sf) - 1)]
    got, _ = call_device(gpu, info, cap, sf, ss, ranges, cap)
    assert_same(got, call_host(info, cap, sf, ss, ranges, cap))


# ------------------------------------------------------------------ 2. end to end against the generator
_BATCHES = {}


def _batch(gpu, name):
    """name -> (Batch of the index, the streams' PCM or None, sp); computed once.  C2: the five
    streams of tests/test_gpu_index_streams.py (12, 1, 7, 0 and 3 frames; gaps of filler sync
    bytes, an odd begin, an empty stream); C4 / C3 / C5: three streams of 40 / 16 / 8 frames."""
    if name not in _BATCHES:
        from birdnest.audio_amd import synth
        torch, libflac, dec = gpu
        if name == "C2":
            m = _mixed(gpu)
            syn, buf, table, sp = m["syn"], m["buf"], m["table"], m["sp"]
        else:
            nf = {"C4": 40, "C3": 16, "C5": 8}[name]
            syn = [synth.encode(synth.config(name, nframes=nf, seed=5 + 100 * i)) for i in range(3)]
            datas = [s.data.tobytes() for s in syn]
            buf, ranges = _pack(datas, (3, 0))
            table = [(b, e, b + _first_frame_offset(d), _stream_params(libflac, d).total_samples)
                     for (b, e), d in zip(ranges, datas)]
            sp = _stream_params(libflac, datas[0], 0)
        b = Batch(gpu, buf, table, sp)
        assert b.status[0] == 0
        pristine = b.d_info.clone()  # decode_parsed completes records in place: selections start from this copy
        _BATCHES[name] = (b, pristine, [s.pcm if s is not None else None for s in syn], sp, len(buf))
    return _BATCHES[name]


def _select(gpu, b, pristine, ranges, sel_cap):
    torch, libflac, dec = gpu
    n = len(b.sf) - 1
    d_sf = torch.from_numpy(b.sf.astype(np.int32)).to(DEV)
    d_ss = torch.from_numpy(b.ss.astype(np.int64)).to(DEV)
    return dec.select_ranges(b.d_offs, pristine.clone(), b.cap, d_sf, d_ss, n, ranges, sel_cap)


def _windows_of_batch(b, shift):
    info = np.zeros(len(b.rec), dtype=b.rec.dtype)
    info["out_sample"], info["blocksize"] = b.rec["out_sample"], b.rec["blocksize"]
    return windows_by_kind(info, b.sf, b.ss, shift)


@pytest.mark.parametrize("name", ["C2", "C4", "C3", "C5"])
def test_chain_against_the_generator(gpu, name):
    torch, libflac, dec = gpu
    b, pristine, pcms, sp, nbytes = _batch(gpu, name)
    n, total = len(b.sf) - 1, int(b.sf[-1])
    sel_cap = total + 4
    stride = 4 * sp.channels
    passes = (0, 5, 10) if name == "C2" else (0, 3, 6, 9)  # 5 streams x 3 passes, 3 streams x 4 passes: every kind
    assert {(s + shift) % len(KINDS) for s in range(n) for shift in passes} == set(range(len(KINDS)))
    for shift in passes:
        ranges = _windows_of_batch(b, shift)
        d_sel_offs, d_sel_info, d_sel_f, d_sel_s, d_win, d_st = _select(gpu, b, pristine, ranges, sel_cap)
        st = d_st.cpu().numpy()
        sel_f, sel_s = d_sel_f.cpu().numpy(), d_sel_s.cpu().numpy()
        win = libflac.window_array(d_win.cpu().numpy())
        assert st[0] == 0 and st[1] == sel_f[-1] <= total
        before = libflac.info_array(d_sel_info.cpu().numpy())
        pcm_bytes = (int(sel_s[-1]) * stride + 15) // 16 * 16 + 64
        d_pcm = torch.full((pcm_bytes,), POISON, dtype=torch.uint8, device=DEV)
        dec.decode_parsed(b.d_bytes, nbytes, sel_cap, sp, libflac.OUT_INTERLEAVED32, d_pcm, d_sel_info)
        R = max(1, max(int(w["nsamples"]) for w in win)) + 3
        d_rows, d_gst = dec.gather_ranges(d_pcm, libflac.OUT_INTERLEAVED32, sp, d_win, n, R)
        torch.cuda.synchronize()
        after = libflac.info_array(d_sel_info.cpu().numpy())
        nsel = int(sel_f[-1])
        assert (after["status"][:nsel] == 0).all() and (after["crc_ok"][:nsel] == 1).all()
        assert after[nsel:].tobytes() == before[nsel:].tobytes() == filler(sel_cap - nsel).tobytes()
        pcm = d_pcm.cpu().numpy()
        assert (pcm[int(sel_s[-1]) * stride:] == POISON).all(), "the decode wrote past the last selected sample"
        rows = d_rows.cpu().numpy().view("<i4").reshape(n, R, sp.channels)
        assert d_gst.cpu().numpy().tolist() == [0, 0, 0, 0]
        for s in range(n):
            first, want = ranges[s]
            T = len(pcms[s]) if pcms[s] is not None else 0
            lo = min(first, T)
            hi = min(lo + want, T)
            assert int(win["nsamples"][s]) == hi - lo
            if hi > lo:
                assert np.array_equal(rows[s, : hi - lo], pcms[s][lo:hi]), (name, shift, s)
            assert not rows[s, hi - lo:].any(), (name, shift, s)


# ------------------------------------------------------------------ 3. the packed layouts against the full decode
@pytest.mark.parametrize("name,fmt_name", [("C2", "OUT_FLACDECODER"), ("C3", "OUT_FILEREADER")])
def test_packed_layouts_against_the_full_decode(gpu, name, fmt_name):
    torch, libflac, dec = gpu
    fmt = getattr(libflac, fmt_name)
    b, pristine, pcms, sp, nbytes = _batch(gpu, name)
    n, total = len(b.sf) - 1, int(b.sf[-1])
    stride = libflac.out_stride(fmt, sp)
    assert stride == (4 if name == "C2" else 6)
    d_full = torch.zeros((int(b.ss[-1]) * stride + 15) // 16 * 16, dtype=torch.uint8, device=DEV)
    full_info = pristine.clone()
    dec.decode_parsed(b.d_bytes, nbytes, total, sp, fmt, d_full, full_info)  # the reference: every frame, today's path
    torch.cuda.synchronize()
    rec = libflac.info_array(full_info[: total * 128].cpu().numpy())
    assert (rec["status"] == 0).all() and (rec["crc_ok"] == 1).all()
    full = d_full.cpu().numpy()
    sel_cap = total + 2
    for shift in (0, 1, 3):
        ranges = _windows_of_batch(b, shift)
        _, d_sel_info, d_sel_f, d_sel_s, d_win, d_st = _select(gpu, b, pristine, ranges, sel_cap)
        hull = int(d_sel_s.cpu().numpy()[-1])
        d_pcm = torch.full(((hull * stride + 15) // 16 * 16 + 16,), POISON, dtype=torch.uint8, device=DEV)
        dec.decode_parsed(b.d_bytes, nbytes, sel_cap, sp, fmt, d_pcm, d_sel_info)
        win = libflac.window_array(d_win.cpu().numpy())
        R = max(1, max(int(w["nsamples"]) for w in win)) + 1
        d_rows, d_gst = dec.gather_ranges(d_pcm, fmt, sp, d_win, n, R, row_bytes=R * stride + 5)
        torch.cuda.synchronize()
        assert d_gst.cpu().numpy().tolist() == [0, 0, 0, 0]
        rows = d_rows.cpu().numpy()
        for s in range(n):
            T = int(b.ss[s + 1] - b.ss[s])
            lo = min(ranges[s][0], T)
            hi = min(lo + ranges[s][1], T)
            row = rows[s * (R * stride + 5):][: R * stride]
            src = (int(b.ss[s]) + lo) * stride
            assert np.array_equal(row[: (hi - lo) * stride], full[src: src + (hi - lo) * stride]), (shift, s)
            assert not row[(hi - lo) * stride:].any(), (shift, s)


# ------------------------------------------------------------------ 4. the gather alone
def _layouts(libflac):
    """(fmt, sp) pairs with strides 2, 3, 4, 6, 8 and 32"""
    sp = lambda ch, bps: libflac.StreamParams(1, 4096, 4096, 44100, ch, bps, 0)
    return [(libflac.OUT_FLACDECODER, sp(1, 16), 2), (libflac.OUT_FILEREADER, sp(1, 24), 3),
            (libflac.OUT_FLACDECODER, sp(2, 16), 4), (libflac.OUT_FILEREADER, sp(2, 24), 6),
            (libflac.OUT_INTERLEAVED32, sp(2, 16), 8), (libflac.OUT_INTERLEAVED32, sp(8, 24), 32)]


def _raw_gather(gpu, d_pcm, pcm_bytes, fmt, sp, win, R, row_bytes, d_rows):
    torch, libflac, dec = gpu
    d_win = _dev(torch, win)
    d_st = torch.full((4,), POISON, dtype=torch.int32, device=DEV)
    rc = dec.L.bnflac_gather_ranges(dec.ctx, _vp(d_pcm), pcm_bytes, fmt, ctypes.byref(sp), _vp(d_win), len(win), R,
                                    row_bytes, _vp(d_rows), _vp(d_st),
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, d_st.cpu().numpy().tolist()


@pytest.mark.parametrize("R", [1, 1000])
def test_gather_alignment_sweep(gpu, R):
    """Every source phase the stride allows x every destination phase x every length class, the
    pad bytes between rows and a canary behind the last row untouched."""
    torch, libflac, dec = gpu
    rng = np.random.default_rng(R)
    for fmt, sp, stride in _layouts(libflac):
        assert libflac.out_stride(fmt, sp) == stride
        n16 = 16 // math.gcd(16, stride)  # samples that fill whole 16-byte blocks exactly
        lengths = sorted({0, 1, 5, n16, R - 1, R, R + 3})
        nsmp = 16 + max(lengths) + 8  # sample frames of the PCM: every window lies inside
        pcm_bytes = nsmp * stride
        pcm = rng.integers(0, 256, (pcm_bytes + 15) // 16 * 16, dtype=np.uint8)
        d_pcm = torch.from_numpy(pcm).to(DEV)
        win = np.zeros(16 * len(lengths), dtype=libflac.WINDOW_DTYPE)
        for k in range(len(win)):
            win[k] = (1 + k % 16, lengths[k // 16], 0, 0, 0, 0)
        assert {int(w["pcm_first"]) * stride % 16 for w in win} == {p * stride % 16 for p in range(16)}
        W = R * stride
        for extra in (1, 7):
            row_bytes = W + extra + (W + extra + 1) % 2  # odd: 16 consecutive rows take every phase
            assert {s * row_bytes % 16 for s in range(len(win))} == set(range(16))
            want = np.full(len(win) * row_bytes + 64, POISON, np.uint8)
            for s, w in enumerate(win):
                ncopy = min(int(w["nsamples"]), R) * stride
                src = int(w["pcm_first"]) * stride
                want[s * row_bytes: s * row_bytes + ncopy] = pcm[src: src + ncopy]
                want[s * row_bytes + ncopy: s * row_bytes + W] = 0
            d_rows = torch.full((len(want),), POISON, dtype=torch.uint8, device=DEV)
            rc, st = _raw_gather(gpu, d_pcm, pcm_bytes, fmt, sp, win, R, row_bytes, d_rows)
            assert rc == 0, dec.L.bnflac_last_error()
            assert st == [0, 0, sum(1 for w in win if w["nsamples"] > R), 0]
            got = d_rows.cpu().numpy()
            if not np.array_equal(got, want):
                bad = int(np.flatnonzero(got != want)[0])
                raise AssertionError("stride %d R %d row_bytes %d: row %d byte %d" % (stride, R, row_bytes, bad // row_bytes,
                                                                                    bad % row_bytes))


def test_gather_window_past_the_pcm_and_refusals(gpu):
    torch, libflac, dec = gpu
    fmt, sp, stride = _layouts(libflac)[3]
    rng = np.random.default_rng(4)
    nsmp, R = 50, 20
    pcm_bytes = nsmp * stride + 2  # a partial sample frame at the end does not count
    pcm = rng.integers(1, 256, (pcm_bytes + 15) // 16 * 16, dtype=np.uint8)
    d_pcm = torch.from_numpy(pcm).to(DEV)
    win = np.zeros(4, dtype=libflac.WINDOW_DTYPE)
    win[0] = (nsmp - 10, 10, 0, 0, 0, 0)  # ends exactly at the last whole sample frame
    win[1] = (nsmp - 10, 11, 0, 0, 0, 0)  # one sample past it
    win[2] = (U64, 1, 0, 0, 0, 0)
    win[3] = (U64, 0, 0, 0, 0, 2)         # empty: nothing is read, whatever pcm_first says
    row_bytes = R * stride
    d_rows = torch.full((4 * row_bytes + 16,), POISON, dtype=torch.uint8, device=DEV)
    rc, st = _raw_gather(gpu, d_pcm, pcm_bytes, fmt, sp, win, R, row_bytes, d_rows)
    assert rc == 0 and st == [1, 2, 0, 0]
    got = d_rows.cpu().numpy()
    assert np.array_equal(got[: 10 * stride], pcm[(nsmp - 10) * stride: nsmp * stride])
    assert not got[10 * stride: 4 * row_bytes].any() and (got[4 * row_bytes:] == POISON).all()
    # refusals: a negative return and a message, nothing launched
    d_rows.fill_(POISON)
    rc, st = _raw_gather(gpu, d_pcm, pcm_bytes, libflac.OUT_PLANAR32, sp, win, R, 4 * sp.channels * R, d_rows)
    assert rc < 0 and b"PLANAR32" in dec.L.bnflac_last_error() and st == [POISON] * 4
    rc, st = _raw_gather(gpu, d_pcm, pcm_bytes, fmt, sp, win, R, R * stride - 1, d_rows)
    assert rc < 0 and b"row_bytes" in dec.L.bnflac_last_error() and st == [POISON] * 4
    assert (d_rows.cpu().numpy() == POISON).all()


# ------------------------------------------------------------------ 5. decode_windows: the chain, not waited for
def test_decode_windows_returns_before_earlier_work_is_done(gpu):
    """decode_windows on the C2 files behind about 26 TFLOP of matrix products queued on the same
    stream (a few hundred milliseconds; a warm decode_windows call takes the host a few): when it
    returns, the products' end event has not happened yet, so no step of the chain waited for
    the stream.  No time is measured or compared."""
    torch, libflac, dec = gpu
    m = _mixed(gpu)
    d_bytes = _upload(torch, m["buf"])
    files = [(t[0], t[1]) for t in m["table"]]
    sp = _stream_params(libflac, m["datas"][0], 0)
    n = 3000
    firsts = [4096 * 3 - 7, 100, 4096 * 6 + 1, 0, 5000]
    d_files = torch.tensor([[b, e, 0, 0] for b, e in files], dtype=torch.int64, device=DEV).reshape(-1)
    d_windows = torch.tensor([[f, n] for f in firsts], dtype=torch.int64, device=DEV).reshape(-1)
    call = lambda: dec.decode_windows(d_bytes, len(m["buf"]), d_files.clone(), d_windows, n, sp, libflac.OUT_INTERLEAVED32)
    call()  # the context's scratch and the allocator's blocks exist from here on
    a = torch.randn(8192, 8192, device=DEV)
    c = torch.empty_like(a)
    torch.mm(a, a, out=c)
    torch.cuda.synchronize()
    done = torch.cuda.Event()
    for _ in range(24):
        torch.mm(a, a, out=c)
    done.record()
    rows, status = call()
    still_busy = not done.query()
    torch.cuda.synchronize()
    assert still_busy, "decode_windows returned only after the work queued in front of it had finished"
    assert status["scan"].cpu().numpy().tolist() == [1, 4, 1, 0]  # the empty stream has no marker
    assert status["index"].cpu().numpy()[0] == 0 and status["gather"].cpu().numpy().tolist() == [0, 0, 0, 0]
    st = status["select"].cpu().numpy().tolist()
    assert st[0] == 0 and st[2] == 4
    got = rows.cpu().numpy()
    assert got.shape == (5, n, sp.channels)
    for s, (syn, first) in enumerate(zip(m["syn"], firsts)):
        T = len(syn.pcm) if syn is not None else 0
        lo, hi = min(first, T), min(first + n, T)
        if hi > lo:
            assert np.array_equal(got[s, : hi - lo], syn.pcm[lo:hi]), s
        assert not got[s, hi - lo:].any(), s
    # the frames decoded are the ones the windows touch, not the batch's 23
    want_frames = sum(len({(x // 4096) for x in (min(f, len(y.pcm)), min(f + n, len(y.pcm)) - 1)})
                      for y, f in zip(m["syn"], firsts) if y is not None and f < len(y.pcm))
    assert st[1] == want_frames < 23
