"""bnflac_select_windows: any crops of an indexed batch, one output row per request.

References, all independent of the code under test: `ref_windows` (the rule in Python) and
bnflac_select_windows_host on the fabricated tables and request sets of
tests/test_select_windows_host.py; the device's own bnflac_select_ranges for identity requests;
the generator's PCM for the whole chain; bnflac_gather_ranges_f32_host for the float planes.
Every comparison is exact.
"""
import ctypes

import numpy as np
import pytest

from tests.conftest import gpu_available
from tests.test_gpu_index_streams import _mixed, _stream_params, _upload
from tests.test_gpu_select_ranges import _batch, _dev, _vp, call_device
from tests.test_select_ranges_host import (BAD_TABLES, CANARY, EMPTY, KINDS, MIXED, OVERFLOW, U64, WINDOW_FIELDS,
                                           assert_same, fabricate, filler, windows_by_kind)
from tests.test_select_windows_host import (NO_STREAM, assert_saturated, bad_ids, bad_slice_tables, call_host_windows,
                                            every_kind_on_every_stream, ref_windows, saturation_case,
                                            three_on_the_long_stream)

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


def call_device_windows(gpu, info, cap, sf, ss, reqs, sel_cap, offsets=None):
    """bnflac_select_windows itself on uploaded tables; every output one entry longer than the
    contract says, the extra entry a canary -> (call_host_windows' shape, sel_offsets or None)"""
    torch, libflac, dec = gpu
    n, k = len(sf) - 1, len(reqs)
    d_info = _dev(torch, info)
    d_sf, d_ss = _dev(torch, np.asarray(sf, np.uint32)), _dev(torch, np.asarray(ss, np.uint64))
    d_r = _dev(torch, libflac.window_requests(reqs))
    d_offs = _dev(torch, np.asarray(offsets, np.uint64)) if offsets is not None else None
    d_sel = torch.full(((sel_cap + 1) * 128,), CANARY, dtype=torch.uint8, device=DEV)
    d_sel_o = torch.full(((sel_cap + 1) * 8,), CANARY, dtype=torch.uint8, device=DEV)
    d_sel_f = torch.full(((k + 2) * 4,), CANARY, dtype=torch.uint8, device=DEV)
    d_sel_s = torch.full(((k + 2) * 8,), CANARY, dtype=torch.uint8, device=DEV)
    d_win = torch.full(((k + 1) * 32,), CANARY, dtype=torch.uint8, device=DEV)
    d_st = torch.full((5 * 4,), CANARY, dtype=torch.uint8, device=DEV)
    rc = dec.L.bnflac_select_windows(dec.ctx, _vp(d_offs), _vp(d_info), cap, _vp(d_sf), _vp(d_ss), n, _vp(d_r), k,
                                     _vp(d_sel_o) if offsets is not None else None, _vp(d_sel), sel_cap, _vp(d_sel_f),
                                     _vp(d_sel_s), _vp(d_win), _vp(d_st),
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, dec.L.bnflac_last_error()
    torch.cuda.synchronize()
    sel, sel_o, sel_f, sel_s, win, st = (t.cpu().numpy() for t in (d_sel, d_sel_o, d_sel_f, d_sel_s, d_win, d_st))
    assert (sel[sel_cap * 128:] == CANARY).all(), "a record was written at sel_cap"
    assert (sel_o[sel_cap * 8:] == CANARY).all(), "an offset was written at sel_cap"
    assert (sel_f[(k + 1) * 4:] == CANARY).all() and (sel_s[(k + 1) * 8:] == CANARY).all()
    assert (win[k * 32:] == CANARY).all() and (st[16:] == CANARY).all()
    w = libflac.window_array(win[: k * 32])
    out = (libflac.info_array(sel[: sel_cap * 128]), sel_f[: (k + 1) * 4].view("<u4").tolist(),
           sel_s[: (k + 1) * 8].view("<u8").tolist(), [tuple(int(x[f]) for f in WINDOW_FIELDS) for x in w],
           st[:16].view("<u4").tolist())
    return out, (sel_o[: sel_cap * 8].view("<u8") if offsets is not None else None)


def _three_way(gpu, info, cap, sf, ss, reqs, sel_cap, offsets=None):
    want = ref_windows(info, cap, sf, ss, reqs, sel_cap)
    assert_same(call_host_windows(info, cap, sf, ss, reqs, sel_cap), want)
    got, sel_o = call_device_windows(gpu, info, cap, sf, ss, reqs, sel_cap, offsets)
    assert_same(got, want)
    return got, sel_o


# ------------------------------------------------------------------ 1. device = host = Python
@pytest.mark.parametrize("shift", [0, 7])
def test_identity_requests_equal_the_device_select_ranges(gpu, shift):
    """Request s = (s, ranges[s]): every output, offsets included, byte-equal to bnflac_select_ranges
    on the same uploaded tables."""
    info, sf, ss = fabricate(MIXED, seed=1)
    cap = len(info)
    ranges = windows_by_kind(info, sf, ss, shift)
    reqs = [(s,) + tuple(r) for s, r in enumerate(ranges)]
    offsets = np.arange(cap, dtype=np.uint64) * 1000 + 7
    for sel_cap in (cap + 3, 9):
        got, sel_o = _three_way(gpu, info, cap, sf, ss, reqs, sel_cap, offsets)
        old, old_o = call_device(gpu, info, cap, sf, ss, ranges, sel_cap, offsets)
        assert_same(got, old)
        assert np.array_equal(sel_o, old_o)


def test_general_requests_on_mixed(gpu):
    """Every kind of window on every stream shape, the same reversed, three windows on one stream,
    streams nobody names, ids that name no stream; with offsets, d_sel_offsets follows the records."""
    info, sf, ss = fabricate(MIXED, seed=1)
    cap = len(info)
    offsets = np.arange(cap, dtype=np.uint64) * 1000 + 7
    every = every_kind_on_every_stream(info, sf, ss)
    for reqs in (every, every[::-1], three_on_the_long_stream(info, sf, ss), bad_ids(info, sf, ss)):
        got, sel_o = _three_way(gpu, info, cap, sf, ss, reqs, 4 * cap, offsets)
        want_o = np.zeros(4 * cap, np.uint64)
        for k, w in enumerate(got[3]):
            want_o[got[1][k]:got[1][k + 1]] = offsets[w[3]:w[3] + w[4]]
        assert np.array_equal(sel_o, want_o)
    assert got[4][0] == NO_STREAM


@pytest.mark.parametrize("nwindows", [0, 1, 1023, 1024, 1025])
def test_window_counts_around_the_scan_block(gpu, nwindows):
    """1,025 windows over 3 streams: the prefixes cross the 1,024-window workgroup of the scan."""
    rng = np.random.default_rng(nwindows)
    info, sf, ss = fabricate((5, 0, 3), seed=40)
    cap = len(info)
    reqs = []
    for _ in range(nwindows):
        t = int(rng.integers(0, 3))
        T = int(ss[t + 1]) - int(ss[t])
        reqs.append((t, int(rng.integers(0, T + 3)), int(rng.integers(0, T + 3))))
    got, _ = _three_way(gpu, info, cap, sf, ss, reqs, 5 * nwindows + 2)
    if nwindows == 1025:
        assert got[1][1025] >= got[1][1024] > 8


def test_no_streams_at_all(gpu):
    info, sf, ss = fabricate((), seed=5)
    got, _ = _three_way(gpu, info, 0, sf, ss, [(0, 0, 5), (1, 2, 3), (U64, U64, U64), (0, 0, 0), (7, 7, 7)], 3)
    assert got[4] == [NO_STREAM, 0, 0, 0] and all(w == (0, 0, 0, 0, 0, EMPTY | NO_STREAM) for w in got[3])


def test_sel_cap_one_short_and_zero(gpu):
    info, sf, ss = fabricate(MIXED, seed=1)
    cap = len(info)
    reqs = three_on_the_long_stream(info, sf, ss) + every_kind_on_every_stream(info, sf, ss)[:40]
    total = ref_windows(info, cap, sf, ss, reqs, 4 * cap)[4][1]
    got, _ = _three_way(gpu, info, cap, sf, ss, reqs, total - 1)
    assert got[4][0] == OVERFLOW and got[4][1] == total
    _three_way(gpu, info, cap, sf, ss, reqs, total)
    _three_way(gpu, info, cap, sf, ss, reqs, 0)
    got, _ = _three_way(gpu, info, cap, sf, ss, reqs[:5], cap + 40)
    assert got[0][got[4][1]:].tobytes() == filler(cap + 40 - got[4][1]).tobytes()


def test_bad_slices_count_only_when_named(gpu):
    info, sf, ss = fabricate(MIXED, seed=1)
    cap = len(info)
    sf2, ss2 = bad_slice_tables(info, sf, ss)
    good = [(3, 100, 5000), (0, 0, U64), (3, 100, 5000), (2, 0, 1), (1, 0, U64), (99, 0, 1)]
    got, _ = _three_way(gpu, info, cap, sf2, ss2, good, cap)
    assert got[4][0] == NO_STREAM and got[4][2] == 4
    for t in (5, 9, 13):
        bad, _ = _three_way(gpu, info, cap, sf2, ss2, good[:2] + [(t, 0, U64)] + good[2:], 24)
        assert bad[4] == [BAD_TABLES | NO_STREAM, 0, 0, 0] and bad[0].tobytes() == filler(24).tobytes()
        assert bad[3][2] == (0, 0, 0, int(sf2[t]), 0, EMPTY) and bad[3][-1] == (0, 0, 0, 0, 0, EMPTY | NO_STREAM)


def test_frame_prefixes_saturate(gpu):
    """65,537 windows of 65,536 frames each: 2^32 + 65,536 frames, an 8 MB index."""
    info, sf, ss, reqs = saturation_case()
    got, _ = call_device_windows(gpu, info, len(info), sf, ss, reqs, 8)
    assert_saturated(info, got)
    assert_same(got, call_host_windows(info, len(info), sf, ss, reqs, 8))


def test_out_sample_values_no_index_wrote(gpu):
    """Non-monotone out_sample: the device call returns and agrees with the host twin."""
    rng = np.random.default_rng(19)
    info, sf, ss = fabricate((9, 1, 30, 0, 5, 64), seed=400)
    cap, n = len(info), len(sf) - 1
    for wide in (False, True):
        info["out_sample"] = rng.integers(0, 1 << 63, cap, dtype=np.uint64) * 2 if wide else rng.integers(0, 20000, cap, dtype=np.uint64)
        reqs = [(int(rng.integers(0, n + 1)), int(rng.integers(0, 9000)), int(rng.integers(0, 9000))) for _ in range(40)]
        got, _ = call_device_windows(gpu, info, cap, sf, ss, reqs, 40 * 64)
        assert_same(got, call_host_windows(info, cap, sf, ss, reqs, 40 * 64))


# ------------------------------------------------------------------ 2. end to end against the generator
def _crops_of_batch(b, name):
    """2 n + 3 requests: two different overlapping windows per stream in reverse stream order, the
    first of them again, one more that is empty (C2: on the stream without frames; else past a
    stream's end) and one with a stream id that is not there."""
    n = len(b.sf) - 1
    T = [int(b.ss[s + 1] - b.ss[s]) for s in range(n)]
    reqs = []
    for s in reversed(range(n)):
        reqs += [(s, T[s] // 5, T[s] // 2), (s, T[s] // 3, T[s] // 2 + 7)]
    reqs.append(reqs[0])
    reqs.append((3, 0, 100) if name == "C2" else (1, T[1] + 5, 100))
    reqs.append((n + 2, 0, 100))
    assert len(reqs) == 2 * n + 3
    return reqs


def _select_crops(gpu, b, pristine, reqs, sel_cap):
    torch, libflac, dec = gpu
    d_sf = torch.from_numpy(b.sf.astype(np.int32)).to(DEV)
    d_ss = torch.from_numpy(b.ss.astype(np.int64)).to(DEV)
    return dec.select_windows(b.d_offs, pristine, b.cap, d_sf, d_ss, len(b.sf) - 1, reqs, sel_cap)


def _check_rows(rows, reqs, pcms, convert=lambda x: x):
    """rows[k, :, ...] against the generator's PCM of the stream request k names"""
    for k, (s, first, want) in enumerate(reqs):
        T = len(pcms[s]) if s < len(pcms) and pcms[s] is not None else 0
        lo = min(first, T)
        hi = min(lo + want, T, lo + rows.shape[1])
        if hi > lo:
            assert np.array_equal(rows[k, : hi - lo], convert(pcms[s][lo:hi])), k
        assert not rows[k, hi - lo:].any(), k


@pytest.mark.parametrize("name", ["C2", "C4", "C3", "C5"])
def test_chain_against_the_generator(gpu, name):
    torch, libflac, dec = gpu
    b, pristine, pcms, sp, nbytes = _batch(gpu, name)
    reqs = _crops_of_batch(b, name)
    k, total = len(reqs), int(b.sf[-1])
    sel_cap = 3 * total + 4
    stride = 4 * sp.channels
    index_before = pristine.clone()
    d_sel_offs, d_sel_info, d_sel_f, d_sel_s, d_win, d_st = _select_crops(gpu, b, pristine, reqs, sel_cap)
    st = d_st.cpu().numpy()
    sel_f, sel_s = d_sel_f.cpu().numpy(), d_sel_s.cpu().numpy()
    win = libflac.window_array(d_win.cpu().numpy())
    nsel = int(sel_f[-1])
    assert st[0] == NO_STREAM and st[1] == nsel <= sel_cap and nsel > total // 2
    assert win["flags"][-1] == EMPTY | NO_STREAM and (win["flags"][-2] & EMPTY)
    before = libflac.info_array(d_sel_info.cpu().numpy())
    pcm_bytes = (int(sel_s[-1]) * stride + 15) // 16 * 16 + 64
    d_pcm = torch.full((pcm_bytes,), POISON, dtype=torch.uint8, device=DEV)
    dec.decode_parsed(b.d_bytes, nbytes, sel_cap, sp, libflac.OUT_INTERLEAVED32, d_pcm, d_sel_info)
    R = max(int(w["nsamples"]) for w in win) + 3
    d_rows, d_gst = dec.gather_ranges(d_pcm, libflac.OUT_INTERLEAVED32, sp, d_win, k, R)
    torch.cuda.synchronize()
    after = libflac.info_array(d_sel_info.cpu().numpy())
    assert (after["status"][:nsel] == 0).all() and (after["crc_ok"][:nsel] == 1).all()
    assert after[nsel:].tobytes() == before[nsel:].tobytes() == filler(sel_cap - nsel).tobytes()
    assert torch.equal(pristine, index_before), "the decode of a selection wrote to the index"
    pcm = d_pcm.cpu().numpy()
    assert (pcm[int(sel_s[-1]) * stride:] == POISON).all(), "the decode wrote past the last selected sample"
    assert d_gst.cpu().numpy().tolist() == [0, 0, 0, 0]
    rows = d_rows.cpu().numpy().view("<i4").reshape(k, R, sp.channels)
    _check_rows(rows, reqs, pcms)
    assert not rows[-1].any() and not rows[-2].any()
    assert np.array_equal(rows[0], rows[2 * (len(b.sf) - 1)]) and rows[0].any()  # the repeat: its own copy, the same samples


# ------------------------------------------------------------------ 3. a packed layout as float planes
def test_packed_layout_as_float_planes(gpu):
    torch, libflac, dec = gpu
    fmt = libflac.OUT_FLACDECODER
    b, pristine, pcms, sp, nbytes = _batch(gpu, "C2")
    reqs = _crops_of_batch(b, "C2")
    k, sel_cap = len(reqs), 3 * int(b.sf[-1]) + 4
    stride = libflac.out_stride(fmt, sp)
    assert stride == 4
    _, d_sel_info, _, d_sel_s, d_win, _ = _select_crops(gpu, b, pristine, reqs, sel_cap)
    hull = int(d_sel_s.cpu().numpy()[-1])
    d_pcm = torch.full(((hull * stride + 15) // 16 * 16 + 16,), POISON, dtype=torch.uint8, device=DEV)
    dec.decode_parsed(b.d_bytes, nbytes, sel_cap, sp, fmt, d_pcm, d_sel_info)
    win = libflac.window_array(d_win.cpu().numpy())
    R = max(int(w["nsamples"]) for w in win) + 1
    planes, d_gst = dec.gather_ranges_f32(d_pcm, fmt, sp, d_win, k, R, pcm_bytes=hull * stride)
    torch.cuda.synchronize()
    want, want_st = libflac.gather_ranges_f32_host(d_pcm.cpu().numpy(), fmt, sp, win, R, pcm_bytes=hull * stride)
    got = planes.cpu().numpy()
    assert got.shape == (k, sp.channels, R) and d_gst.cpu().numpy().tolist() == want_st.tolist() == [0, 0, 0, 0]
    assert got.view(np.uint32).tobytes() == np.ascontiguousarray(want).view(np.uint32).tobytes()
    _check_rows(got.transpose(0, 2, 1), reqs, pcms, lambda x: x.astype(np.float32) / np.float32(32768))


# ------------------------------------------------------------------ 4. one index, many batches of crops
def test_corpus_reuse(gpu):
    torch, libflac, dec = gpu
    m = _mixed(gpu)
    d_bytes = _upload(torch, m["buf"])
    files = [(t[0], t[1]) for t in m["table"]]
    sp = _stream_params(libflac, m["datas"][0], 0)
    pcms = [s.pcm if s is not None else None for s in m["syn"]]
    corpus = dec.index_corpus(d_bytes, len(m["buf"]), files, sp)
    torch.cuda.synchronize()
    assert corpus.nstreams == 5 and corpus.cap == len(m["buf"]) // 16 + 16 and corpus.nbytes == len(m["buf"])
    assert corpus.scan_status.cpu().numpy().tolist() == [1, 4, 1, 0]  # the empty stream has no marker
    assert corpus.index_status.cpu().numpy()[0] == 0
    tables = (corpus.d_info, corpus.d_offsets, corpus.d_stream_frames, corpus.d_stream_samples)
    before = [t.clone() for t in tables]
    n = 3000
    batches = ([(0, 4096 * 3 - 7), (0, 100), (2, 4096 * 6 + 1), (3, 0), (4, 5000), (0, 4096 * 3 - 7)],
               [(4, 0, 10), (2, 9000, n), (1, 4000, 500)],
               [(s, 1234 * j) for j in range(6) for s in (4, 0, 2)] + [(9, 0)])
    for reqs in batches:
        rows, status = dec.decode_crops(corpus, reqs, n, libflac.OUT_INTERLEAVED32)
        torch.cuda.synchronize()
        st = status["select"].cpu().numpy().tolist()
        assert sorted(status) == ["gather", "select"] and status["gather"].cpu().numpy().tolist() == [0, 0, 0, 0]
        assert st[0] == (NO_STREAM if reqs[-1][0] == 9 else 0)
        got = rows.cpu().numpy()
        assert got.shape == (len(reqs), n, sp.channels)
        _check_rows(got, [(r[0], r[1], r[2] if len(r) == 3 else n) for r in reqs], pcms)
    reqs = batches[0]
    planes, status = dec.decode_crops_f32(corpus, torch.tensor([[s, f, n] for s, f in reqs], dtype=torch.int64, device=DEV).reshape(-1), n)
    torch.cuda.synchronize()
    assert status["select"].cpu().numpy()[0] == 0 and status["gather"].cpu().numpy().tolist() == [0, 0, 0, 0]
    got = planes.cpu().numpy()
    assert got.shape == (len(reqs), sp.channels, n)
    _check_rows(got.transpose(0, 2, 1), [(s, f, n) for s, f in reqs], pcms, lambda x: x.astype(np.float32) / np.float32(32768))
    for t, was in zip(tables, before):
        assert torch.equal(t, was), "a call over the corpus wrote to its tables"


# ------------------------------------------------------------------ 5. refusals
def test_refusals(gpu):
    torch, libflac, dec = gpu
    info, sf, ss = fabricate((4, 2), seed=8)
    cap = len(info)
    d_info, d_sf, d_ss = _dev(torch, info), _dev(torch, sf), _dev(torch, ss)
    d_r = _dev(torch, np.concatenate([libflac.window_requests([(0, 0, 1), (1, 0, 1)]).view(np.uint64), np.zeros(1, np.uint64)]))
    outs = [torch.full((n,), POISON, dtype=torch.uint8, device=DEV) for n in (4 * 128, 3 * 4, 3 * 8, 2 * 32, 16)]
    d_sel, d_sel_f, d_sel_s, d_win, d_st = outs
    hs = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(req_ptr, k):
        rc = dec.L.bnflac_select_windows(dec.ctx, None, _vp(d_info), cap, _vp(d_sf), _vp(d_ss), 2, req_ptr, k, None, _vp(d_sel),
                                         4, _vp(d_sel_f), _vp(d_sel_s), _vp(d_win), _vp(d_st), hs)
        torch.cuda.synchronize()
        return rc

    assert call(ctypes.c_void_p(d_r.data_ptr() + 4), 2) < 0 and b"d_requests must be 8-byte aligned" in dec.L.bnflac_last_error()
    assert all((t.cpu().numpy() == POISON).all() for t in outs)
    assert call(_vp(d_r), 1 << 30) < 0 and b"too many windows" in dec.L.bnflac_last_error()
    assert all((t.cpu().numpy() == POISON).all() for t in outs)
    assert call(_vp(d_r), 2) == 0 and d_st.cpu().numpy().view("<u4").tolist() == [0, 2, 2, 0]


# ------------------------------------------------------------------ 6. decode_crops: the chain, not waited for
def test_decode_crops_returns_before_earlier_work_is_done(gpu):
    """The method of tests/test_gpu_select_ranges.py section 5: decode_crops over an indexed corpus
    behind about 26 TFLOP of matrix products queued on the same stream.  When it returns, the
    products' end event has not happened yet, so no step of the chain waited for the stream.  No
    time is measured or compared."""
    torch, libflac, dec = gpu
    m = _mixed(gpu)
    d_bytes = _upload(torch, m["buf"])
    files = [(t[0], t[1]) for t in m["table"]]
    sp = _stream_params(libflac, m["datas"][0], 0)
    corpus = dec.index_corpus(d_bytes, len(m["buf"]), files, sp)
    n = 3000
    crops = [(2, 4096 * 6 + 1), (0, 4096 * 3 - 7), (0, 100), (7, 0), (4, 5000), (2, 4096 * 6 + 1), (3, 0)]
    d_reqs = torch.tensor([[s, f, n] for s, f in crops], dtype=torch.int64, device=DEV).reshape(-1)
    call = lambda: dec.decode_crops(corpus, d_reqs, n, libflac.OUT_INTERLEAVED32)
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
    assert still_busy, "decode_crops returned only after the work queued in front of it had finished"
    st = status["select"].cpu().numpy().tolist()
    assert st[0] == NO_STREAM and st[2] == 5 and status["gather"].cpu().numpy().tolist() == [0, 0, 0, 0]
    got = rows.cpu().numpy()
    assert got.shape == (len(crops), n, sp.channels)
    _check_rows(got, [(s, f, n) for s, f in crops], [s.pcm if s is not None else None for s in m["syn"]])
