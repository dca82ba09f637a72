"""bnflac_select_windows_shared: overlapping crops of an indexed batch, every frame selected once.

References, all independent of the code under test: bnflac_select_windows_shared_host (and through
tests/test_select_shared_host.py the Python `ref_shared`) on that file's cases and on the shapes at
which the device scans carry; the bnflac_select_windows chain and the generator's PCM for the whole
chain; bnflac_gather_ranges_f32_host for the float planes.  Every comparison is exact.
"""
import ctypes

import numpy as np
import pytest

from tests.conftest import gpu_available
from tests.test_gpu_index_streams import _mixed, _stream_params, _upload
from tests.test_gpu_select_ranges import _batch, _dev, _vp
from tests.test_gpu_select_windows import _check_rows, _select_crops
from tests.test_select_ranges_host import CANARY, EMPTY, OVERFLOW, U64, WINDOW_FIELDS, fabricate, filler
from tests.test_select_shared_host import (CASES, assert_same_shared, call_host_shared, ref_shared, runs_by_ref_select,
                                           sliding)
from tests.test_select_windows_host import NO_STREAM

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


def call_device_shared(gpu, info, cap, sf, ss, reqs, sel_cap, offsets=None, d_info=None):
    """bnflac_select_windows_shared itself on uploaded tables; every output one entry longer than the
    contract says, the extra entry a canary -> (call_host_shared's shape, sel_offsets or None)"""
    torch, libflac, dec = gpu
    n, k = len(sf) - 1, len(reqs)
    d_info = _dev(torch, info) if d_info is None else d_info
    d_sf, d_ss = _dev(torch, np.asarray(sf, np.uint32)), _dev(torch, np.asarray(ss, np.uint64))
    d_r = _dev(torch, libflac.window_requests(reqs))
    d_offs = _dev(torch, np.asarray(offsets, np.uint64)) if offsets is not None else None
    d_sel = torch.full(((sel_cap + 1) * 128,), CANARY, dtype=torch.uint8, device=DEV)
    d_sel_o = torch.full(((sel_cap + 1) * 8,), CANARY, dtype=torch.uint8, device=DEV)
    d_win = torch.full(((k + 1) * 32,), CANARY, dtype=torch.uint8, device=DEV)
    d_first = torch.full(((k + 1) * 4,), CANARY, dtype=torch.uint8, device=DEV)
    d_tot = torch.full((3 * 8,), CANARY, dtype=torch.uint8, device=DEV)
    d_st = torch.full((5 * 4,), CANARY, dtype=torch.uint8, device=DEV)
    rc = dec.L.bnflac_select_windows_shared(dec.ctx, _vp(d_offs), _vp(d_info), cap, _vp(d_sf), _vp(d_ss), n, _vp(d_r), k,
                                            _vp(d_sel_o) if offsets is not None else None, _vp(d_sel), sel_cap, _vp(d_win),
                                            _vp(d_first), _vp(d_tot), _vp(d_st),
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, dec.L.bnflac_last_error()
    torch.cuda.synchronize()
    sel, sel_o, win, first, tot, st = (t.cpu().numpy() for t in (d_sel, d_sel_o, d_win, d_first, d_tot, d_st))
    assert (sel[sel_cap * 128:] == CANARY).all(), "a record was written at sel_cap"
    assert (sel_o[sel_cap * 8:] == CANARY).all(), "an offset was written at sel_cap"
    assert (win[k * 32:] == CANARY).all() and (first[k * 4:] == CANARY).all()
    assert (tot[16:] == CANARY).all() and (st[16:] == CANARY).all()
    w = libflac.window_array(win[: k * 32])
    out = (libflac.info_array(sel[: sel_cap * 128]), [tuple(int(x[f]) for f in WINDOW_FIELDS) for x in w],
           first[: k * 4].view("<u4").tolist(), tot[:16].view("<u8").tolist(), st[:16].view("<u4").tolist())
    return out, (sel_o[: sel_cap * 8].view("<u8") if offsets is not None else None)


# ------------------------------------------------------------------ 1. device = host twin, on every host case
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_the_host_twin(gpu, name):
    """With offsets: d_sel_offsets follows the records, rank by rank."""
    info, cap, sf, ss, reqs, sel_cap, _ = CASES[name]
    want = call_host_shared(info, cap, sf, ss, reqs, sel_cap)
    offsets = np.arange(max(cap, 1), dtype=np.uint64) * 1000 + 7
    got, sel_o = call_device_shared(gpu, info, cap, sf, ss, reqs, sel_cap, offsets)
    assert_same_shared(got, want)
    members = sorted({i for w in got[1] for i in range(w[3], w[3] + w[4])})
    want_o = np.zeros(sel_cap, np.uint64)
    keep = min(len(members), sel_cap)
    want_o[:keep] = offsets[members[:keep]]
    assert np.array_equal(sel_o, want_o)
    got, _ = call_device_shared(gpu, info, cap, sf, ss, reqs, sel_cap)  # and without offsets
    assert_same_shared(got, want)


# ------------------------------------------------------------------ 2. where the scans carry
def test_2049_windows(gpu):
    """Three window workgroups, the last with one lane; random overlapping requests and bad ids."""
    rng = np.random.default_rng(2049)
    info, sf, ss = fabricate((5, 0, 3, 9), seed=41)
    cap = len(info)
    reqs = []
    for _ in range(2049):
        t = int(rng.integers(0, 5))  # 4: no such stream
        T = int(ss[t + 1]) - int(ss[t]) if t < 4 else 9
        reqs.append((t, int(rng.integers(0, T + 3)), int(rng.integers(0, T + 3))))
    reqs[2048] = (3, 1, U64)  # the last workgroup's one lane selects
    want = call_host_shared(info, cap, sf, ss, reqs, cap)
    assert_same_shared(want, ref_shared(info, cap, sf, ss, reqs, cap))
    got, _ = call_device_shared(gpu, info, cap, sf, ss, reqs, cap)
    assert_same_shared(got, want)
    assert got[4][0] == NO_STREAM and got[1][2048][4] > 0 and got[4][1] == cap


TWO_ROUNDS_CAP = 1024 * 1024 + 3


def two_round_tables():
    """An index of 1024 * 1024 + 3 positions that is zeros but for four short slices: at position 0,
    across position 1,024 (two position workgroups), across 1024 * 1024 (the one-workgroup scan's
    two rounds) and the last two positions, ending exactly at cap.  Stream 2 k is slice k, stream
    2 k + 1 the run of zeros behind it, which nobody names.
    -> (info, sf, ss, requests, [(first position, the slice's records)])"""
    from birdnest.audio_amd import libflac
    cap = TWO_ROUNDS_CAP
    small, s_sf, s_ss = fabricate((12, 12, 7, 2), seed=77)
    starts = (0, 1018, 1024 * 1024 - 6, cap - 2)
    info = np.zeros(cap, dtype=libflac.FRAME_INFO_DTYPE)
    sf, ss, slices = [], [], []
    for k, at in enumerate(starts):
        f0, f1 = int(s_sf[k]), int(s_sf[k + 1])
        info[at: at + f1 - f0] = small[f0:f1]
        slices.append((at, small[f0:f1]))
        sf += [at, at + f1 - f0]
        ss += [int(s_ss[k]), int(s_ss[k + 1])]
    assert sf[-1] == cap and sf[2] < 1024 < sf[3] and sf[4] < 1024 * 1024 < sf[5] == sf[6]
    sf, ss = np.array(sf, np.uint32), np.array(ss, np.uint64)
    reqs = [r for r in sliding(ss) if r[0] % 2 == 0]  # overlapping windows inside each slice
    reqs += [reqs[5], (1, 0, 10), (77, 0, 1)]  # a duplicate, an unnamed stream's empty window, no stream
    assert max(r[0] for r in reqs[:-1]) == 6 and len(reqs) > 30
    return info, sf, ss, reqs, slices


def test_an_index_of_two_scan_rounds(gpu):
    """1,025 position workgroups: the one-workgroup scan loops twice and the second round starts from
    the first one's carry.  The index is 128 MiB of zeros allocated on the device, only the slices
    are uploaded.  The last slice's last window puts its -1 into the end slot delta[cap]."""
    torch, libflac, dec = gpu
    cap = TWO_ROUNDS_CAP
    info, sf, ss, reqs, slices = two_round_tables()
    d_info = torch.zeros(cap * 128, dtype=torch.uint8, device=DEV)
    for at, rec in slices:
        d_info[at * 128: (at + len(rec)) * 128] = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(DEV)
    for sel_cap in (300, 30):
        want = call_host_shared(info, cap, sf, ss, reqs, sel_cap)
        assert_same_shared(want, ref_shared(info, cap, sf, ss, reqs, sel_cap))
        got, _ = call_device_shared(gpu, info, cap, sf, ss, reqs, sel_cap, d_info=d_info)
        assert_same_shared(got, want)
    assert got[3][0] == 33 and got[4][0] == OVERFLOW | NO_STREAM
    last = max(range(len(reqs)), key=lambda k: got[1][k][3] + got[1][k][4])
    assert got[1][last][3] + got[1][last][4] == cap, "no window ends at cap: delta[cap] was not exercised"


# ------------------------------------------------------------------ 3. end to end against the generator
def _sliding_of_batch(b, sp):
    """Windows of 3 hops every hop over every stream (hop: half a block and one sample), one of them
    again, one empty request and one that names no stream -> (requests, window)"""
    n = len(b.sf) - 1
    hop = int(sp.max_blocksize) // 2 + 1
    reqs = sliding(b.ss, 3 * hop, hop)
    T = [int(b.ss[s + 1] - b.ss[s]) for s in range(n)]
    reqs += [reqs[len(reqs) // 2], (0, T[0] + 5, 100), (n + 2, 0, 100)]
    return reqs, 3 * hop


def _distinct_positions(libflac, b, reqs):
    """The union's size from the host copy of the index, by the rule in Python."""
    info = np.zeros(len(b.rec), dtype=b.rec.dtype)
    info["out_sample"], info["blocksize"] = b.rec["out_sample"], b.rec["blocksize"]
    runs, bad = runs_by_ref_select(info, b.cap, b.sf, b.ss, reqs)
    assert not bad
    return len({i for p in runs if p is not None for i in range(p[3], p[3] + p[4])})


def _shared_chain(gpu, b, pristine, sp, nbytes, reqs, fmt, sel_cap):
    """select_windows_shared -> decode_parsed(nframes = sel_cap) into a poisoned PCM
    -> (d_pcm, d_win, d_sel_info, records before the decode, F, S, status)"""
    torch, libflac, dec = gpu
    d_sf = torch.from_numpy(b.sf.astype(np.int32)).to(DEV)
    d_ss = torch.from_numpy(b.ss.astype(np.int64)).to(DEV)
    _, d_sel_info, d_win, d_first, d_tot, d_st = dec.select_windows_shared(b.d_offs, pristine, b.cap, d_sf, d_ss,
                                                                          len(b.sf) - 1, reqs, sel_cap)
    F, S = (int(x) for x in d_tot.cpu().numpy())
    before = libflac.info_array(d_sel_info.cpu().numpy())
    stride = libflac.out_stride(fmt, sp)
    d_pcm = torch.full(((S * stride + 15) // 16 * 16 + 64,), POISON, dtype=torch.uint8, device=DEV)
    dec.decode_parsed(b.d_bytes, nbytes, sel_cap, sp, fmt, d_pcm, d_sel_info)
    return d_pcm, d_win, d_first, d_sel_info, before, F, S, d_st.cpu().numpy().tolist()


@pytest.mark.parametrize("name", ["C2", "C4", "C3", "C5"])
def test_chain_against_the_generator(gpu, name):
    torch, libflac, dec = gpu
    fmt = libflac.OUT_INTERLEAVED32
    b, pristine, pcms, sp, nbytes = _batch(gpu, name)
    reqs, window = _sliding_of_batch(b, sp)
    k, total = len(reqs), int(b.sf[-1])
    sel_cap = total + 4
    stride = 4 * sp.channels
    R = window + 3
    index_before = pristine.clone()
    d_pcm, d_win, d_first, d_sel_info, before, F, S, st = _shared_chain(gpu, b, pristine, sp, nbytes, reqs, fmt, sel_cap)
    d_rows, d_gst = dec.gather_ranges(d_pcm, fmt, sp, d_win, k, R, pcm_bytes=S * stride)
    # the bnflac_select_windows chain over the same requests
    old_cap = k * ((window - 1) // sp.min_blocksize + 2)
    _, d_old_info, d_old_f, d_old_s, d_old_win, d_old_st = _select_crops(gpu, b, pristine, reqs, old_cap)
    old_total = int(d_old_s.cpu().numpy()[-1])
    d_old_pcm = torch.zeros((old_total * stride + 15) // 16 * 16 + 16, dtype=torch.uint8, device=DEV)
    dec.decode_parsed(b.d_bytes, nbytes, old_cap, sp, fmt, d_old_pcm, d_old_info)
    d_old_rows, d_old_gst = dec.gather_ranges(d_old_pcm, fmt, sp, d_old_win, k, R)
    torch.cuda.synchronize()
    old_st = d_old_st.cpu().numpy().tolist()
    assert old_st[0] == NO_STREAM and st[0] == NO_STREAM and st[2:] == old_st[2:]
    assert st[1] == F == _distinct_positions(libflac, b, reqs) <= total
    assert F < old_st[1], "sliding windows at a third of the window share frames"
    win, old_win = libflac.window_array(d_win.cpu().numpy()), libflac.window_array(d_old_win.cpu().numpy())
    for f in ("nsamples", "skip", "first_frame", "nframes", "flags"):
        assert np.array_equal(win[f], old_win[f]), f
    assert win["flags"][-1] == EMPTY | NO_STREAM and (win["flags"][-2] & EMPTY) and not win["pcm_first"][-2:].any()
    after = libflac.info_array(d_sel_info.cpu().numpy())
    assert (after["status"][:F] == 0).all() and (after["crc_ok"][:F] == 1).all()
    assert after[F:].tobytes() == before[F:].tobytes() == filler(sel_cap - F).tobytes()
    first = d_first.cpu().numpy()
    assert all(int(first[w]) + int(win["nframes"][w]) <= F for w in range(k))
    assert torch.equal(pristine, index_before), "the decode of a selection wrote to the index"
    pcm = d_pcm.cpu().numpy()
    assert (pcm[S * stride:] == POISON).all(), "the decode wrote past the last selected sample"
    assert d_gst.cpu().numpy().tolist() == d_old_gst.cpu().numpy().tolist() == [0, 0, 0, 0]
    assert torch.equal(d_rows[: k * R * stride], d_old_rows[: k * R * stride]), "the two chains' rows differ"
    rows = d_rows.cpu().numpy()[: k * R * stride].view("<i4").reshape(k, R, sp.channels)
    _check_rows(rows, reqs, pcms)
    assert not rows[-1].any() and not rows[-2].any() and rows[: k - 2].any()


def test_packed_layout_as_float_planes(gpu):
    torch, libflac, dec = gpu
    fmt = libflac.OUT_FLACDECODER
    b, pristine, pcms, sp, nbytes = _batch(gpu, "C2")
    reqs, window = _sliding_of_batch(b, sp)
    k, sel_cap = len(reqs), int(b.sf[-1]) + 4
    stride = libflac.out_stride(fmt, sp)
    assert stride == 4
    d_pcm, d_win, _, _, _, F, S, st = _shared_chain(gpu, b, pristine, sp, nbytes, reqs, fmt, sel_cap)
    win = libflac.window_array(d_win.cpu().numpy())
    R = window + 1
    planes, d_gst = dec.gather_ranges_f32(d_pcm, fmt, sp, d_win, k, R, pcm_bytes=S * stride)
    torch.cuda.synchronize()
    want, want_st = libflac.gather_ranges_f32_host(d_pcm.cpu().numpy(), fmt, sp, win, R, pcm_bytes=S * stride)
    got = planes.cpu().numpy()
    assert got.shape == (k, sp.channels, R) and d_gst.cpu().numpy().tolist() == want_st.tolist() == [0, 0, 0, 0]
    assert got.view(np.uint32).tobytes() == np.ascontiguousarray(want).view(np.uint32).tobytes()
    _check_rows(got.transpose(0, 2, 1), reqs, pcms, lambda x: x.astype(np.float32) / np.float32(32768))


# ------------------------------------------------------------------ 4. the Python layer
def test_decode_crops_shared(gpu):
    torch, libflac, dec = gpu
    m = _mixed(gpu)
    d_bytes = _upload(torch, m["buf"])
    files = [(t[0], t[1]) for t in m["table"]]
    sp = _stream_params(libflac, m["datas"][0], 0)
    pcms = [s.pcm if s is not None else None for s in m["syn"]]
    corpus = dec.index_corpus(d_bytes, len(m["buf"]), files, sp)
    tables = (corpus.d_info, corpus.d_offsets, corpus.d_stream_frames, corpus.d_stream_samples)
    before = [t.clone() for t in tables]
    fmt = libflac.OUT_INTERLEAVED32
    n, hop = 3000, 1000
    reqs = [(s, first, n) for s, p in enumerate(pcms) if p is not None for first in range(0, len(p), hop)]
    reqs += [reqs[3], (9, 0, n), (3, 0, n)]  # a duplicate, no such stream, the stream without frames
    k = len(reqs)
    rows0, st0 = dec.decode_crops(corpus, reqs, n, fmt)
    rows1, st1 = dec.decode_crops(corpus, reqs, n, fmt, shared=True)
    torch.cuda.synchronize()
    assert sorted(st0) == ["gather", "select"] and sorted(st1) == ["gather", "select", "totals"]
    assert torch.equal(rows0, rows1) and rows1.shape == (k, n, sp.channels)
    _check_rows(rows1.cpu().numpy(), reqs, pcms)
    sel0, sel1 = st0["select"].cpu().numpy().tolist(), st1["select"].cpu().numpy().tolist()
    F, S = (int(x) for x in st1["totals"].cpu().numpy())
    assert sel1[0] == sel0[0] == NO_STREAM and sel1[2:] == sel0[2:] and sel1[1] == F < sel0[1]
    assert st1["gather"].cpu().numpy().tolist() == [0, 0, 0, 0]
    nframes = int(corpus.d_stream_frames.cpu().numpy().view(np.uint32)[-1])
    assert F == nframes, "the windows cover every stream: the union is the index"
    # the exact union bounds
    rows2, st2 = dec.decode_crops(corpus, reqs, n, fmt, shared=True, max_frames=F, max_samples=S)
    torch.cuda.synchronize()
    assert torch.equal(rows2, rows0) and st2["select"].cpu().numpy().tolist() == sel1
    assert st2["gather"].cpu().numpy().tolist() == [0, 0, 0, 0]
    # one frame short: bit 0, the rows that need the last frame are zero and counted, the others are right
    info = libflac.info_array(corpus.d_info.cpu().numpy()[: nframes * 128])
    last = int(info["blocksize"][nframes - 1])
    rows3, st3 = dec.decode_crops(corpus, reqs, n, fmt, shared=True, max_frames=F - 1, max_samples=S - last)
    torch.cuda.synchronize()
    sel3 = st3["select"].cpu().numpy().tolist()
    assert sel3 == [sel1[0] | OVERFLOW] + sel1[1:] and st3["totals"].cpu().numpy().tolist() == [F, S]
    last_stream = max(s for s, p in enumerate(pcms) if p is not None)
    needs_last = [r[0] == last_stream and r[1] + n > len(pcms[last_stream]) - last for r in reqs]
    got3, want = rows3.cpu().numpy(), rows0.cpu().numpy()
    assert any(needs_last) and st3["gather"].cpu().numpy().tolist() == [1, sum(needs_last), 0, 0]
    for w in range(k):
        assert not got3[w].any() if needs_last[w] else np.array_equal(got3[w], want[w]), w
    # float planes
    planes0, _ = dec.decode_crops_f32(corpus, reqs, n)
    planes1, stf = dec.decode_crops_f32(corpus, reqs, n, shared=True)
    planes2, _ = dec.decode_crops_f32(corpus, reqs, n, mono=True, shared=True, max_frames=F, max_samples=S)
    planes3, _ = dec.decode_crops_f32(corpus, reqs, n, mono=True)
    torch.cuda.synchronize()
    assert torch.equal(planes0, planes1) and torch.equal(planes2, planes3) and planes1.shape == (k, sp.channels, n)
    assert stf["totals"].cpu().numpy().tolist() == [F, S] and stf["gather"].cpu().numpy().tolist() == [0, 0, 0, 0]
    with pytest.raises(ValueError):
        dec.decode_crops(corpus, reqs, n, fmt, max_frames=F)
    for t, was in zip(tables, before):
        assert torch.equal(t, was), "a call over the corpus wrote to its tables"


# ------------------------------------------------------------------ 5. refusals
def test_refusals(gpu):
    torch, libflac, dec = gpu
    info, sf, ss = fabricate((4, 2), seed=8)
    cap = len(info)
    d_info, d_sf, d_ss = _dev(torch, info), _dev(torch, sf), _dev(torch, ss)
    d_r = _dev(torch, np.concatenate([libflac.window_requests([(0, 0, 1), (1, 0, 1)]).view(np.uint64), np.zeros(1, np.uint64)]))
    outs = [torch.full((n,), POISON, dtype=torch.uint8, device=DEV) for n in (4 * 128, 2 * 32, 2 * 4, 3 * 8, 16)]
    d_sel, d_win, d_first, d_tot, d_st = outs
    hs = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(req_ptr=_vp(d_r), k=2, tot_ptr=_vp(d_tot), st_ptr=_vp(d_st), win_ptr=_vp(d_win), first_ptr=_vp(d_first)):
        rc = dec.L.bnflac_select_windows_shared(dec.ctx, None, _vp(d_info), cap, _vp(d_sf), _vp(d_ss), 2, req_ptr, k, None,
                                                _vp(d_sel), 4, win_ptr, first_ptr, tot_ptr, st_ptr, hs)
        torch.cuda.synchronize()
        return rc

    for kw, word in (({"req_ptr": ctypes.c_void_p(d_r.data_ptr() + 4)}, b"d_requests must be 8-byte aligned"),
                     ({"tot_ptr": ctypes.c_void_p(d_tot.data_ptr() + 4)}, b"d_sel_totals must be 8-byte aligned"),
                     ({"first_ptr": ctypes.c_void_p(d_first.data_ptr() + 2)}, b"32-bit tables must be 4-byte aligned"),
                     ({"k": 1 << 30}, b"too many windows"), ({"tot_ptr": None}, b"null output"),
                     ({"st_ptr": None}, b"null output"), ({"win_ptr": None}, b"null table"),
                     ({"req_ptr": None}, b"null table")):
        assert call(**kw) < 0, kw
        assert word in dec.L.bnflac_last_error(), (kw, dec.L.bnflac_last_error())
        assert all((t.cpu().numpy() == POISON).all() for t in outs), kw
    sel_o = torch.zeros(4, dtype=torch.int64, device=DEV)
    rc = dec.L.bnflac_select_windows_shared(dec.ctx, None, _vp(d_info), cap, _vp(d_sf), _vp(d_ss), 2, _vp(d_r), 2, _vp(sel_o),
                                            _vp(d_sel), 4, _vp(d_win), _vp(d_first), _vp(d_tot), _vp(d_st), hs)
    assert rc < 0 and b"d_sel_offsets without d_frame_offsets" in dec.L.bnflac_last_error()
    assert all((t.cpu().numpy() == POISON).all() for t in outs)
    assert call(first_ptr=None) == 0 and (d_first.cpu().numpy() == POISON).all()  # win_sel_first may be NULL
    assert call() == 0 and d_st.cpu().numpy().view("<u4").tolist() == [0, 2, 2, 0]
    assert d_tot.cpu().numpy()[:16].view("<u8").tolist() == [2, int(info["blocksize"][0]) + int(info["blocksize"][4])]
    assert d_first.cpu().numpy().view("<u4").tolist() == [0, 1] and (d_tot.cpu().numpy()[16:] == POISON).all()
