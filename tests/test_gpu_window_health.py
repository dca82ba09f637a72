"""bnflac_window_health: which crops of a decoded selection hold damaged or missing audio.

References, all independent of the kernels: bnflac_window_health_host (and through
tests/test_window_health_host.py the rule restated in Python) on the shapes at which the device
scans carry; the geometry of a stream cut at its damage, and the generator's PCM, for the whole
chain.  Every comparison is exact.
"""
import ctypes

import numpy as np
import pytest

from tests.conftest import gpu_available
from tests.test_gpu_index_streams import _crc16, _pack, _stream_params, _upload
from tests.test_gpu_select_ranges import _dev, _vp
from tests.test_select_ranges_host import CANARY
from tests.test_window_health_host import (DAMAGED, EMPTY, HEALTH_FIELDS, NO_STREAM, SHORT, U32, UNKNOWN, call_host_health,
                                           carry_tables, stream_descs)

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


def call_device_health(gpu, sel, sel_cap, wins, first, reqs=None, totals=None, ss=None, d_sel=None):
    """bnflac_window_health itself on uploaded tables; both outputs one entry longer than the contract
    says, the extra entry a canary -> call_host_health's shape"""
    torch, libflac, dec = gpu
    k = len(wins)
    d_sel = _dev(torch, sel) if d_sel is None else d_sel
    d_win, d_first = _dev(torch, wins), _dev(torch, np.asarray(first, np.uint32))
    d_r = d_sd = d_ss = None
    if reqs is not None:
        d_r, d_sd = _dev(torch, libflac.window_requests(reqs)), _dev(torch, stream_descs(totals))
        d_ss = _dev(torch, np.asarray(ss, np.uint64))
    d_health = torch.full(((k + 1) * 32,), CANARY, dtype=torch.uint8, device=DEV)
    d_st = torch.full((5 * 4,), CANARY, dtype=torch.uint8, device=DEV)
    rc = dec.L.bnflac_window_health(dec.ctx, _vp(d_sel), sel_cap, _vp(d_win), _vp(d_first), k, _vp(d_r), _vp(d_sd), _vp(d_ss),
                                    len(totals) if reqs is not None else 0, _vp(d_health), _vp(d_st),
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, dec.L.bnflac_last_error()
    torch.cuda.synchronize()
    health, st = d_health.cpu().numpy(), d_st.cpu().numpy()
    assert (health[k * 32:] == CANARY).all(), "a record was written at nwindows"
    assert (st[16:] == CANARY).all(), "a fifth status word was written"
    h = libflac.health_array(health[: k * 32])
    return [[int(x[f]) for f in HEALTH_FIELDS] for x in h], st[:16].view("<u4").tolist()


def assert_same_health(got, want):
    assert got[1] == want[1]
    assert len(got[0]) == len(want[0])
    for w, (g, x) in enumerate(zip(got[0], want[0])):
        assert g == x, (w, g, x)


# ------------------------------------------------------------------ 5. device = host twin where the scans carry
def test_three_record_workgroups(gpu):
    """sel_cap = 2051: three workgroups of records, the last with three lanes; 2049 windows: nine
    window workgroups, the last with one lane.  Runs that start at 0, straddle 1023|1024 and
    2047|2048, end at sel_cap and one past it, cover everything, and f = n = 2^32 - 1."""
    sel, sel_cap, wins, first, reqs, totals, ss = carry_tables()
    assert sel_cap == 2051 and len(wins) == 2049
    runs = {(int(f), int(n)) for f, n in zip(first, wins["nframes"])}
    assert {(0, 5), (1020, 9), (2040, 12), (sel_cap - 4, 4), (sel_cap - 4, 5), (0, sel_cap), (U32, U32)} <= runs
    assert {0, U32} <= set(sel["blocksize"].tolist()) and any(r[0] >= len(totals) for r in reqs)
    want = call_host_health(sel, sel_cap, wins, first, reqs, totals, ss)
    assert want[1][0] == DAMAGED | SHORT | UNKNOWN
    assert_same_health(call_device_health(gpu, sel, sel_cap, wins, first, reqs, totals, ss), want)
    # and without the request tables
    want = call_host_health(sel, sel_cap, wins, first)
    assert want[1][2] == 0
    assert_same_health(call_device_health(gpu, sel, sel_cap, wins, first), want)


def test_small_and_empty_selections(gpu):
    """One workgroup with a few lanes; sel_cap = 0, where no record is read and every run is unknown."""
    for sel_cap, k in ((5, 70), (1024, 64), (1025, 65), (0, 9)):
        sel, _, wins, first, reqs, totals, ss = carry_tables(sel_cap=sel_cap, nwindows=k, seed=sel_cap + 1)
        want = call_host_health(sel, sel_cap, wins, first, reqs, totals, ss)
        assert_same_health(call_device_health(gpu, sel, sel_cap, wins, first, reqs, totals, ss), want)
    assert all(r[1:5] == [0, 0, 0, 0] for r in want[0]) and want[1][1] == 0


# ------------------------------------------------------------------ 6. two rounds of the one-workgroup scan
TWO_ROUNDS = 1024 * 1024 + 3


def test_two_rounds_of_the_workgroup_scan(gpu):
    """1,025 record workgroups: k_hl_scan loops twice and the second round starts from the first one's
    carry.  The records are 128 MiB of zeros allocated on the device (a zero record is bad: status 0,
    crc_ok 0), only four slices of good records are uploaded."""
    torch, libflac, dec = gpu
    cap = TWO_ROUNDS
    rng = np.random.default_rng(6)
    sel = np.zeros(cap, dtype=libflac.FRAME_INFO_DTYPE)
    d_sel = torch.zeros(cap * 128, dtype=torch.uint8, device=DEV)
    slices = ((0, 12), (1018, 12), (1024 * 1024 - 6, 7), (cap - 1, 1))
    for at, n in slices:
        good = np.frombuffer(rng.bytes(128 * n), dtype=libflac.FRAME_INFO_DTYPE).copy()
        good["status"], good["crc_ok"] = 0, 1
        good["blocksize"] = rng.integers(1, 4609, n)
        sel[at: at + n] = good
        d_sel[at * 128: (at + n) * 128] = torch.from_numpy(good.view(np.uint8).reshape(-1).copy()).to(DEV)
    ngood = sum(n for _, n in slices)
    runs = [(0, 12), (1018, 12), (1000, 40), (1024 * 1024 - 6, 7), (1024 * 1024 - 1, 2), (1024 * 1024, 1), (cap - 3, 3),
            (cap - 3, 4), (cap - 2, 2), (0, cap), (1023, 1), (1024, 1), (300000, 700010), (cap, 1), (5, 0)]
    wins = np.zeros(len(runs), dtype=libflac.WINDOW_DTYPE)
    wins["nframes"] = [n for _, n in runs]
    wins["skip"] = rng.integers(0, 100, len(runs))
    wins["nsamples"] = rng.integers(0, 20000, len(runs))
    first = [f for f, _ in runs]
    want = call_host_health(sel, cap, wins, first)
    got = call_device_health(gpu, sel, cap, wins, first, d_sel=d_sel)
    assert_same_health(got, want)
    by = dict(zip(runs, got[0]))
    assert by[(0, 12)][:3] == [0, 0, 0] and by[(1018, 12)][:3] == [0, 0, 0] and by[(1024 * 1024 - 6, 7)][:3] == [0, 0, 0]
    assert by[(0, cap)][:3] == [DAMAGED, cap - ngood, cap - ngood], "every zero record is a crc record"
    assert by[(cap - 3, 3)][:3] == [DAMAGED, 1, 1] and by[(cap - 3, 4)][:3] == [DAMAGED | UNKNOWN, 1, 1]
    assert by[(cap - 2, 2)][:3] == [DAMAGED, 1, 1] and by[(1024 * 1024 - 1, 2)][:3] == by[(1024 * 1024, 1)][:3] == [0, 0, 0]
    assert by[(300000, 700010)][1] == 700010 and by[(1000, 40)][1] == 40 - 12 and got[1] == [DAMAGED | UNKNOWN, 6, 0, 2]


# ------------------------------------------------------------------ 7. end to end on real damage
CROPS = [(1, 0), (1, 18000), (1, 22000), (1, 30000), (1, 47000), (0, 18000), (2, 40000), (2, 47000), (7, 0)]
N = 6000


@pytest.fixture(scope="module")
def damaged(gpu):
    """The corpus of test_damage_is_local: three C2 streams of 12 frames of 4096, stream 1 with one
    bit flipped in frame 5's last subframe.  The index keeps 12, 6 and 12 frames: T_1 = 24576 of
    STREAMINFO's 49152, and frame 5 = [20480, 24576) fails its CRC."""
    from birdnest.audio_amd import synth
    torch, libflac, dec = gpu
    syn = [synth.encode(synth.config("C2", nframes=12, seed=21 + i)) for i in range(3)]
    datas = [bytearray(s.data.tobytes()) for s in syn]
    o = [int(x) for x in syn[1].frame_offsets]
    datas[1][o[6] - 10] ^= 0x10
    assert _crc16(bytes(datas[1][o[5]:o[6]])) != 0
    datas = [bytes(d) for d in datas]
    buf, ranges = _pack(datas, (7, 2))
    sp = _stream_params(libflac, datas[0], 0)
    assert sp.min_blocksize == sp.max_blocksize == 4096 and all(s.nsamples == 49152 for s in syn)
    corpus = dec.index_corpus(_upload(torch, buf), len(buf), ranges, sp)
    torch.cuda.synchronize()
    assert np.diff(corpus.d_stream_frames.cpu().numpy()).tolist() == [12, 6, 12]
    assert np.diff(corpus.d_stream_samples.cpu().numpy()).tolist() == [49152, 24576, 49152]
    return corpus, [s.pcm for s in syn], sp


def _health(libflac, status):
    h = libflac.health_array(status["windows_health"].cpu().numpy())
    return {c: {f: int(x[f]) for f in HEALTH_FIELDS} for c, x in zip(CROPS, h)}, status["health"].cpu().numpy().tolist()


@pytest.mark.parametrize("shared", [False, True])
def test_crops_of_a_damaged_corpus(gpu, damaged, shared):
    torch, libflac, dec = gpu
    corpus, pcms, sp = damaged
    fmt = libflac.OUT_INTERLEAVED32
    rows0, st0 = dec.decode_crops(corpus, CROPS, N, fmt, shared=shared)
    rows, st = dec.decode_crops(corpus, CROPS, N, fmt, shared=shared, health=True)
    torch.cuda.synchronize()
    assert torch.equal(rows, rows0), "health=True changed the rows"
    assert sorted(st) == sorted(list(st0) + ["health", "windows_health"])
    assert all(torch.equal(st[key], st0[key]) for key in st0)
    assert st["windows_health"].shape == (len(CROPS), 32) and st["health"].dtype == torch.int32
    h, words = _health(libflac, st)
    print("health", shared, words, h)
    got = rows.cpu().numpy()
    row = {c: got[k] for k, c in enumerate(CROPS)}
    zero = dict.fromkeys(HEALTH_FIELDS, 0)
    for s, lo in ((1, 0), (0, 18000), (2, 40000)):
        assert h[(s, lo)] == zero and np.array_equal(row[(s, lo)], pcms[s][lo: lo + N]), (s, lo)
    x = h[(1, 18000)]
    assert (x["flags"], x["bad_frames"], x["bad_samples"], x["missing"]) == (DAMAGED, 1, 3520, 0) and x["crc_frames"] <= 1
    assert np.array_equal(row[(1, 18000)][:2480], pcms[1][18000:20480]) and not row[(1, 18000)][2480:].any()
    x = h[(1, 22000)]
    assert (x["flags"], x["bad_frames"], x["bad_samples"], x["missing"]) == (DAMAGED | SHORT, 1, 2576, 3424)
    assert h[(1, 30000)] == dict(zero, flags=SHORT | EMPTY, missing=6000) and not row[(1, 30000)].any()
    assert h[(1, 47000)] == dict(zero, flags=SHORT | EMPTY, missing=2152) and not row[(1, 47000)].any()
    assert h[(2, 47000)] == zero, "clipped by the stream's true end: not SHORT"
    assert np.array_equal(row[(2, 47000)][:2152], pcms[2][47000:]) and not row[(2, 47000)][2152:].any()
    assert h[(7, 0)] == dict(zero, flags=NO_STREAM | EMPTY) and not row[(7, 0)].any()
    assert words == [DAMAGED | SHORT, 2, 3, 0]
    # the float planes' call reports the same health
    planes0, _ = dec.decode_crops_f32(corpus, CROPS, N, shared=shared)
    planes, stf = dec.decode_crops_f32(corpus, CROPS, N, shared=shared, health=True)
    torch.cuda.synchronize()
    assert torch.equal(planes, planes0) and _health(libflac, stf) == (h, words)
    assert corpus.missing_samples().cpu().numpy().tolist() == [0, 24576, 0]


# ------------------------------------------------------------------ 8. UNKNOWN through the public path
def test_unknown_when_records_were_not_provided(gpu, damaged):
    """A shared selection one record short of the union: select status bit 0, and UNKNOWN on exactly
    the windows whose runs pass sel_cap.  The same chain by its single calls gives the records the
    twin needs."""
    torch, libflac, dec = gpu
    corpus, pcms, sp = damaged
    fmt = libflac.OUT_INTERLEAVED32
    reqs = [(s, lo, N) for s in range(3) for lo in range(0, 49152, 3000)]
    k = len(reqs)
    _, st = dec.decode_crops(corpus, reqs, N, fmt, shared=True)
    F, S = (int(x) for x in st["totals"].cpu().numpy())
    assert F == 30
    rows, st = dec.decode_crops(corpus, reqs, N, fmt, shared=True, max_frames=F - 1, health=True)
    torch.cuda.synchronize()
    assert st["select"].cpu().numpy()[0] & 1, "more frames selected than provided"
    # the same chain, call by call
    _, d_sel_info, d_win, d_first, _, _ = dec.select_windows_shared(corpus.d_offsets, corpus.d_info, corpus.cap,
                                                                    corpus.d_stream_frames, corpus.d_stream_samples,
                                                                    corpus.nstreams, reqs, F - 1)
    d_pcm = torch.zeros(S * 4 * sp.channels + 64, dtype=torch.uint8, device=DEV)
    dec.decode_parsed(corpus.d_bytes, corpus.nbytes, F - 1, sp, fmt, d_pcm, d_sel_info)
    d_health, d_st = dec.window_health(d_sel_info, F - 1, d_win, d_first, k, reqs, corpus)
    torch.cuda.synchronize()
    assert torch.equal(d_health.view(k, 32), st["windows_health"]) and torch.equal(d_st, st["health"])
    sel = libflac.info_array(d_sel_info.cpu().numpy())
    wins, first = libflac.window_array(d_win.cpu().numpy()), d_first.cpu().numpy().view(np.uint32)
    totals = corpus.d_streams.cpu().numpy().reshape(-1, 4)[:, 3].tolist()
    assert totals == [49152] * 3
    twin, twin_st = call_host_health(sel, F - 1, wins, first, reqs, totals, corpus.d_stream_samples.cpu().numpy())
    h = libflac.health_array(st["windows_health"].cpu().numpy())
    assert [[int(x[f]) for f in HEALTH_FIELDS] for x in h] == twin and st["health"].cpu().numpy().tolist() == twin_st
    passes = [int(first[w]) + int(wins["nframes"][w]) > F - 1 for w in range(k)]
    assert [bool(x["flags"] & UNKNOWN) for x in h] == passes and sum(passes) == 3 == twin_st[3]
    assert all(r[0] == 2 and r[1] >= 42000 for r, p in zip(reqs, passes) if p)
    assert twin_st[1] == sum(1 for s, lo, _ in reqs if s == 1 and lo < 24576 and lo + N > 20480) == 4
    assert twin_st[2] == sum(1 for s, lo, _ in reqs if s == 1 and lo + N > 24576) == 10
    # a corpus made without the descriptor table serves health=False only
    bare = libflac.Corpus(corpus.d_bytes, corpus.nbytes, sp, corpus.nstreams, corpus.cap, corpus.d_offsets, corpus.d_info,
                          corpus.d_stream_frames, corpus.d_stream_samples, corpus.scan_status, corpus.index_status)
    for refused in (lambda: dec.decode_crops(bare, reqs, N, fmt, health=True), bare.missing_samples,
                    lambda: dec.window_health(d_sel_info, F - 1, d_win, d_first, k, reqs, bare),
                    lambda: dec.window_health(d_sel_info, F - 1, d_win, d_first, k, reqs)):
        with pytest.raises(ValueError):
            refused()
    bad_only, _ = dec.window_health(d_sel_info, F - 1, d_win, d_first, k)
    torch.cuda.synchronize()
    flags = libflac.health_array(bad_only.cpu().numpy())["flags"]
    assert [int(x) for x in flags] == [r[0] & ~(SHORT | NO_STREAM) for r in twin]


# ------------------------------------------------------------------ 9. refusals and no windows
def test_refusals_and_no_windows(gpu):
    torch, libflac, dec = gpu
    sel, sel_cap, wins, first, reqs, totals, ss = carry_tables(sel_cap=20, nwindows=8)
    pad = lambda a: np.concatenate([np.ascontiguousarray(a).view(np.uint8).reshape(-1), np.zeros(16, np.uint8)])
    d_sel, d_win, d_first = _dev(torch, pad(sel)), _dev(torch, pad(wins)), _dev(torch, pad(first))
    d_r, d_sd = _dev(torch, pad(libflac.window_requests(reqs))), _dev(torch, pad(stream_descs(totals)))
    d_ss = _dev(torch, pad(ss))
    d_health = torch.full((8 * 32 + 16,), POISON, dtype=torch.uint8, device=DEV)
    d_st = torch.full((16 + 16,), POISON, dtype=torch.uint8, device=DEV)
    hs = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    off = lambda t, n: ctypes.c_void_p(t.data_ptr() + n)

    def call(**kw):
        a = dict(ctx=dec.ctx, sel=_vp(d_sel), win=_vp(d_win), first=_vp(d_first), k=8, r=_vp(d_r), sd=_vp(d_sd), ss=_vp(d_ss),
                 health=_vp(d_health), st=_vp(d_st))
        a.update(kw)
        rc = dec.L.bnflac_window_health(a["ctx"], a["sel"], sel_cap, a["win"], a["first"], a["k"], a["r"], a["sd"], a["ss"],
                                        len(totals), a["health"], a["st"], hs)
        torch.cuda.synchronize()
        return rc

    for kw, word in (({"ctx": None}, b"null ctx"), ({"sel": None}, b"null table"), ({"win": None}, b"null table"),
                     ({"first": None}, b"null table"), ({"health": None}, b"null output"), ({"st": None}, b"null output"),
                     ({"r": None}, b"all given or all null"), ({"sd": None}, b"all given or all null"),
                     ({"ss": None}, b"all given or all null"), ({"sd": None, "ss": None}, b"all given or all null"),
                     ({"sel": off(d_sel, 8)}, b"d_sel_info must be 16-byte aligned"),
                     ({"win": off(d_win, 4)}, b"64-bit tables must be 8-byte aligned"),
                     ({"r": off(d_r, 4)}, b"64-bit tables must be 8-byte aligned"),
                     ({"sd": off(d_sd, 4)}, b"64-bit tables must be 8-byte aligned"),
                     ({"ss": off(d_ss, 4)}, b"64-bit tables must be 8-byte aligned"),
                     ({"health": off(d_health, 4)}, b"64-bit tables must be 8-byte aligned"),
                     ({"first": off(d_first, 2)}, b"32-bit tables must be 4-byte aligned"),
                     ({"st": off(d_st, 2)}, b"32-bit tables must be 4-byte aligned"), ({"k": 1 << 30}, b"too many windows")):
        assert call(**kw) < 0, kw
        assert word in dec.L.bnflac_last_error(), (kw, dec.L.bnflac_last_error())
        assert (d_health.cpu().numpy() == POISON).all() and (d_st.cpu().numpy() == POISON).all(), kw
    # no windows: a zero status, no record written
    assert call(k=0) == 0
    assert d_st.cpu().numpy()[:16].view("<u4").tolist() == [0, 0, 0, 0] and (d_st.cpu().numpy()[16:] == POISON).all()
    assert (d_health.cpu().numpy() == POISON).all()
    # the call as it is meant, and with tables that are 8- but not 16-byte aligned
    want = call_host_health(sel, sel_cap, wins, first, reqs, totals, ss)
    assert call() == 0
    h = libflac.health_array(d_health.cpu().numpy()[: 8 * 32])
    assert [[int(x[f]) for f in HEALTH_FIELDS] for x in h] == want[0] and d_st.cpu().numpy()[:16].view("<u4").tolist() == want[1]
    assert (d_health.cpu().numpy()[8 * 32:] == POISON).all()
    d_win8 = torch.zeros(8 * 32 + 24, dtype=torch.uint8, device=DEV)
    d_win8[8: 8 + 8 * 32] = d_win[: 8 * 32]
    d_health.fill_(POISON)
    assert call(win=off(d_win8, 8), health=off(d_health, 8)) == 0
    h = libflac.health_array(d_health.cpu().numpy()[8: 8 + 8 * 32])
    assert [[int(x[f]) for f in HEALTH_FIELDS] for x in h] == want[0]
    assert (d_health.cpu().numpy()[:8] == POISON).all() and (d_health.cpu().numpy()[8 + 8 * 32:] == POISON).all()
