"""bnflac_index_streams: many streams of one buffer indexed in one call.

Two references, both independent of the batched code: the generator's frame offsets / PCM, and
bnflac_index_stream run on each stream copied alone into its own buffer.  Everything is exact.
"""
import ctypes
import json
import os

import numpy as np
import pytest

from tests.conftest import gpu_available

pytestmark = pytest.mark.gpu

GOLD_DIR = os.path.join(os.path.dirname(__file__), "golden")
GOLD = json.load(open(os.path.join(GOLD_DIR, "golden.json")))
GAP = bytes([0xF8, 0xFF]) * 32  # gap filler: sync pairs in the gaps and across the stream ends
POISON = 0x5A


@pytest.fixture(scope="module")
def gpu():
    if not gpu_available():
        pytest.skip("no GPU")
    import torch
    from birdnest.audio_amd import libflac
    return torch, libflac, libflac.BatchDecoder(0)


def _stream_params(libflac, data: bytes, total=None):
    """STREAMINFO -> StreamParams (host parse of the 34-byte block, like MetadataCallback)."""
    si = data[8:42]
    x = int.from_bytes(si[10:18], "big")
    return libflac.StreamParams(1, int.from_bytes(si[0:2], "big"), int.from_bytes(si[2:4], "big"), x >> 44,
                                ((x >> 41) & 7) + 1, ((x >> 36) & 31) + 1, (x & ((1 << 36) - 1)) if total is None else total)


def _first_frame_offset(data: bytes) -> int:
    """Byte after the last metadata block (what read_metadata_ leaves the reader at)."""
    assert data[:4] == b"fLaC"
    p = 4
    while True:
        hdr = data[p]
        p += 4 + int.from_bytes(data[p + 1:p + 4], "big")
        if hdr & 0x80:
            return p


def _crc16(b: bytes) -> int:
    c = 0
    for x in b:
        c ^= x << 8
        for _ in range(8):
            c = ((c << 1) ^ 0x8005) & 0xFFFF if c & 0x8000 else (c << 1) & 0xFFFF
    return c


def _upload(torch, data: bytes):
    n = len(data)
    d = torch.zeros((n + 15) // 16 * 16 + 16, dtype=torch.uint8, device="cuda:0")
    if n:
        d[:n] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")
    return d


def _alone(gpu, data: bytes, first: int, total: int):
    """The reference: bnflac_index_stream on one stream alone -> (offsets, out_sample, records)."""
    torch, libflac, dec = gpu
    if not data:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), libflac.info_array(np.zeros(0, np.uint8))
    sp = _stream_params(libflac, data, total)
    cap = len(data) // 16 + 16
    offs, os_, info, nf = dec.index_stream(_upload(torch, data), len(data), first, sp, cap)
    assert nf <= cap
    rec = libflac.info_array(info[: nf * libflac.FRAME_INFO_BYTES].cpu().numpy())
    return offs[:nf].cpu().numpy(), os_[:nf].cpu().numpy(), rec


def _pack(streams, gaps):
    """streams: [bytes]; gaps[i] bytes of filler after stream i -> (buffer, [(begin, end)])"""
    buf, ranges = bytearray(), []
    for i, d in enumerate(streams):
        ranges.append((len(buf), len(buf) + len(d)))
        buf += d
        if i < len(gaps):
            buf += GAP[: gaps[i]]
    return bytes(buf), ranges


class Batch:
    """One index_streams call, synchronised and copied to the host."""

    def __init__(self, gpu, buf: bytes, table, sp, cap=None, cand_cap=0, d_bytes=None):
        torch, libflac, dec = gpu
        self.d_bytes = _upload(torch, buf) if d_bytes is None else d_bytes
        self.cap = cap = (len(buf) // 16 + 16) if cap is None else cap
        self.d_offs, self.d_os, self.d_info, d_sf, d_ss, d_st = dec.index_streams(self.d_bytes, len(buf), table, sp, cap,
                                                                                  cand_cap=cand_cap)
        torch.cuda.synchronize()
        self.sf = d_sf.cpu().numpy().astype(np.int64)
        self.ss = d_ss.cpu().numpy()
        self.status = d_st.cpu().numpy().astype(np.int64)
        n = min(int(self.sf[-1]), cap)
        self.offs = self.d_offs[:n].cpu().numpy()
        self.os = self.d_os[:n].cpu().numpy()
        self.rec = libflac.info_array(self.d_info[: n * libflac.FRAME_INFO_BYTES].cpu().numpy())

    def stream(self, s):
        return slice(int(self.sf[s]), int(self.sf[s + 1]))


def _assert_parity(b: Batch, s: int, begin: int, ref):
    """Stream s of the batch against its stream-alone reference, records byte for byte"""
    r_offs, r_os, r_rec = ref
    sl = b.stream(s)
    assert sl.stop - sl.start == len(r_offs), s
    assert np.array_equal(b.offs[sl], r_offs + begin), s
    assert np.array_equal(b.os[sl] - int(b.ss[s]), r_os), s
    got = b.rec[sl].copy()
    assert np.array_equal(got["frame_off"].astype(np.int64), r_offs + begin), s
    assert np.array_equal(got["out_sample"].astype(np.int64), b.os[sl]), s
    got["frame_off"] -= np.uint64(begin)
    got["out_sample"] -= np.uint64(int(b.ss[s]))
    assert got.tobytes() == r_rec.tobytes(), s
    assert int(b.ss[s + 1] - b.ss[s]) == int(r_rec["blocksize"].sum()), s


# ------------------------------------------------------------------ 1. parity, mixed sizes
_MIXED = {}


def _mixed(gpu):
    """Five C2 streams of 12, 1, 7, 0 and 3 frames, gaps of 0, 5, 16 and 33 filler bytes, one
    trailing 0xFF inside stream 2's range; with the stream-alone references (computed once)."""
    if not _MIXED:
        from birdnest.audio_amd import synth
        torch, libflac, dec = gpu
        syn = [synth.encode(synth.config("C2", nframes=nf, seed=11 + 7 * i)) if nf else None
               for i, nf in enumerate((12, 1, 7, 0, 3))]
        datas = [s.data.tobytes() if s else b"" for s in syn]
        datas[2] += b"\xff"  # junk in the range; with the filler's 0xF8 a sync pair across its end
        buf, ranges = _pack(datas, (0, 5, 16, 33))
        assert any(b & 1 for b, _ in ranges)
        table = [(b, e, b + (_first_frame_offset(d) if d else 0), _stream_params(libflac, d).total_samples if d else 0)
                 for (b, e), d in zip(ranges, datas)]
        refs = [_alone(gpu, d, t[2] - t[0], t[3]) for d, t in zip(datas, table)]
        _MIXED.update(syn=syn, datas=datas, buf=buf, table=table, refs=refs, sp=_stream_params(libflac, datas[0], 0))
    return _MIXED


def _assert_mixed(m, b: Batch):
    assert b.status[0] == 0 and b.status[3] == 0
    assert np.diff(b.sf).tolist() == [12, 1, 7, 0, 3]
    assert b.status[2] == 23
    for s, (syn, t) in enumerate(zip(m["syn"], m["table"])):
        if syn is not None:
            assert np.array_equal(b.offs[b.stream(s)], syn.frame_offsets.astype(np.int64) + t[0])
        _assert_parity(b, s, t[0], m["refs"][s])


def test_parity_mixed_sizes(gpu):
    m = _mixed(gpu)
    _assert_mixed(m, Batch(gpu, m["buf"], m["table"], m["sp"]))


# ------------------------------------------------------------------ 2. each config once
@pytest.mark.parametrize("cfg,nframes", [("C3", 16), ("C4", 40), ("C5", 8)])
def test_configs_decode_whole_buffer(gpu, cfg, nframes):
    from birdnest.audio_amd import synth
    torch, libflac, dec = gpu
    syn = [synth.encode(synth.config(cfg, nframes=nframes, seed=5 + 100 * i)) for i in range(3)]
    datas = [s.data.tobytes() for s in syn]
    buf, ranges = _pack(datas, (3, 0))
    sps = [_stream_params(libflac, d) for d in datas]
    sp = _stream_params(libflac, datas[0], 0)
    for q in sps:  # a batch shares everything but the totals
        assert (q.min_blocksize, q.max_blocksize, q.sample_rate, q.channels, q.bps) == \
            (sp.min_blocksize, sp.max_blocksize, sp.sample_rate, sp.channels, sp.bps)
    table = [(b, e, b + _first_frame_offset(d), q.total_samples) for (b, e), d, q in zip(ranges, datas, sps)]
    b = Batch(gpu, buf, table, sp)
    assert b.status[0] == 0
    assert np.diff(b.sf).tolist() == [nframes] * 3
    for s, (y, t) in enumerate(zip(syn, table)):
        assert np.array_equal(b.offs[b.stream(s)], y.frame_offsets.astype(np.int64) + t[0])
    want = np.concatenate([y.pcm for y in syn])
    assert np.array_equal(b.ss, np.concatenate([[0], np.cumsum([len(y.pcm) for y in syn])]))
    total, nf = len(want), int(b.sf[-1])
    d_out = torch.full((total * sp.channels * 4 + 64,), 0xAB, dtype=torch.uint8, device="cuda:0")
    dec.decode_parsed(b.d_bytes, len(buf), nf, sp, libflac.OUT_INTERLEAVED32, d_out, b.d_info)
    torch.cuda.synchronize()
    rec = libflac.info_array(b.d_info[: nf * libflac.FRAME_INFO_BYTES].cpu().numpy())
    assert (rec["status"] == 0).all() and (rec["crc_ok"] == 1).all()
    pcm = d_out[: total * sp.channels * 4].cpu().numpy().view("<i4").reshape(-1, sp.channels)
    assert np.array_equal(pcm, want)


# ------------------------------------------------------------------ 3. the stream end as the limit
def test_stream_end_is_the_truncation_limit(gpu):
    """An 8-channel stream cut 40 bytes into its last frame, the next stream right behind it:
    the cut frame's walk runs on into the next stream's bytes and must not count."""
    from birdnest.audio_amd import synth
    torch, libflac, dec = gpu
    a = synth.encode(synth.config("C5", nframes=6, seed=3))
    c = synth.encode(synth.config("C5", nframes=4, seed=4))
    da = a.data.tobytes()[: int(a.frame_offsets[-1]) + 40]
    dc = c.data.tobytes()
    buf, ranges = _pack([da, dc], ())
    assert ranges[1][0] == ranges[0][1]
    table = [(ranges[0][0], ranges[0][1], _first_frame_offset(da), _stream_params(libflac, da).total_samples),
             (ranges[1][0], ranges[1][1], ranges[1][0] + _first_frame_offset(dc), _stream_params(libflac, dc).total_samples)]
    refs = [_alone(gpu, d, t[2] - t[0], t[3]) for d, t in zip((da, dc), table)]
    assert len(refs[0][0]) == 5 and len(refs[1][0]) == 4  # the reference really drops the cut frame
    b = Batch(gpu, buf, table, _stream_params(libflac, da, 0))
    assert b.status[0] == 0
    assert np.diff(b.sf).tolist() == [5, 4]
    for s in range(2):
        _assert_parity(b, s, table[s][0], refs[s])


# ------------------------------------------------------------------ 4. damage is local
def test_damage_is_local(gpu):
    from birdnest.audio_amd import synth
    torch, libflac, dec = gpu
    syn = [synth.encode(synth.config("C2", nframes=12, seed=21 + i)) for i in range(3)]
    datas = [bytearray(s.data.tobytes()) for s in syn]
    o = [int(x) for x in syn[1].frame_offsets]
    datas[1][o[6] - 10] ^= 0x10  # inside frame 5's last subframe: its header and walk stay valid
    assert _crc16(bytes(datas[1][o[5]:o[6]])) != 0
    datas = [bytes(d) for d in datas]
    buf, ranges = _pack(datas, (7, 2))
    table = [(b, e, b + _first_frame_offset(d), _stream_params(libflac, d).total_samples)
             for (b, e), d in zip(ranges, datas)]
    b = Batch(gpu, buf, table, _stream_params(libflac, datas[0], 0))
    assert b.status[0] == 0
    assert np.diff(b.sf).tolist() == [12, 6, 12]
    for s, keep in enumerate((12, 6, 12)):
        assert np.array_equal(b.offs[b.stream(s)], syn[s].frame_offsets.astype(np.int64)[:keep] + table[s][0])


# ------------------------------------------------------------------ 5. EOS and head per stream
def test_eos_and_head_per_stream(gpu):
    torch, libflac, dec = gpu
    g = GOLD["c4_mixed_varbs"]
    data = open(os.path.join(GOLD_DIR, g["file"]), "rb").read()
    fo = np.array(g["frame_offsets"], dtype=np.int64)
    nf = len(fo)
    first = _first_frame_offset(data)
    sp = _stream_params(libflac, data)
    r_offs, r_os, r_rec = _alone(gpu, data, first, sp.total_samples)
    assert np.array_equal(r_offs, fo)
    bs = r_rec["blocksize"].astype(np.int64)
    k = nf // 2
    buf, ranges = _pack([data] * 3, (1, 0))
    table = [(ranges[0][0], ranges[0][1], ranges[0][0] + first, sp.total_samples),
             (ranges[1][0], ranges[1][1], ranges[1][0] + first, int(r_os[k]) + 1),  # ends inside frame k
             (ranges[2][0], ranges[2][1], ranges[2][0] + int(fo[0]) + 1, 0)]       # starts inside frame 0
    b = Batch(gpu, buf, table, sp)
    assert b.status[0] == 0
    assert np.diff(b.sf).tolist() == [nf, k + 1, nf - 1]
    assert np.array_equal(b.offs[b.stream(0)], fo + ranges[0][0])
    assert np.array_equal(b.offs[b.stream(1)], fo[: k + 1] + ranges[1][0])
    assert np.array_equal(b.offs[b.stream(2)], fo[1:] + ranges[2][0])
    assert b.ss.tolist() == np.concatenate([[0], np.cumsum([bs.sum(), bs[: k + 1].sum(), bs[1:].sum()])]).tolist()
    want_os = np.concatenate([np.cumsum(bs) - bs, b.ss[1] + np.cumsum(bs[: k + 1]) - bs[: k + 1],
                              b.ss[2] + np.cumsum(bs[1:]) - bs[1:]])
    assert np.array_equal(b.os, want_os)
    assert np.array_equal(b.rec["out_sample"].astype(np.int64), want_os)


# ------------------------------------------------------------------ 6. overflow and bad table
def _raw(gpu, d_bytes, nbytes, table, sp, cap, nout, cand_cap=0):
    """The C call itself on poisoned outputs of nout entries -> host copies"""
    torch, libflac, dec = gpu
    dev = "cuda:0"
    n = len(table)
    tab = np.array([tuple(t) for t in table], dtype=libflac.STREAM_DESC_DTYPE)
    d_tab = torch.from_numpy(tab.view(np.int64).reshape(-1).copy()).to(dev)
    d_offs = torch.full((nout,), POISON, dtype=torch.int64, device=dev)
    d_os = torch.full((nout,), POISON, dtype=torch.int64, device=dev)
    d_info = torch.full((nout * libflac.FRAME_INFO_BYTES,), POISON, dtype=torch.uint8, device=dev)
    d_sf = torch.full((n + 1,), POISON, dtype=torch.int32, device=dev)
    d_ss = torch.full((n + 1,), POISON, dtype=torch.int64, device=dev)
    d_st = torch.full((4,), POISON, dtype=torch.int32, device=dev)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = dec.L.bnflac_index_streams(dec.ctx, vp(d_bytes), nbytes, vp(d_tab), n, ctypes.byref(sp), cand_cap, vp(d_offs),
                                    vp(d_os), vp(d_info), cap, vp(d_sf), vp(d_ss), vp(d_st),
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, d_offs.cpu().numpy(), d_os.cpu().numpy(), d_info.cpu().numpy(), d_sf.cpu().numpy(), d_st.cpu().numpy()


def test_candidate_overflow_and_retry(gpu):
    m = _mixed(gpu)
    a = np.frombuffer(m["buf"], dtype=np.uint8)
    nsync = int(((a[:-1] == 0xFF) & ((a[1:] >> 2) == 0x3E)).sum())  # bnflac_index_frames' rule
    assert nsync > 4
    b = Batch(gpu, m["buf"], m["table"], m["sp"], cand_cap=4)  # the call returned 0
    assert b.status[0] & 1
    assert b.status[1] == nsync
    assert not b.sf.any()
    _assert_mixed(m, Batch(gpu, m["buf"], m["table"], m["sp"], cand_cap=int(b.status[1])))


def test_frame_cap(gpu):
    torch, libflac, dec = gpu
    m = _mixed(gpu)
    full = Batch(gpu, m["buf"], m["table"], m["sp"])
    rc, offs, os_, info, sf, st = _raw(gpu, full.d_bytes, len(m["buf"]), m["table"], m["sp"], cap=5, nout=8)
    assert rc == 0
    assert st[0] == 2 and st[2] == 23 and sf[-1] == 23
    assert np.array_equal(offs[:5], full.offs[:5]) and np.array_equal(os_[:5], full.os[:5])
    assert info[: 5 * libflac.FRAME_INFO_BYTES].tobytes() == full.rec[:5].tobytes()
    assert (offs[5:] == POISON).all() and (os_[5:] == POISON).all()
    assert (info[5 * libflac.FRAME_INFO_BYTES:] == POISON).all()


def test_bad_table(gpu):
    torch, libflac, dec = gpu
    m = _mixed(gpu)
    t = m["table"]
    with pytest.raises(ValueError):  # overlapping ranges
        dec.index_streams(_upload(torch, m["buf"]), len(m["buf"]), [t[0], (t[1][0] - 1,) + t[1][1:]] + t[2:], m["sp"], 64)
    nbytes = len(m["buf"])
    bad = t[:4] + [(t[4][0], nbytes + 1, t[4][2], t[4][3])]  # end > nbytes
    rc, offs, os_, info, sf, st = _raw(gpu, _upload(torch, m["buf"]), nbytes, bad, m["sp"], cap=64, nout=64)
    assert rc == 0
    assert st[0] & 4 and st[2] == 0 and st[3] == 0
    assert not sf.any()
    assert (offs == POISON).all() and (os_ == POISON).all() and (info == POISON).all()


# ------------------------------------------------------------------ 7. scan seams
def test_scan_seams(gpu):
    """More than 2,048 candidates: every three-launch scan crosses workgroup boundaries."""
    from birdnest.audio_amd import synth
    torch, libflac, dec = gpu
    syn = [synth.encode(synth.config("C4", nframes=600, seed=31 + i)) for i in range(3)]
    datas = [s.data.tobytes() for s in syn]
    buf, ranges = _pack(datas, (9, 0))
    table = [(b, e, b + _first_frame_offset(d), _stream_params(libflac, d).total_samples)
             for (b, e), d in zip(ranges, datas)]
    b = Batch(gpu, buf, table, _stream_params(libflac, datas[0], 0), cap=2048)
    assert b.status[0] == 0
    assert b.status[1] > 2048
    assert np.diff(b.sf).tolist() == [600] * 3
    for s in range(3):
        assert np.array_equal(b.offs[b.stream(s)], syn[s].frame_offsets.astype(np.int64) + table[s][0])
    assert np.array_equal(b.ss, np.concatenate([[0], np.cumsum([len(y.pcm) for y in syn])]))


# ------------------------------------------------------------------ 8. hand-off dropped
def test_drops_the_crc_handoff(gpu):
    torch, libflac, dec = gpu
    m = _mixed(gpu)
    L = libflac.load()
    L.bnflac_debug_set_crc_mode(1)
    L.bnflac_debug_set_parse_wave(0)  # k_parse: the kernel that hands over
    try:
        d_bytes = _upload(torch, m["buf"])
        o = m["syn"][0].frame_offsets.astype(np.int64)
        nf = len(o)
        offs = torch.tensor(o.tolist(), dtype=torch.int64, device="cuda:0")
        d_info = torch.zeros(nf * libflac.FRAME_INFO_BYTES, dtype=torch.uint8, device="cuda:0")
        sp = _stream_params(libflac, m["datas"][0])
        dec.parse_frames(d_bytes, len(m["buf"]), offs, nf, sp, d_info)
        dec.crc_handoff(nf)
        dec.index_streams(d_bytes, len(m["buf"]), m["table"], m["sp"], 64)
        torch.cuda.synchronize()
        with pytest.raises(RuntimeError):
            dec.crc_handoff(nf)
    finally:
        L.bnflac_debug_set_crc_mode(-1)
        L.bnflac_debug_set_parse_wave(-1)
