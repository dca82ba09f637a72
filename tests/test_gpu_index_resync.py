"""bnflac_index_streams_resync: the batched index goes on past a stream's damage.

Every batch is compared with three references: (a) bnflac_resync_plan_host over the device's own
candidate table (bnflac_debug_index_candidates), which pins the kernels to the rule; (b) the
geometry of the damage, from the generator's frame offsets; (c) where stated, the CPU oracle's
deliveries.  Streams are C2 with blocksize 256 (frame-number headers, STREAMINFO min = max = 256).
Everything is exact.  Damaged bytes are ordinary input: no test provokes a device fault.
"""
import ctypes
import os

import numpy as np
import pytest

from tests.conftest import gpu_available
from tests.test_gpu_index_streams import (GOLD, GOLD_DIR, POISON, Batch, _crc16, _first_frame_offset, _pack,
                                          _stream_params, _upload)

pytestmark = pytest.mark.gpu

B = 256
RESYNCED, CONTRADICTION, HEAD, LEADING = 1, 2, 4, 8


@pytest.fixture(scope="module")
def gpu():
    if not gpu_available():
        pytest.skip("no GPU")
    import torch
    from birdnest.audio_amd import libflac
    return torch, libflac, libflac.BatchDecoder(0)


_SYN = {}


def _syn(nframes, seed):
    """One C2 stream of blocksize 256 (made once per shape and seed)."""
    from birdnest.audio_amd import synth
    if (nframes, seed) not in _SYN:
        _SYN[nframes, seed] = synth.encode(synth.config("C2", nframes=nframes, seed=seed, blocksize=B))
    return _SYN[nframes, seed]


def _offsets(s):
    return [int(x) for x in s.frame_offsets] + [int(s.data.size)]


def _damage(s, pattern, f=None):
    """The damage patterns on stream s -> bytes"""
    d, o = bytearray(s.data.tobytes()), _offsets(s)
    if pattern == "body":  # inside frame f's last subframe: its header and walk stay valid
        d[o[f + 1] - 10] ^= 0x10
    elif pattern == "header":
        d[o[f] + 2] ^= 0x10
    elif pattern == "zeros":  # frames f..f+2 overwritten
        d[o[f]:o[f + 3]] = bytes(o[f + 3] - o[f])
    elif pattern == "headers_9_11":
        d[o[9] + 2] ^= 0x10
        d[o[11] + 2] ^= 0x10
    else:
        raise ValueError(pattern)
    return bytes(d)


def _table(libflac, buf_ranges, datas, totals=None, firsts=None):
    out = []
    for k, ((b, e), d) in enumerate(zip(buf_ranges, datas)):
        total = _stream_params(libflac, d).total_samples if totals is None or totals[k] is None else totals[k]
        first = _first_frame_offset(d) if firsts is None or firsts[k] is None else firsts[k]
        out.append((b, e, b + first, total))
    return out


class RBatch:
    """One index_streams_resync call, synchronised and copied to the host, with the candidate table
    the call left behind."""

    def __init__(self, gpu, buf: bytes, table, sp, cap=None, cand_cap=0):
        torch, libflac, dec = gpu
        self.buf, self.table, self.sp = buf, table, sp
        self.d_bytes = _upload(torch, buf)
        self.cap = cap = (len(buf) // 16 + 16) if cap is None else cap
        self.d_offs, self.d_os, self.d_info, d_sf, d_ss, d_st, d_rs = dec.index_streams_resync(
            self.d_bytes, len(buf), table, sp, cap, cand_cap=cand_cap)
        torch.cuda.synchronize()
        self.cands = dec.index_candidates()
        self.sf = d_sf.cpu().numpy().astype(np.int64)
        self.ss = d_ss.cpu().numpy().astype(np.int64)
        self.status = d_st.cpu().numpy().astype(np.int64)
        self.rs = libflac.resync_array(d_rs.cpu().numpy())
        n = self.n = min(int(self.sf[-1]), cap)
        self.offs = self.d_offs[:n].cpu().numpy()
        self.os = self.d_os[:n].cpu().numpy()
        self.rec = libflac.info_array(self.d_info[: n * libflac.FRAME_INFO_BYTES].cpu().numpy())

    def stream(self, s):
        return slice(int(self.sf[s]), int(self.sf[s + 1]))

    def gap(self, s):
        """Per record of stream s: is it a placeholder"""
        return (self.rec["flags"][self.stream(s)] & 0x800) != 0

    def decode(self, gpu):
        """decode_parsed of every record into INTERLEAVED32 -> (pcm [samples, channels], records after)"""
        torch, libflac, dec = gpu
        total, ch = int(self.ss[-1]), self.sp.channels
        d_out = torch.full((total * ch * 4 + 64,), 0xAB, dtype=torch.uint8, device="cuda:0")
        d_info = self.d_info.clone()
        dec.decode_parsed(self.d_bytes, len(self.buf), self.n, self.sp, libflac.OUT_INTERLEAVED32, d_out, d_info)
        torch.cuda.synchronize()
        rec = libflac.info_array(d_info[: self.n * libflac.FRAME_INFO_BYTES].cpu().numpy())
        assert (d_out[total * ch * 4:].cpu().numpy() == 0xAB).all()
        return d_out[: total * ch * 4].cpu().numpy().view("<i4").reshape(-1, ch), rec


def _assert_placeholder(b: RBatch, q: int, next_off: int, position: int, out_sample: int):
    r, sp = b.rec[q], b.sp
    want = np.zeros(1, dtype=r.dtype)[0]
    want["status"], want["err"], want["cached"] = 1, 0, -1
    want["frame_off"], want["blocksize"] = next_off, sp.min_blocksize
    want["sample_rate"], want["channels"], want["bps"] = sp.sample_rate, sp.channels, sp.bps
    want["number"], want["out_sample"] = position // sp.min_blocksize, out_sample
    want["sub_start"][0] = 1
    want["flags"] = 0x800
    assert r.tobytes() == want.tobytes(), (q, r, want)


def assert_plan(gpu, b: RBatch):
    """Reference (a): the device's tables are the host rule's over the device's candidate table."""
    torch, libflac, dec = gpu
    sd = np.array([tuple(t) for t in b.table], dtype=libflac.STREAM_DESC_DTYPE)
    slots, sf, ss, rs, st = libflac.resync_plan_host(b.cands, sd, b.sp.min_blocksize, b.cap)
    assert b.status[1] == len(b.cands) and b.status[0] & 5 == 0
    assert [int(b.status[0]), int(b.status[2]), int(b.status[3])] == [int(st[0]), int(st[2]), int(st[3])]
    assert np.array_equal(b.sf, sf.astype(np.int64)) and np.array_equal(b.ss, ss.astype(np.int64))
    assert b.rs.tobytes() == rs.tobytes()
    assert len(slots) == b.n
    stream_of = np.searchsorted(b.sf[1:], np.arange(b.n), side="right")
    for q, x in enumerate(slots):
        c = b.cands[int(x["cand"])]
        s = int(stream_of[q])
        assert c["stream"] == s
        os_ = int(b.ss[s]) + int(x["position"])
        assert int(b.offs[q]) == int(c["offset"]) and int(b.os[q]) == os_
        if x["gap"]:
            _assert_placeholder(b, q, int(c["offset"]), int(x["position"]), os_)
        else:
            r = b.rec[q]
            assert r["status"] == 0 and r["flags"] & 0x800 == 0
            assert (int(r["frame_off"]), int(r["out_sample"]), int(r["number"]), int(r["blocksize"])) == \
                (int(c["offset"]), os_, int(c["number"]), int(c["blocksize"]))
    # the candidate table itself: offsets are the buffer's sync pairs, owners follow the ranges
    a = np.frombuffer(b.buf, dtype=np.uint8)
    sync = np.flatnonzero((a[:-1] == 0xFF) & ((a[1:] >> 2) == 0x3E))
    assert np.array_equal(b.cands["offset"].astype(np.int64), sync)
    for i, c in enumerate(b.cands):
        own = [s for s, t in enumerate(b.table) if t[0] <= c["offset"] and c["offset"] + 2 <= t[1]]
        assert c["stream"] == (own[0] if own else -1)
        if c["succ"] >= 0:
            assert c["succ"] > i and b.cands[c["succ"]]["stream"] == c["stream"] and c["flags"] & 1


def assert_geometry(b: RBatch, s: int, begin: int, frame_offsets, present, kept=None):
    """Reference (b): stream s holds, position by position, frame k of the generator where present[k]
    and else a placeholder that names the next present frame; kept positions in all."""
    kept = len(present) if kept is None else kept
    sl = b.stream(s)
    assert sl.stop - sl.start == kept
    assert int(b.ss[s + 1] - b.ss[s]) == kept * B
    gap = b.gap(s)
    for k in range(kept):
        q = sl.start + k
        assert int(b.os[q]) == int(b.ss[s]) + k * B
        assert bool(gap[k]) == (not present[k]), (s, k)
        nxt = k if present[k] else min(j for j in range(k, len(present)) if present[j])
        assert int(b.offs[q]) == begin + int(frame_offsets[nxt])
        assert int(b.rec["frame_off"][q]) == begin + int(frame_offsets[nxt])
    assert int(b.rs["gap_frames"][s]) == sum(1 for k in range(kept) if not present[k])


# ------------------------------------------------------------------ 1. intact parity
def test_intact_parity(gpu):
    """Mixed sizes, an empty stream, junk behind a stream, a total inside a frame and a first_offset
    inside frame 0 of an unknown-length stream: byte for byte what bnflac_index_streams writes."""
    torch, libflac, dec = gpu
    syn = [_syn(nf, 11 + 7 * i) if nf else None for i, nf in enumerate((12, 1, 7, 0, 3))]
    datas = [s.data.tobytes() if s else b"" for s in syn]
    datas[2] += b"\xff"
    whole = _syn(12, 22)
    fo = _offsets(whole)
    k = 6
    datas += [whole.data.tobytes()] * 2
    buf, ranges = _pack(datas, (0, 5, 16, 33, 1, 0))
    totals = [None if d else 0 for d in datas[:5]] + [k * B + 1, 0]          # ends inside frame k; unknown
    firsts = [None if d else 0 for d in datas[:5]] + [None, fo[0] + 1]       # starts inside frame 0
    table = _table(libflac, ranges, datas, totals, firsts)
    sp = _stream_params(libflac, datas[0], 0)
    want = Batch(gpu, buf, table, sp)
    assert np.diff(want.sf).tolist() == [12, 1, 7, 0, 3, k + 1, 11]  # the plain index handles all of it
    b = RBatch(gpu, buf, table, sp)
    assert_plan(gpu, b)
    assert np.array_equal(b.sf, want.sf) and np.array_equal(b.ss, want.ss.astype(np.int64))
    assert b.status.tolist() == want.status.tolist() and b.status[0] == 0 and b.status[3] == 0
    assert np.array_equal(b.offs, want.offs) and np.array_equal(b.os, want.os)
    assert b.rec.tobytes() == want.rec.tobytes()
    assert b.rs["segments"].tolist() == [1, 1, 1, 0, 1, 1, 1]
    assert b.rs["base"].tolist() == [0, 0, 0, 0, 0, 0, B]
    for f in ("flags", "gap_frames", "reserved", "gap_samples"):
        assert not b.rs[f].any(), f


# ------------------------------------------------------------------ 2. test_damage_is_local's corpus
def _damage_is_local(libflac):
    from birdnest.audio_amd import synth
    syn = [synth.encode(synth.config("C2", nframes=12, seed=21 + i)) for i in range(3)]
    datas = [bytearray(s.data.tobytes()) for s in syn]
    o = [int(x) for x in syn[1].frame_offsets]
    datas[1][o[6] - 10] ^= 0x10
    assert _crc16(bytes(datas[1][o[5]:o[6]])) != 0
    datas = [bytes(d) for d in datas]
    buf, ranges = _pack(datas, (7, 2))
    return syn, datas, buf, ranges, _table(libflac, ranges, datas)


def test_damage_is_local_keeps_every_frame(gpu):
    torch, libflac, dec = gpu
    syn, datas, buf, ranges, table = _damage_is_local(libflac)
    sp = _stream_params(libflac, datas[0], 0)
    assert sp.min_blocksize == sp.max_blocksize  # the generator's own blocksize, fixed
    b = RBatch(gpu, buf, table, sp)
    assert_plan(gpu, b)
    assert np.diff(b.sf).tolist() == [12, 12, 12]
    for s in range(3):
        assert np.array_equal(b.offs[b.stream(s)], syn[s].frame_offsets.astype(np.int64) + table[s][0])
    assert not (b.rec["flags"] & 0x800).any() and b.status[3] == 0
    assert b.rs["segments"].tolist() == [1, 2, 1] and b.rs["flags"].tolist() == [0, RESYNCED, 0]
    assert b.status[0] == 8
    pcm, rec = b.decode(gpu)
    bad = int(b.sf[1]) + 5
    assert rec["crc_ok"][bad] == 0 and rec["status"][bad] == 0
    assert (np.delete(rec["crc_ok"], bad) == 1).all() and (rec["status"] == 0).all()
    want = np.concatenate([y.pcm for y in syn])
    lo = int(b.os[bad])
    hi = lo + int(rec["blocksize"][bad])
    assert not pcm[lo:hi].any()
    want[lo:hi] = 0
    assert np.array_equal(pcm, want)


# ------------------------------------------------------------------ 3. oracle parity
PATTERNS = [("body", 5, list(range(12)), 12),  # all 12 delivered, frame 5 as zeros
            ("header", 5, [k for k in range(12) if k != 5], 12),
            ("zeros", 4, [0, 1, 2, 3, 7, 8, 9, 10, 11], 12),
            ("header", 0, list(range(1, 12)), 12),
            ("headers_9_11", None, list(range(9)) + [10], 9)]  # frame 10 is not resumed at: T = 9 * 256


def test_oracle_parity(gpu):
    import oracle
    torch, libflac, dec = gpu
    s = _syn(12, 22)
    fo = _offsets(s)
    datas = [_damage(s, p, f) for p, f, _, _ in PATTERNS]
    placed = []
    for d, (p, f, delivered, _) in zip(datas, PATTERNS):
        ev, opcm = oracle.run(d)
        writes = [e for e in ev if e.kind == oracle.EV_WRITE]
        # a condition on the input: the oracle delivers exactly these frames, each at its header's number
        assert [e.sample_number for e in writes] == [k * B for k in delivered], p
        assert all(e.blocksize == B for e in writes)
        frames = {e.sample_number // B: opcm[e.pcm_offset: e.pcm_offset + B * e.channels].reshape(e.channels, B).T
                  for e in writes}
        if p == "body":
            assert not frames[5].any() and sum(e.kind == oracle.EV_ERROR for e in ev) == 1
        placed.append(frames)
    buf, ranges = _pack(datas, (3, 0, 9, 1))
    table = _table(libflac, ranges, datas)
    sp = _stream_params(libflac, datas[0], 0)
    b = RBatch(gpu, buf, table, sp)
    assert_plan(gpu, b)
    pcm, rec = b.decode(gpu)
    for n, ((p, f, delivered, kept), frames) in enumerate(zip(PATTERNS, placed)):
        present = [k in delivered for k in range(12)]
        assert_geometry(b, n, table[n][0], fo, present, kept)
        T = int(b.ss[n + 1] - b.ss[n])
        assert T == kept * B
        want = np.zeros((T, sp.channels), np.int32)
        for k, fr in frames.items():
            if k < kept:
                want[k * B:(k + 1) * B] = fr
        assert np.array_equal(pcm[int(b.ss[n]): int(b.ss[n + 1])], want), p
        gap = b.gap(n)
        st = rec["status"][b.stream(n)]
        assert np.array_equal(st != 0, gap)  # only the placeholders fail to decode
    assert b.rs["flags"].tolist() == [RESYNCED, RESYNCED, RESYNCED, LEADING, 0]
    assert b.rs["segments"].tolist() == [2, 2, 2, 1, 1]
    assert b.status[0] == 8 and b.status[3] == 0 + 1 + 3 + 1 + 0


# ------------------------------------------------------------------ 4. contradiction
def test_contradiction_ends_the_chain(gpu):
    torch, libflac, dec = gpu
    s = _syn(12, 22)
    fo = _offsets(s)
    d = bytearray(s.data.tobytes()[: fo[7]])
    d[fo[6] + 2] ^= 0x10  # frame 6's header
    d += s.data.tobytes()[fo[3]:]  # frames 3..11 again: their numbers go back
    buf, ranges = _pack([bytes(d)], ())
    table = _table(libflac, ranges, [bytes(d)])
    b = RBatch(gpu, buf, table, _stream_params(libflac, bytes(d), 0))
    assert_plan(gpu, b)
    assert_geometry(b, 0, 0, fo, [True] * 6, 6)
    assert int(b.ss[1]) == 6 * B and b.rs["flags"][0] == CONTRADICTION and b.rs["segments"][0] == 1
    assert b.status[0] == 16 and b.status[3] == 0


# ------------------------------------------------------------------ 5. rebase
def test_unknown_length_is_rebased(gpu):
    torch, libflac, dec = gpu
    s = _syn(12, 22)
    d = _damage(s, "header", 0)
    buf, ranges = _pack([d], ())
    table = _table(libflac, ranges, [d], totals=[0])
    sp = _stream_params(libflac, d, 0)
    want = Batch(gpu, buf, table, sp)
    assert np.diff(want.sf).tolist() == [11]
    b = RBatch(gpu, buf, table, sp)
    assert_plan(gpu, b)
    assert b.rs["base"][0] == B and b.rs["flags"][0] == 0 and b.status[3] == 0 and b.status[0] == 0
    assert not (b.rec["flags"] & 0x800).any()
    assert np.array_equal(b.sf, want.sf) and np.array_equal(b.ss, want.ss.astype(np.int64))
    assert np.array_equal(b.offs, want.offs) and np.array_equal(b.os, want.os)
    assert b.rec.tobytes() == want.rec.tobytes()


# ------------------------------------------------------------------ 6. scan seams
def _sync_pairs(d: bytes):
    a = np.frombuffer(d, dtype=np.uint8)
    return np.flatnonzero((a[:-1] == 0xFF) & ((a[1:] >> 2) == 0x3E))


def seam_corpus():
    """60 streams of 40 frames; the damage plan {stream: (pattern, frame)}: the first and the last
    stream, and the streams whose candidates straddle indices 1,024 and 2,048, at the frames whose
    candidates sit at those indices -> (syn, datas, plan, buf, ranges)"""
    syn = [_syn(40, 300 + i) for i in range(60)]
    clean = [s.data.tobytes() for s in syn]
    gaps = tuple((7 * i) % 40 for i in range(59))
    buf, ranges = _pack(clean, gaps)  # the damage changes no length: the ranges stay
    cand = _sync_pairs(buf)  # the filler holds sync pairs too
    assert len(cand) > 2048
    plan = {0: ("header", 5), 59: ("zeros", 4)}
    for seam, pattern in ((1024, "zeros"), (2048, "header")):
        at = int(cand[seam])
        s = [k for k, (b, e) in enumerate(ranges) if b <= at < e][0]
        assert s not in plan
        f = int(np.searchsorted(syn[s].frame_offsets.astype(np.int64), at - ranges[s][0], side="right")) - 1
        plan[s] = (pattern, min(max(f, 1), 36))
    datas = [_damage(syn[s], *plan[s]) if s in plan else clean[s] for s in range(60)]
    buf, ranges = _pack(datas, gaps)
    # a condition on the input: in the damaged buffer the two seams still lie inside damaged streams
    cand = _sync_pairs(buf)
    for seam in (1024, 2048):
        owner = [s for s, (b, e) in enumerate(ranges) if b <= cand[seam] and cand[seam] + 2 <= e]
        assert owner and owner[0] in plan and owner[0] not in (0, 59), seam
    return syn, datas, plan, buf, ranges


def test_scan_seams(gpu):
    """About 2,500 candidates: three workgroups of every 1,024-wide scan (seam_corpus)."""
    torch, libflac, dec = gpu
    syn, datas, plan, buf, ranges = seam_corpus()
    table = _table(libflac, ranges, datas)
    sp = _stream_params(libflac, datas[0], 0)
    b = RBatch(gpu, buf, table, sp)
    assert b.status[1] > 2048
    assert_plan(gpu, b)
    for seam in (1024, 2048):
        assert int(b.cands["stream"][seam]) in plan
    for s in range(60):
        lost = set()
        if s in plan:
            p, f = plan[s]
            lost = {f} if p == "header" else {f, f + 1, f + 2}
        assert_geometry(b, s, table[s][0], _offsets(syn[s]), [k not in lost for k in range(40)])
        assert b.rs["flags"][s] == (RESYNCED if s in plan else 0)
    assert b.status[0] == 8 and b.status[3] == 1 + 3 + 3 + 1
    assert np.array_equal(b.ss, np.arange(61) * 40 * B)


# ------------------------------------------------------------------ 7. a long gap, and cap below the total
def _raw(gpu, d_bytes, nbytes, table, sp, cap, nout):
    """The C call itself on poisoned outputs of nout entries -> rc and host copies"""
    torch, libflac, dec = gpu
    dev, n = "cuda:0", len(table)
    tab = np.array([tuple(t) for t in table], dtype=libflac.STREAM_DESC_DTYPE)
    d_tab = torch.from_numpy(tab.view(np.int64).reshape(-1).copy()).to(dev)
    d_offs = torch.full((nout,), POISON, dtype=torch.int64, device=dev)
    d_os = torch.full((nout,), POISON, dtype=torch.int64, device=dev)
    d_info = torch.full((nout * libflac.FRAME_INFO_BYTES,), POISON, dtype=torch.uint8, device=dev)
    d_sf = torch.full((n + 2,), POISON, dtype=torch.int32, device=dev)
    d_ss = torch.full((n + 2,), POISON, dtype=torch.int64, device=dev)
    d_rs = torch.full(((n + 1) * libflac.RESYNC_REC_BYTES,), POISON, dtype=torch.uint8, device=dev)
    d_st = torch.full((5,), POISON, dtype=torch.int32, device=dev)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = dec.L.bnflac_index_streams_resync(dec.ctx, vp(d_bytes), nbytes, vp(d_tab), n, ctypes.byref(sp), 0, vp(d_offs),
                                           vp(d_os), vp(d_info), cap, vp(d_sf), vp(d_ss), vp(d_rs), vp(d_st),
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, [t.cpu().numpy() for t in (d_offs, d_os, d_info, d_sf, d_ss, d_rs, d_st)]


def test_long_gap_and_cap(gpu):
    """Frames 50..1,150 of 1,200 zeroed: 1,101 placeholders from one gap, several workgroups of output
    positions that all find the same candidate."""
    torch, libflac, dec = gpu
    s = _syn(1200, 77)
    fo = _offsets(s)
    d = bytearray(s.data.tobytes())
    d[fo[50]:fo[1151]] = bytes(fo[1151] - fo[50])
    d = bytes(d)
    buf, ranges = _pack([d], ())
    table = _table(libflac, ranges, [d])
    sp = _stream_params(libflac, d, 0)
    b = RBatch(gpu, buf, table, sp)
    assert_plan(gpu, b)
    present = [not 50 <= k <= 1150 for k in range(1200)]
    assert_geometry(b, 0, 0, fo, present)
    assert b.status[3] == 1101 and b.status[2] == 1200 and b.status[0] == 8
    assert b.rs["gap_samples"][0] == 1101 * B and b.rs["segments"][0] == 2
    assert np.array_equal(b.rec["number"][50:1151], np.arange(50, 1151))
    pcm, rec = b.decode(gpu)
    want = s.pcm.copy()
    want[50 * B: 1151 * B] = 0
    assert np.array_equal(pcm, want)
    # cap inside the gap: the tables hold the true totals, nothing past cap is written
    cap, nout = 700, 720
    rc, (offs, os_, info, sf, ss, rs, st) = _raw(gpu, b.d_bytes, len(buf), table, sp, cap, nout)
    assert rc == 0
    assert st[:4].tolist() == [8 | 2, int(b.status[1]), 1200, 1101] and st[4] == POISON
    assert sf[:2].tolist() == [0, 1200] and ss[:2].tolist() == [0, 1200 * B]
    assert np.array_equal(offs[:cap], b.offs[:cap]) and np.array_equal(os_[:cap], b.os[:cap])
    assert info[: cap * libflac.FRAME_INFO_BYTES].tobytes() == b.rec[:cap].tobytes()
    assert rs[: libflac.RESYNC_REC_BYTES].tobytes() == b.rs.tobytes()
    for a in (offs[cap:], os_[cap:], info[cap * libflac.FRAME_INFO_BYTES:], sf[2:], ss[2:],
              rs[libflac.RESYNC_REC_BYTES:]):
        assert (a == POISON).all()


# ------------------------------------------------------------------ 8. refusal
def test_variable_blocksize_is_refused(gpu):
    torch, libflac, dec = gpu
    g = GOLD["c4_mixed_varbs"]
    data = open(os.path.join(GOLD_DIR, g["file"]), "rb").read()
    sp = _stream_params(libflac, data)
    assert sp.min_blocksize != sp.max_blocksize
    table = [(0, len(data), _first_frame_offset(data), sp.total_samples)]
    rc, outs = _raw(gpu, _upload(torch, data), len(data), table, sp, 64, 64)
    assert rc < 0 and dec.L.bnflac_last_error()
    for a in outs:
        assert (a == POISON).all()
    with pytest.raises(ValueError):
        dec.index_streams_resync(_upload(torch, data), len(data), table, sp, 64)
    with pytest.raises(ValueError):
        dec.index_corpus(_upload(torch, data), len(data), [(0, len(data))], sp, resync=True)
    nosi = libflac.StreamParams(0, B, B, sp.sample_rate, sp.channels, sp.bps, 0)
    rc, outs = _raw(gpu, _upload(torch, data), len(data), table, nosi, 64, 64)
    assert rc < 0
    for a in outs:
        assert (a == POISON).all()


# ------------------------------------------------------------------ 9. end to end
def _crops(gpu, corpus, reqs, nsamples, shared):
    torch, libflac, dec = gpu
    rows, status = dec.decode_crops(corpus, reqs, nsamples, libflac.OUT_INTERLEAVED32, shared=shared, health=True)
    torch.cuda.synchronize()
    return rows.cpu().numpy(), libflac.health_array(status["windows_health"].cpu().numpy()), status


def _md5_verdicts(gpu, corpus, ranges):
    """Whole-corpus decode of a copy of the records, then md5_streams against STREAMINFO's sums."""
    torch, libflac, dec = gpu
    sp = corpus.sp
    ss = corpus.d_stream_samples.cpu().numpy()
    nf = int(corpus.d_stream_frames.cpu().numpy()[-1])
    d_info = corpus.d_info.clone()
    d_out = torch.zeros(int(ss[-1]) * sp.channels * 4 + 64, dtype=torch.uint8, device="cuda:0")
    dec.decode_parsed(corpus.d_bytes, corpus.nbytes, nf, sp, libflac.OUT_INTERLEAVED32, d_out, d_info)
    _, _, d_md5, _ = dec.scan_streams(corpus.d_bytes, corpus.nbytes, ranges, expect=sp)
    _, d_verdict, _ = dec.md5_streams(d_out, libflac.OUT_INTERLEAVED32, sp, corpus.d_stream_samples, corpus.nstreams,
                                      d_expected=d_md5.reshape(-1), pcm_bytes=int(ss[-1]) * sp.channels * 4)
    torch.cuda.synchronize()
    return d_verdict.cpu().numpy().tolist()


@pytest.mark.parametrize("shared", [False, True])
def test_crops_behind_the_damage(gpu, shared):
    torch, libflac, dec = gpu
    # test 2's corpus: stream 1's frame 5 fails its CRC-16
    syn, datas, buf, ranges, table = _damage_is_local(libflac)
    sp = _stream_params(libflac, datas[0], 0)
    bs = sp.min_blocksize
    d_bytes = _upload(torch, buf)
    plain = dec.index_corpus(d_bytes, len(buf), ranges, sp)
    corpus = dec.index_corpus(d_bytes, len(buf), ranges, sp, resync=True)
    assert plain.d_resync is None and corpus.d_resync is not None
    n = 300
    lost = min(n, bs - 10)
    reqs = [(1, 5 * bs + 10), (1, 8 * bs + 5), (0, 3 * bs), (1, 12 * bs - n), (2, 0)]
    rows, health, status = _crops(gpu, corpus, reqs, n, shared)
    for k, (s, lo) in enumerate(reqs):
        want = syn[s].pcm[lo: lo + n].copy()
        if k == 0:
            want[: lost] = 0  # what the crop holds of frame 5
        assert np.array_equal(rows[k], want), k
    assert health["flags"].tolist() == [libflac.HEALTH_DAMAGED, 0, 0, 0, 0]
    assert (int(health["bad_frames"][0]), int(health["crc_frames"][0]), int(health["bad_samples"][0])) == (1, 1, lost)
    assert not health["missing"].any()
    # without resync the same crops behind the damage are SHORT and empty
    rows0, health0, _ = _crops(gpu, plain, reqs, n, shared)
    assert health0["flags"][1] & libflac.HEALTH_SHORT and not rows0[1].any()
    assert _md5_verdicts(gpu, corpus, ranges) == [0, 1, 0]

    # frames 4..6 zeroed: three placeholders
    s = _syn(12, 22)
    d = _damage(s, "zeros", 4)
    d_bytes = _upload(torch, d)
    sp = _stream_params(libflac, d, 0)
    corpus = dec.index_corpus(d_bytes, len(d), [(0, len(d))], sp, resync=True)
    n = 700
    reqs = [(0, 3 * B + 100), (0, 7 * B + 3), (0, 0), (0, 12 * B - n)]
    rows, health, status = _crops(gpu, corpus, reqs, n, shared)
    pcm = s.pcm.copy()
    pcm[4 * B: 7 * B] = 0
    for k, (_, lo) in enumerate(reqs):
        assert np.array_equal(rows[k], pcm[lo: lo + n]), k
    assert health["flags"].tolist() == [libflac.HEALTH_DAMAGED, 0, 0, 0]
    assert (int(health["bad_frames"][0]), int(health["crc_frames"][0])) == (3, 0)
    assert int(health["bad_samples"][0]) == min(3 * B + 100 + n, 7 * B) - 4 * B
    assert not health["missing"].any()
    rs = libflac.resync_array(corpus.d_resync.cpu().numpy())
    assert rs["gap_frames"].tolist() == [3] and rs["flags"].tolist() == [RESYNCED]
    assert _md5_verdicts(gpu, corpus, [(0, len(d))]) == [1]
