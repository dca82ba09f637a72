"""k_parse's residual walk with its ring refilled in 64-byte groups (pk_refill), and the frame's
first CRC line read only inside the 16-byte-rounded buffer.

Everything is checked against sources that do not depend on the walk: the PCM against the
generator's source and the CPU oracle, the header fields and the frame's end against the oracle's
frame decode, and sub_start[1] -- what the walk is for -- against a bit walk of channel 0 written
here in Python (which proves itself on every frame it walks: continued over channel 1, it must end
on the frame's footer).  The records must also be those of k_parse_wave, which the change does not
touch.

The shapes are the smallest at which the refill can go wrong: a frame whose channel 0 ends in the
buffer's last 64-byte group with the device buffer exactly round_up(nbytes, 16) long (the clamped
form of the group fetch), lanes of one wave that consume their rings at very different rates,
cursors that jump (escaped partitions, VERBATIM), frames of very different lengths in one launch,
and the CRC-16 hand-off on each of its paths."""
import json
import os

import numpy as np
import pytest

from tests.conftest import gpu_available

pytestmark = pytest.mark.gpu

GOLD_DIR = os.path.join(os.path.dirname(__file__), "golden")
GOLD = json.load(open(os.path.join(GOLD_DIR, "golden.json")))
BLK_REFILL = 0x800000  # include/bnflac.h: the walk refills block by block (br_refill), an exact A/B switch
ST_TRUNC = 2


@pytest.fixture(scope="module")
def gpu():
    if not gpu_available():
        pytest.skip("no GPU")
    import torch
    from birdnest.audio_amd import libflac
    dec = libflac.BatchDecoder(0)
    L = dec.L
    L.bnflac_debug_set_decode_sys(0)   # the lane kernels: k_decode_st reads sub_start[1] and the hand-off
    L.bnflac_debug_set_parse_wave(0)   # the lane-per-frame k_parse (small batches otherwise take k_parse_wave)
    L.bnflac_debug_set_crc_mode(1)
    yield torch, libflac, dec
    L.bnflac_debug_set_ablate(0)
    L.bnflac_debug_set_crc_mode(-1)
    L.bnflac_debug_set_parse_wave(-1)
    L.bnflac_debug_set_decode_sys(-1)


# ------------------------------------------------------------------ an independent bit walk
class _Bits:
    def __init__(self, frame: bytes):
        self.b = np.unpackbits(np.frombuffer(frame, dtype=np.uint8))
        self.ones = np.flatnonzero(self.b)
        self.pos = 0
        self.i = 0  # first entry of ones at or after pos (kept up by unary)

    def read(self, n):
        v = 0
        for x in self.b[self.pos:self.pos + n]:
            v = (v << 1) | int(x)
        self.pos += n
        return v

    def unary(self):
        ones, i, p = self.ones, self.i, self.pos
        while ones[i] < p:
            i += 1
        q = int(ones[i]) - p
        self.i, self.pos = i, p + q + 1
        return q


def _walk_subframe(r, bs, bps):
    assert r.read(1) == 0
    ty = r.read(6)
    if r.read(1):
        bps -= r.unary() + 1
    if ty == 0:
        r.pos += bps
        return
    if ty == 1:
        r.pos += bps * bs
        return
    if 8 <= ty <= 12:
        order = ty - 8
        r.pos += order * bps
    else:
        assert ty >= 32, ty
        order = (ty & 31) + 1
        r.pos += order * bps
        prec = r.read(4) + 1
        r.pos += 5 + order * prec
    plen = 5 if r.read(2) else 4
    porder = r.read(4)
    for p in range(1 << porder):
        cnt = (bs >> porder) - (order if p == 0 else 0)
        k = r.read(plen)
        if k == (1 << plen) - 1:
            nb = r.read(5)  # escaped: cnt raw values of nb bits
            r.pos += nb * cnt
        else:
            for _ in range(cnt):
                r.unary()
                r.pos += k


def _walk_frame(data: bytes, off: int, end: int):
    """-> (bit offset of subframe 1 from the frame's start, blocksize) of the 16-bit stereo frame
    data[off:end]; asserts that the walk of both channels ends on the footer at `end`."""
    r = _Bits(data[off:end])
    assert r.read(14) == 0x3FFE
    r.pos += 2
    bsc, src = r.read(4), r.read(4)
    asg, bpc = r.read(4), r.read(3)
    assert bpc == 4 and asg in (1, 8, 9, 10), (bpc, asg)
    r.pos += 1
    n = (r.read(8) << 1) & 0x1FF  # the frame / sample number: 0xxxxxxx, or L ones for L - 1 more bytes
    while n & 0x180 == 0x180:
        r.pos += 8
        n = (n << 1) & 0x1FF
    if bsc == 6:
        bs = r.read(8) + 1
    elif bsc == 7:
        bs = r.read(16) + 1
    else:
        bs = 192 if bsc == 1 else (576 << (bsc - 2)) if bsc <= 5 else (256 << (bsc - 8))
    r.pos += {12: 8, 13: 16, 14: 16}.get(src, 0) + 8
    _walk_subframe(r, bs, 16 + (asg == 9))
    sub1 = r.pos
    _walk_subframe(r, bs, 16 + (asg in (8, 10)))
    assert (r.pos + 7) // 8 + 2 == end - off, (off, r.pos, end - off)
    return sub1, bs


def _first_rice_param(data: bytes, off: int):
    """Rice parameter of the first partition of channel 0 (an LPC subframe of a fixed-blocksize
    16-bit frame with a one-byte frame number, as the generator's C2 shape writes it)."""
    r = _Bits(data[off:off + 64])
    r.pos = 6 * 8 + 1
    ty = r.read(6)
    assert ty >= 32 and r.read(1) == 0
    order = (ty & 31) + 1
    r.pos += order * 16
    prec = r.read(4) + 1
    r.pos += 5 + order * prec + 2 + 4
    return r.read(4)


# ------------------------------------------------------------------ decode + checks
def _sp(libflac, data, total=None):
    si = data[8:42]
    x = int.from_bytes(si[10:18], "big")
    return libflac.StreamParams(1, int.from_bytes(si[0:2], "big"), int.from_bytes(si[2:4], "big"), x >> 44,
                                ((x >> 41) & 7) + 1, ((x >> 36) & 31) + 1,
                                x & ((1 << 36) - 1) if total is None else total)


def _decode(gpu, data, offs, sp, out_sample, total, crc_mode=1, ablate=0, nbytes=None, parse_wave=0):
    """One batch decode (FLACDecoder's 16-bit layout) of `data`, the device buffer exactly
    round_up(nbytes, 16) bytes long: what the API asks for and no more."""
    torch, libflac, dec = gpu
    dev = torch.device("cuda:0")
    n = len(data) if nbytes is None else nbytes
    d_bytes = torch.zeros((n + 15) // 16 * 16, dtype=torch.uint8, device=dev)
    d_bytes[:n] = torch.frombuffer(bytearray(data[:n]), dtype=torch.uint8).to(dev)
    d_offs = torch.tensor([int(o) for o in offs], dtype=torch.int64, device=dev)
    d_os = torch.tensor([int(o) for o in out_sample], dtype=torch.int64, device=dev)
    stride = libflac.out_stride(libflac.OUT_FLACDECODER, sp)
    d_out = torch.full((total * stride,), 0xAB, dtype=torch.uint8, device=dev)
    d_info = torch.zeros(len(offs) * libflac.FRAME_INFO_BYTES, dtype=torch.uint8, device=dev)
    dec.L.bnflac_debug_set_crc_mode(crc_mode)
    dec.L.bnflac_debug_set_parse_wave(parse_wave)
    dec.L.bnflac_debug_set_ablate(ablate)
    try:
        dec.decode_frames(d_bytes, n, d_offs, len(offs), sp, libflac.OUT_FLACDECODER, d_out, d_info, d_out_sample=d_os)
        torch.cuda.synchronize()
    finally:
        dec.L.bnflac_debug_set_ablate(0)
        dec.L.bnflac_debug_set_parse_wave(0)
        dec.L.bnflac_debug_set_crc_mode(1)
    return libflac.info_array(d_info.cpu().numpy()), d_out.cpu().numpy()


def _check_records(data, offs, ends, info, walk=None):
    """Every record OK with a checked CRC-16; the header fields and the frame's end against the
    oracle's decode of that frame; sub_start[1] against the Python walk (frames in `walk`)."""
    import oracle
    assert (info["status"] == 0).all() and (info["crc_ok"] == 1).all(), info[["status", "err", "crc_ok"]]
    for i, o in enumerate(offs):
        rc, res, _ = oracle.decode_frame_at(data, int(o), None)
        assert rc == 0 and res.crc_ok == 1, (i, rc)
        for name in ("blocksize", "sample_rate", "channels", "assignment", "bps", "number_type", "number"):
            assert int(info[name][i]) == int(getattr(res, name)), (i, name)
        assert int(info["frame_off"][i]) == int(o)
        assert int(info["resume_bit"][i]) == 8 * int(res.end_off) == 8 * int(ends[i]), i
        assert int(info["crc16_read"][i]) == int.from_bytes(data[ends[i] - 2:ends[i]], "big"), i
        assert int(info["crc16_calc"][i]) == oracle.crc16(data[int(o):ends[i] - 2]), i
    for i in (range(len(offs)) if walk is None else walk):
        sub1, bs = _walk_frame(data, int(offs[i]), int(ends[i]))
        assert int(info["sub_start"][i][1]) == sub1 and int(info["blocksize"][i]) == bs, (i, sub1)


def _pcm16(pcm):
    return (np.asarray(pcm).astype(np.int64) & 0xFFFF).astype("<u2").tobytes()


def _same_records(a, b, but=()):
    for name in a.dtype.names:
        if name not in but:
            assert np.array_equal(a[name], b[name]), name


def _stream(cfg="C2", **kw):
    from birdnest.audio_amd import synth
    s = synth.encode(synth.config(cfg, **({"last_blocksize": 0} | kw)))
    data = s.data.tobytes()
    offs = [int(x) for x in s.frame_offsets]
    return s, data, offs, offs[1:] + [len(data)]


def _whole(gpu, s, data, offs, ends, walk=None, **kw):
    """Decode the whole stream, check records and PCM (source and oracle), and the same records
    from k_parse_wave and from the block-by-block refill."""
    import oracle
    torch, libflac, dec = gpu
    sp = _sp(libflac, data)
    ev, opcm = oracle.run(data)
    want = oracle.interleave(ev, opcm)
    assert np.array_equal(want, s.pcm)
    starts = np.concatenate([[0], np.cumsum([e.blocksize for e in ev if e.kind == oracle.EV_WRITE])])[:len(offs)]
    info, out = _decode(gpu, data, offs, sp, starts, s.nsamples, **kw)
    _check_records(data, offs, ends, info, walk)
    assert out.tobytes() == _pcm16(s.pcm)
    info_w, out_w = _decode(gpu, data, offs, sp, starts, s.nsamples, parse_wave=1, **kw)
    _same_records(info, info_w)
    info_b, out_b = _decode(gpu, data, offs, sp, starts, s.nsamples, ablate=BLK_REFILL, **kw)
    _same_records(info, info_b)
    assert out_w.tobytes() == out_b.tobytes() == out.tobytes()
    return info


# ------------------------------------------------------------------ the buffer's end
@pytest.fixture(scope="module")
def end_stream():
    """Four frames of blocksize 1152, LPC-8; the last frame's channel 1 replaced by a CONSTANT
    subframe (3 bytes), so channel 0's walk runs into the buffer's last 64 bytes.  The splice
    point comes from the Python walk; the footer is the oracle's CRC-16."""
    import oracle
    s, data, offs, ends = _stream(nframes=4, blocksize=1152, seed=61)
    o = offs[-1]
    sub1, bs = _walk_frame(data, o, ends[-1])
    assert bs == 1152
    cval = -1234
    bits = np.unpackbits(np.frombuffer(data[o:ends[-1]], dtype=np.uint8))[:sub1]
    tail = np.unpackbits(np.frombuffer(bytes([0x00]) + (cval & 0xFFFF).to_bytes(2, "big"), dtype=np.uint8))
    fr = np.packbits(np.concatenate([bits, tail])).tobytes()
    fr += oracle.crc16(fr).to_bytes(2, "big")
    assert len(fr) - (sub1 // 8) <= 8
    pcm = s.pcm.copy()
    pcm[3 * 1152:, 1] = cval
    return data[:o] + fr, offs, ends[:-1] + [o + len(fr)], pcm


def _shifted(end_stream, rem):
    """The stream behind leading junk such that nbytes % 64 == rem (the header stays at 0:
    the junk follows STREAMINFO, where nothing reads it)."""
    data, offs, ends, pcm = end_stream
    pad = (rem - len(data)) % 64
    d = data[:offs[0]] + bytes([0x5A, 0x00, 0x13, 0x7E] * 16)[:pad] + data[offs[0]:]
    assert len(d) % 64 == rem
    return d, [x + pad for x in offs], [x + pad for x in ends], pcm


def _end_case(gpu, end_stream, rem, **kw):
    torch, libflac, dec = gpu
    d, offs, ends, pcm = _shifted(end_stream, rem)
    sp = _sp(libflac, d)
    info, out = _decode(gpu, d, offs, sp, [1152 * i for i in range(len(offs))], len(pcm), **kw)
    return d, offs, ends, pcm, info, out


@pytest.mark.parametrize("rem", [0, 1, 16, 17, 48, 63])
def test_buffer_end_clamped_group(gpu, end_stream, rem):
    d, offs, ends, pcm, info, out = _end_case(gpu, end_stream, rem)
    _check_records(d, offs, ends, info)
    assert out.tobytes() == _pcm16(pcm)
    ch1 = offs[-1] + int(info["sub_start"][-1][1]) // 8
    assert len(d) - ch1 <= 8  # channel 0 ends in the buffer's last bytes


@pytest.mark.parametrize("rem", [1, 9, 16])
def test_short_frame_ends_the_buffer(gpu, rem):
    """A last frame of 16 samples (under 100 bytes): the line its prefix starts from is the
    line the buffer ends in, 1..16 bytes into it."""
    s, data, offs, ends = _stream(nframes=3, blocksize=1152, last_blocksize=16, seed=62)
    pad = (rem - len(data)) % 64
    d = data[:offs[0]] + bytes([0x13, 0x00, 0x5A, 0x7E] * 16)[:pad] + data[offs[0]:]
    offs, ends = [x + pad for x in offs], [x + pad for x in ends]
    assert len(d) % 64 == rem and ends[-1] - offs[-1] < 100
    torch, libflac, dec = gpu
    for mode in (0, 1, 2):
        info, out = _decode(gpu, d, offs, _sp(libflac, d), [0, 1152, 2304], s.nsamples, crc_mode=mode)
        _check_records(d, offs, ends, info)
        assert out.tobytes() == _pcm16(s.pcm)


@pytest.mark.parametrize("rem", [0, 1, 16, 17, 48, 63])
def test_crc_handoff_modes_agree_at_buffer_end(gpu, end_stream, rem):
    """CRC modes 0, 1 and 2: identical records and PCM, clean and with frame 1 damaged in channel 1
    (past the prefix k_parse folds), which every mode rejects and zero-fills."""
    runs = [_end_case(gpu, end_stream, rem, crc_mode=m) for m in (0, 1, 2)]
    d, offs, ends, pcm = runs[0][:4]
    _check_records(d, offs, ends, runs[0][4])
    for r in runs[1:]:
        _same_records(runs[0][4], r[4])
        assert r[5].tobytes() == runs[0][5].tobytes() == _pcm16(pcm)
    bad = bytearray(d)
    bad[ends[1] - 40] ^= 0x08
    torch, libflac, dec = gpu
    sp = _sp(libflac, d)
    outs = [_decode(gpu, bytes(bad), offs, sp, [1152 * i for i in range(4)], len(pcm), crc_mode=m) for m in (0, 1, 2)]
    want = pcm.copy()
    want[1152:2304] = 0
    for info, out in outs:
        assert info["status"].tolist() == [0, 0, 0, 0] and info["crc_ok"].tolist() == [1, 0, 1, 1]
        _same_records(outs[0][0], info)
        assert out.tobytes() == _pcm16(want)


# ------------------------------------------------------------------ lanes that diverge
@pytest.fixture(scope="module")
def loud_quiet():
    """Frames of blocksize 4096 from three streams of one format: loud (Rice parameter 13+,
    codewords near 16 bits), near-silent (parameter 0..2) and C2's own (parameter ~8)."""
    loud = _stream(nframes=48, level=0.9, noise=0.5, seed=71)
    quiet = _stream(nframes=48, level=0.0001, noise=0.00001, seed=72)
    mid = _stream(nframes=48, seed=73)
    for (s, data, offs, _), lo, hi in ((loud, 13, 15), (quiet, 0, 2), (mid, 3, 9)):  # 15: the partition escaped
        ks = [_first_rice_param(data, o) for o in offs]
        assert lo <= min(ks) and max(ks) <= hi, ks
    return loud, quiet, mid


def _interleaved(gpu, a, b, n):
    """Frames of the two streams alternately, n in all, in one buffer (b's frames appended behind
    a's stream; each frame placed in the output by its own out_sample)."""
    torch, libflac, dec = gpu
    (sa, da, oa, ea), (sb, db, ob, eb) = a, b
    data = da + db[ob[0]:]
    shift = len(da) - ob[0]
    offs, ends, pcm = [], [], []
    for i in range(n):
        s, o, e, sh = (sa, oa, ea, 0) if i % 2 == 0 else (sb, ob, eb, shift)
        offs.append(o[i // 2] + sh)
        ends.append(e[i // 2] + sh)
        pcm.append(s.pcm[(i // 2) * 4096:(i // 2 + 1) * 4096])
    pcm = np.concatenate(pcm)
    sp = _sp(libflac, data, total=len(pcm))
    starts = [4096 * i for i in range(n)]
    info, out = _decode(gpu, data, offs, sp, starts, len(pcm))
    _check_records(data, offs, ends, info, walk=range(0, n, 7))
    assert out.tobytes() == _pcm16(pcm)
    info_b, out_b = _decode(gpu, data, offs, sp, starts, len(pcm), ablate=BLK_REFILL)
    _same_records(info, info_b)
    assert out_b.tobytes() == out.tobytes()
    info_w, _ = _decode(gpu, data, offs, sp, starts, len(pcm), parse_wave=1)
    _same_records(info, info_w)


def test_loud_and_quiet_lanes_plain_walk(gpu, loud_quiet):
    """A first Rice parameter above 9 in the wave: the plain instance of the walk."""
    loud, quiet, _ = loud_quiet
    _interleaved(gpu, loud, quiet, 96)


def test_mid_and_quiet_lanes_bulk_walk(gpu, loud_quiet):
    """Every first parameter at most 9: the bulk instance, its lanes consuming ~1.3 and ~10
    bits a codeword."""
    _, quiet, mid = loud_quiet
    _interleaved(gpu, mid, quiet, 96)


# ------------------------------------------------------------------ cursor jumps, uneven lengths
@pytest.mark.parametrize("kw", [dict(escape_permille=300, seed=81), dict(escape_permille=150, rice2=1, partition_order=2, seed=82),
                                dict(impulse_permille=3, seed=83)], ids=["escape", "rice2-escape", "impulse"])
def test_escaped_partitions_and_long_prefixes(gpu, kw):
    s, data, offs, ends = _stream(nframes=70, **kw)
    _whole(gpu, s, data, offs, ends, walk=range(0, 70, 9))


def test_c4_uneven_lengths_one_launch(gpu):
    """128 frames of blocksizes 192..16384, CONSTANT / VERBATIM / FIXED / LPC in either channel
    (a VERBATIM channel 0 before an LPC channel 1 among them)."""
    s, data, offs, ends = _stream("C4", nframes=128)
    info = _whole(gpu, s, data, offs, ends, walk=range(0, 128, 5))
    assert int(info["blocksize"].min()) <= 256 and int(info["blocksize"].max()) == 16384


@pytest.mark.parametrize("name", ["rice2_escape", "verbatim_12bit_3ch"])
def test_fixture_streams(gpu, name):
    """The escape / VERBATIM fixtures through the lane walk: the golden PCM, and k_parse_wave's
    records."""
    import hashlib
    torch, libflac, dec = gpu
    g = GOLD[name]
    data = open(os.path.join(GOLD_DIR, g["file"]), "rb").read()
    sp = _sp(libflac, data)
    dev = torch.device("cuda:0")
    res = []
    for wave in (0, 1):
        d_bytes = torch.zeros((len(data) + 15) // 16 * 16, dtype=torch.uint8, device=dev)
        d_bytes[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
        offs = torch.tensor(g["frame_offsets"], dtype=torch.int64, device=dev)
        d_out = torch.zeros(sp.total_samples * sp.channels * 4, dtype=torch.uint8, device=dev)
        d_info = torch.zeros(len(g["frame_offsets"]) * libflac.FRAME_INFO_BYTES, dtype=torch.uint8, device=dev)
        dec.L.bnflac_debug_set_parse_wave(wave)
        try:
            dec.decode_frames(d_bytes, len(data), offs, len(g["frame_offsets"]), sp, libflac.OUT_INTERLEAVED32, d_out, d_info)
            torch.cuda.synchronize()
        finally:
            dec.L.bnflac_debug_set_parse_wave(0)
        res.append((libflac.info_array(d_info.cpu().numpy()), d_out.cpu().numpy()))
    info, out = res[0]
    assert (info["status"] == 0).all() and (info["crc_ok"] == 1).all()
    pcm = np.ascontiguousarray(out.view("<i4").reshape(-1, sp.channels), dtype="<i4")
    assert hashlib.sha256(pcm.tobytes()).hexdigest() == g["pcm_sha256"]
    _same_records(info, res[1][0])
    assert res[1][1].tobytes() == out.tobytes()


def test_truncated_last_frame(gpu):
    """nbytes inside the last frame's channel 0: TRUNC for it, as before; the others decode."""
    torch, libflac, dec = gpu
    s, data, offs, ends = _stream(nframes=5, blocksize=1152, seed=91)
    sp = _sp(libflac, data)
    starts = [1152 * i for i in range(5)]
    for cut in (offs[4] + 200, offs[4] + 64 * ((ends[4] - offs[4]) // 192), offs[4] + 701):
        res = [_decode(gpu, data, offs, sp, starts, s.nsamples, nbytes=cut, ablate=a, parse_wave=w)
               for a, w in ((0, 0), (BLK_REFILL, 0), (0, 1))]
        info, out = res[0]
        assert info["status"].tolist() == [0, 0, 0, 0, ST_TRUNC] and info["crc_ok"][:4].tolist() == [1, 1, 1, 1]
        assert out[:4 * 1152 * 4].tobytes() == _pcm16(s.pcm[:4 * 1152])
        assert not out[4 * 1152 * 4:].any()
        for info_x, out_x in res[1:]:
            _same_records(info, info_x)
            assert out_x.tobytes() == out.tobytes()
