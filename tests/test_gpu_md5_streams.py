"""bnflac_md5_streams: the STREAMINFO md5sum of every stream of a decoded batch, on the device.

Everything is exact.  The reference is hashlib.md5 over bytes numpy builds (independent of the
library) and, end to end, each stream's own STREAMINFO sum.
"""
import hashlib

import numpy as np
import pytest

from tests.conftest import gpu_available
from tests.test_gpu_index_streams import _first_frame_offset, _pack, _stream_params, _upload

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EMPTY = bytes.fromhex("d41d8cd98f00b204e9800998ecf8427e")
ZERO = bytes(16)


@pytest.fixture(scope="module")
def gpu():
    if not gpu_available():
        pytest.skip("no GPU")
    import torch
    from birdnest.audio_amd import libflac
    return torch, libflac, libflac.BatchDecoder(0)


def _params(libflac, channels, bps):
    return libflac.StreamParams(1, 4096, 4096, 44100, channels, bps, 0)


def _bounds(lengths, start=0):
    return np.concatenate([[start], start + np.cumsum(lengths)]).astype(np.int64)


def _run(gpu, d_pcm, fmt, sp, bounds, expected=None, pcm_bytes=None):
    """One md5_streams call -> ([sum bytes], verdicts, status) on the host"""
    torch, libflac, dec = gpu
    n = len(bounds) - 1
    d_b = torch.from_numpy(np.asarray(bounds, dtype=np.int64)).to(DEV)
    d_e = None
    if expected is not None:
        d_e = torch.from_numpy(np.frombuffer(b"".join(expected), dtype=np.uint8).copy()).to(DEV)
    d_md5, d_v, d_st = dec.md5_streams(d_pcm, fmt, sp, d_b, n, d_expected=d_e, pcm_bytes=pcm_bytes)
    torch.cuda.synchronize()
    md5 = d_md5.cpu().numpy()
    return [md5[i].tobytes() for i in range(n)], d_v.cpu().numpy().tolist(), d_st.cpu().numpy().tolist()


def _message(pcm: np.ndarray, bps: int) -> bytes:
    """libFLAC's MD5 message of int32 PCM: the low (bps + 7) / 8 bytes of each sample, interleaved"""
    nb = (bps + 7) // 8
    return np.ascontiguousarray(pcm, dtype="<i4").reshape(-1).view(np.uint8).reshape(-1, 4)[:, :nb].tobytes()


def _md5(b: bytes) -> bytes:
    return hashlib.md5(b).digest()


# ------------------------------------------------------------------ 1. padding classes (int32 source, B = 1)
def test_padding_classes_b1(gpu):
    torch, libflac, dec = gpu
    lengths = [0, 1, 55, 56, 57, 63, 64, 65, 119, 120, 127, 128, 129, 191, 192, 193]
    rng = np.random.default_rng(1)
    pcm = rng.integers(-(1 << 31), 1 << 31, size=sum(lengths), dtype=np.int64).astype(np.int32)
    assert (pcm < 0).any()
    b = _bounds(lengths)
    sums, verdicts, status = _run(gpu, torch.from_numpy(pcm).to(DEV), libflac.OUT_INTERLEAVED32, _params(libflac, 1, 8), b)
    for s, n in enumerate(lengths):
        assert sums[s] == _md5(_message(pcm[b[s]:b[s + 1]], 8)), n
    assert verdicts == [2] * 16
    assert status == [0, 0, 0, 16]


# ------------------------------------------------------------------ 2. every B (int32 source)
@pytest.mark.parametrize("channels,bps", [(1, 4), (1, 8), (3, 12), (2, 16), (6, 20), (2, 24), (3, 32)])
def test_every_bytes_per_sample(gpu, channels, bps):
    torch, libflac, dec = gpu
    lengths = [0, 1, 21, 64, 311]
    rng = np.random.default_rng(100 * channels + bps)
    pcm = rng.integers(-(1 << 31), 1 << 31, size=(sum(lengths), channels), dtype=np.int64).astype(np.int32)
    b = _bounds(lengths)
    sums, verdicts, status = _run(gpu, torch.from_numpy(pcm).to(DEV), libflac.OUT_INTERLEAVED32,
                                  _params(libflac, channels, bps), b)
    for s in range(len(lengths)):
        assert sums[s] == _md5(_message(pcm[b[s]:b[s + 1]], bps)), lengths[s]
    assert sums[4] == libflac.md5_interleaved32(pcm[b[4]:b[5]], channels, bps)
    assert status == [0, 0, 0, 5]


# ------------------------------------------------------------------ 3. packed source, every start alignment
@pytest.mark.parametrize("fmt_name,channels,bps,stride", [("FILEREADER", 1, 24, 3), ("FILEREADER", 2, 24, 6),
                                                          ("FLACDECODER", 1, 16, 2), ("FLACDECODER", 2, 16, 4)])
def test_packed_source_alignments(gpu, fmt_name, channels, bps, stride):
    torch, libflac, dec = gpu
    fmt = getattr(libflac, "OUT_" + fmt_name)
    sp = _params(libflac, channels, bps)
    assert libflac.out_stride(fmt, sp) == stride and libflac.md5_layout(fmt, sp) == bps // 8
    lengths = [1, 1, 1, 1, 22, 43, 0, 85]
    b = _bounds(lengths, start=1 if stride in (2, 6) else 0)  # an odd frame total where that unaligns the end
    pcm_bytes = int(b[-1]) * stride  # the last stream ends exactly at pcm_bytes
    assert stride == 4 or pcm_bytes % 4 != 0
    if stride == 3:
        assert [int(x) * stride & 3 for x in b[:5]] == [0, 3, 2, 1, 0]
    rng = np.random.default_rng(stride)
    raw = rng.integers(0, 256, size=pcm_bytes, dtype=np.uint8)
    want = [_md5(raw[int(b[s]) * stride:int(b[s + 1]) * stride].tobytes()) for s in range(len(lengths))]
    d_pcm = torch.empty((pcm_bytes + 15) // 16 * 16 + 64, dtype=torch.uint8, device=DEV)
    for poison in (0x5A, 0xC3):  # the bytes past pcm_bytes must not matter
        d_pcm.fill_(poison)
        d_pcm[:pcm_bytes] = torch.from_numpy(raw).to(DEV)
        sums, verdicts, status = _run(gpu, d_pcm, fmt, sp, b, pcm_bytes=pcm_bytes)
        assert sums == want, hex(poison)
        assert verdicts == [2] * 8 and status == [0, 0, 0, 8]


# ------------------------------------------------------------------ 4. more than one wave, divergent lengths
def test_many_streams_divergent_lengths(gpu):
    torch, libflac, dec = gpu
    rng = np.random.default_rng(4)
    lengths = rng.choice([0, 13, 14, 16, 1000], size=130).tolist()
    lengths[37] = 30000  # one long lane beside finished ones
    b = _bounds(lengths)
    raw = rng.integers(0, 256, size=int(b[-1]) * 4, dtype=np.uint8)
    sums, verdicts, status = _run(gpu, torch.from_numpy(raw).to(DEV), libflac.OUT_FLACDECODER, _params(libflac, 2, 16), b)
    for s in range(130):
        assert sums[s] == _md5(raw[int(b[s]) * 4:int(b[s + 1]) * 4].tobytes()), (s, lengths[s])
    assert status == [0, 0, 0, 130]


# ------------------------------------------------------------------ 5. addresses above 2^32
def test_addresses_above_4gib(gpu):
    torch, libflac, dec = gpu
    size = (4 << 30) + (1 << 20)
    try:
        d_pcm = torch.empty(size, dtype=torch.uint8, device=DEV)
    except Exception as e:  # out of memory on a shared card
        pytest.skip(f"cannot allocate 4 GiB + 1 MiB: {e}")
    rng = np.random.default_rng(5)
    lo = rng.integers(0, 256, size=4 * 777, dtype=np.uint8)
    hi = rng.integers(0, 256, size=4 * 1501, dtype=np.uint8)
    hi_frame = (4 << 30) // 4 + 33  # sample frames of 4 bytes: 132 bytes above 4 GiB
    d_pcm[: lo.size] = torch.from_numpy(lo).to(DEV)
    d_pcm[hi_frame * 4: hi_frame * 4 + hi.size] = torch.from_numpy(hi).to(DEV)
    # the high range first: the pair between the two ranges then descends (verdict 3, nothing
    # read) instead of spanning the 4 GiB of unwritten memory between them
    bounds = [hi_frame, hi_frame + 1501, 0, 777]
    sums, verdicts, status = _run(gpu, d_pcm, libflac.OUT_FLACDECODER, _params(libflac, 2, 16), bounds)
    assert sums[0] == _md5(hi.tobytes())
    assert sums[2] == _md5(lo.tobytes())
    assert verdicts == [2, 3, 2] and status == [1, 0, 0, 2]


# ------------------------------------------------------------------ 6. verdicts and errors
def test_verdicts(gpu):
    torch, libflac, dec = gpu
    rng = np.random.default_rng(6)
    raw = rng.integers(0, 256, size=4 * 400, dtype=np.uint8)
    pcm_bytes = raw.size
    d_pcm = torch.from_numpy(raw).to(DEV)
    sp = _params(libflac, 2, 16)
    #          true   bit in byte 0   bit in byte 15   all zero   empty      past pcm_bytes
    bounds = [0, 100, 200, 300, 400, 400, 401]
    true = [_md5(raw[4 * bounds[s]:4 * bounds[s + 1]].tobytes()) for s in range(5)]
    assert true[4] == EMPTY
    flip0 = bytes([true[1][0] ^ 0x01]) + true[1][1:]
    flip15 = true[2][:15] + bytes([true[2][15] ^ 0x80])
    expected = [true[0], flip0, flip15, ZERO, EMPTY, true[0]]
    sums, verdicts, status = _run(gpu, d_pcm, libflac.OUT_FLACDECODER, sp, bounds, expected, pcm_bytes=pcm_bytes)
    assert sums[:5] == true and sums[5] == ZERO
    assert verdicts == [0, 1, 1, 2, 0, 3]
    assert status == [1, 2, 2, 1]
    # a descending pair
    sums, verdicts, status = _run(gpu, d_pcm, libflac.OUT_FLACDECODER, sp, [0, 100, 50, 60], [true[0], ZERO, ZERO],
                                  pcm_bytes=pcm_bytes)
    assert verdicts == [0, 3, 2] and sums[0] == true[0] and sums[1] == ZERO
    assert status == [1, 1, 0, 1]
    # layouts that do not hold the message
    d_b = torch.tensor([0, 10], dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="layout does not carry the MD5 bytes"):
        dec.md5_streams(d_pcm, libflac.OUT_PLANAR32, sp, d_b, 1)
    with pytest.raises(RuntimeError, match="layout does not carry the MD5 bytes"):
        dec.md5_streams(d_pcm, libflac.OUT_FILEREADER, _params(libflac, 2, 20), d_b, 1)
    # no streams: a zero status
    d_md5, d_v, d_st = dec.md5_streams(d_pcm, libflac.OUT_FLACDECODER, sp, d_b, 0)
    torch.cuda.synchronize()
    assert d_st.cpu().tolist() == [0, 0, 0, 0] and d_md5.numel() == 0


# ------------------------------------------------------------------ 7. end to end
def _batch_inputs(gpu, datas):
    torch, libflac, dec = gpu
    buf, ranges = _pack(datas, (0, 5, 16, 33)[: len(datas) - 1])
    table = [(b, e, b + (_first_frame_offset(d) if d else 0), _stream_params(libflac, d).total_samples if d else 0)
             for (b, e), d in zip(ranges, datas)]
    sp = _stream_params(libflac, datas[0], 0)
    d_exp = torch.from_numpy(np.frombuffer(b"".join(libflac.streaminfo_md5(d) if d else EMPTY for d in datas),
                                           dtype=np.uint8).copy()).to(DEV)
    return buf, table, sp, d_exp


def _flow(gpu, datas, nframes, fmt):
    """index_streams -> decode_parsed over all nframes records -> md5_streams against the
    STREAMINFO sums, with no host synchronisation in between
    -> (sums, verdicts, status, records, frames per stream, sample bounds)"""
    torch, libflac, dec = gpu
    buf, table, sp, d_exp = _batch_inputs(gpu, datas)
    total = sum(t[3] for t in table)
    stride = libflac.out_stride(fmt, sp)
    d_bytes = _upload(torch, buf)
    d_out = torch.full(((total * stride + 15) // 16 * 16 + 64,), 0xAB, dtype=torch.uint8, device=DEV)
    d_offs, d_os, d_info, d_sf, d_ss, d_st = dec.index_streams(d_bytes, len(buf), table, sp, len(buf) // 16 + 16)
    dec.decode_parsed(d_bytes, len(buf), nframes, sp, fmt, d_out, d_info)
    d_md5, d_v, d_status = dec.md5_streams(d_out, fmt, sp, d_ss, len(datas), d_expected=d_exp, pcm_bytes=total * stride)
    torch.cuda.synchronize()
    assert d_st.cpu().tolist()[0] == 0 and int(d_sf[-1]) == nframes
    md5 = d_md5.cpu().numpy()
    rec = libflac.info_array(d_info[: nframes * libflac.FRAME_INFO_BYTES].cpu().numpy())
    return ([md5[i].tobytes() for i in range(len(datas))], d_v.cpu().tolist(), d_status.cpu().tolist(), rec,
            np.diff(d_sf.cpu().numpy()).tolist(), d_ss.cpu().numpy())


_C2 = {}
_C2_SHAPE = [(12, 1001), (1, 14), (7, 0), (0, 0), (3, 13)]  # (frames, last blocksize; 0: a full block)


def _c2_batch():
    """Five C2 streams of 12, 1, 7, 0 and 3 frames; last blocks of 1001, 14 (56 message bytes:
    the length spills into a second padding block) and 13 (52: it does not) samples"""
    if not _C2:
        from birdnest.audio_amd import synth
        syn = [synth.encode(synth.config("C2", nframes=nf, last_blocksize=lb, seed=11 + 7 * i)) if nf else None
               for i, (nf, lb) in enumerate(_C2_SHAPE)]
        datas = [s.data.tobytes() if s else b"" for s in syn]
        assert len(syn[1].pcm) * 4 == 56 and len(syn[4].pcm) * 4 == 2 * 4096 * 4 + 52
        _C2.update(syn=syn, datas=datas)
    return _C2


@pytest.mark.parametrize("fmt_name", ["FLACDECODER", "INTERLEAVED32"])
def test_end_to_end_16bit(gpu, fmt_name):
    torch, libflac, dec = gpu
    m = _c2_batch()
    sums, verdicts, status, rec, sf, ss = _flow(gpu, m["datas"], 23, getattr(libflac, "OUT_" + fmt_name))
    assert sf == [12, 1, 7, 0, 3]
    assert (rec["status"] == 0).all() and (rec["crc_ok"] == 1).all()
    assert verdicts == [0] * 5
    assert status == [0, 5, 0, 0]
    for s, (syn, d) in enumerate(zip(m["syn"], m["datas"])):
        if syn is None:
            assert sums[s] == EMPTY
            continue
        assert sums[s] == libflac.streaminfo_md5(d), s
        assert sums[s] == _md5(_message(syn.pcm, 16)), s


@pytest.mark.parametrize("fmt_name", ["FILEREADER", "INTERLEAVED32"])
def test_end_to_end_24bit(gpu, fmt_name):
    from birdnest.audio_amd import synth
    torch, libflac, dec = gpu
    syn = [synth.encode(synth.config("C3", nframes=2, blocksize=1152, last_blocksize=577, seed=40 + i)) for i in range(3)]
    datas = [s.data.tobytes() for s in syn]
    assert (len(syn[0].pcm) * 6) & 3 == 2  # the second stream's packed start
    sums, verdicts, status, rec, sf, ss = _flow(gpu, datas, 6, getattr(libflac, "OUT_" + fmt_name))
    assert sf == [2, 2, 2]
    assert (rec["status"] == 0).all() and (rec["crc_ok"] == 1).all()
    assert verdicts == [0] * 3 and status == [0, 3, 0, 0]
    for s, (y, d) in enumerate(zip(syn, datas)):
        assert sums[s] == libflac.streaminfo_md5(d), s
        assert sums[s] == _md5(_message(y.pcm, 24)), s


def _damaged_c2():
    """The C2 batch with one byte flipped inside frame 3's residual of the 7-frame stream"""
    m = _c2_batch()
    datas = list(m["datas"])
    o = [int(x) for x in m["syn"][2].frame_offsets]
    d = bytearray(datas[2])
    d[o[4] - 10] ^= 0x10  # the end of frame 3's last subframe: its header and walk stay valid
    datas[2] = bytes(d)
    return m, datas


def test_end_to_end_damage(gpu):
    """Every frame of the batch decoded from the generator's frame offsets (parse_frames ->
    decode_parsed -> md5_streams): the damaged frame fails its CRC-16, is written as zeros, and
    the stream's sum is that of its PCM with the frame zeroed."""
    torch, libflac, dec = gpu
    m, datas = _damaged_c2()
    buf, table, sp, d_exp = _batch_inputs(gpu, datas)
    offs, out_sample, bounds = [], [], [0]
    for (nf, lb), syn, t in zip(_C2_SHAPE, m["syn"], table):
        for k in range(nf):
            offs.append(t[0] + int(syn.frame_offsets[k]))
            out_sample.append(bounds[-1] + 4096 * k)
        bounds.append(bounds[-1] + (len(syn.pcm) if syn else 0))
    nf, total = len(offs), bounds[-1]
    d_bytes = _upload(torch, buf)
    d_offs = torch.tensor(offs, dtype=torch.int64, device=DEV)
    d_os = torch.tensor(out_sample, dtype=torch.int64, device=DEV)
    d_ss = torch.tensor(bounds, dtype=torch.int64, device=DEV)
    d_info = torch.zeros(nf * libflac.FRAME_INFO_BYTES, dtype=torch.uint8, device=DEV)
    d_out = torch.full((total * 4 + 64,), 0xAB, dtype=torch.uint8, device=DEV)
    dec.parse_frames(d_bytes, len(buf), d_offs, nf, sp, d_info, d_out_sample=d_os)
    dec.decode_parsed(d_bytes, len(buf), nf, sp, libflac.OUT_FLACDECODER, d_out, d_info)
    d_md5, d_v, d_status = dec.md5_streams(d_out, libflac.OUT_FLACDECODER, sp, d_ss, 5, d_expected=d_exp, pcm_bytes=total * 4)
    torch.cuda.synchronize()
    rec = libflac.info_array(d_info.cpu().numpy())
    bad = 12 + 1 + 3  # the record of the 7-frame stream's frame 3
    assert (rec["status"] == 0).all()
    assert rec["crc_ok"][bad] == 0 and rec["crc_ok"].sum() == nf - 1
    assert d_v.cpu().tolist() == [0, 0, 1, 0, 0]
    assert d_status.cpu().tolist() == [0, 4, 1, 0]
    sums = [x.tobytes() for x in d_md5.cpu().numpy()]
    pcm = m["syn"][2].pcm.copy()
    pcm[3 * 4096:4 * 4096] = 0  # libFLAC writes a CRC-failed frame as zeros
    assert sums[2] == _md5(_message(pcm, 16))
    assert sums[2] != libflac.streaminfo_md5(datas[2])
    for s in (0, 1, 4):
        assert sums[s] == libflac.streaminfo_md5(datas[s])
    assert sums[3] == EMPTY


def test_end_to_end_damage_indexed(gpu):
    """The same damage through index_streams: the chain of the damaged stream ends with the
    damaged frame (no frame start follows at which its CRC-16 is zero), so the stream is its
    first four frames, the fourth zeroed; the sum differs from STREAMINFO's all the same."""
    torch, libflac, dec = gpu
    m, datas = _damaged_c2()
    sums, verdicts, status, rec, sf, ss = _flow(gpu, datas, 20, libflac.OUT_FLACDECODER)
    assert sf == [12, 1, 4, 0, 3]
    assert rec["crc_ok"][12 + 1 + 3] == 0 and rec["crc_ok"].sum() == 19
    assert verdicts == [0, 0, 1, 0, 0]
    assert status == [0, 4, 1, 0]
    pcm = m["syn"][2].pcm[: 4 * 4096].copy()
    pcm[3 * 4096:] = 0
    assert sums[2] == _md5(_message(pcm, 16))
    for s in (0, 1, 4):
        assert sums[s] == libflac.streaminfo_md5(datas[s])
