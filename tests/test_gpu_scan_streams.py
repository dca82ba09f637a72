"""bnflac_scan_streams: the metadata of many streams of one buffer, read on the device.

Every comparison is exact.  The references are independent of the kernel: the Python
restatement of the rule and the variants of tests/test_scan_streams_host.py, the host twin
bnflac_scan_stream_host, the libFLAC stream API of the library, and for the chain the generator's
frame offsets and PCM.
"""
import ctypes
import hashlib

import numpy as np
import pytest

from tests.conftest import gpu_available
from tests.test_scan_streams_host import (APP, BAD_RANGE, DIFFERENT, F_DIFFERS, FAILED, KEPT, META_FIELDS, OK, SEEK, TAGGED,
                                          VARIANTS, all_cases, blk, golden_files, id3_tag, meta_tuple, ref_scan)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POISON = 0x5A
POISON64 = int.from_bytes(bytes([POISON]) * 8, "little")
FILL = bytes([0xFF, 0xF8, 0x66, 0x4C, 0x61, 0x43, 0x80, 0x00]) * 8  # gap filler: sync pairs, a marker, a block header


@pytest.fixture(scope="module")
def gpu():
    if not gpu_available():
        pytest.skip("no GPU")
    import torch
    from birdnest.audio_amd import libflac
    return torch, libflac, libflac.BatchDecoder(0)


def _pack(datas, gaps, lead=0):
    """datas: [bytes]; gaps cycled: gaps[i % len] filler bytes after stream i -> (buffer, [(begin, end)])"""
    buf, ranges = bytearray(FILL[:lead]), []
    for i, d in enumerate(datas):
        ranges.append((len(buf), len(buf) + len(d)))
        buf += d
        buf += FILL[: gaps[i % len(gaps)]]
    return bytes(buf), ranges


def _upload(torch, data: bytes, tail=POISON):
    """The buffer on the device, its allocation round_up(n, 16) + 16 bytes, poisoned past n"""
    n = len(data)
    d = torch.full(((n + 15) // 16 * 16 + 16,), tail, dtype=torch.uint8, device=DEV)
    if n:
        d[:n] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(DEV)
    return d


class Scan:
    """One scan_streams call, synchronised and copied to the host"""

    def __init__(self, gpu, buf: bytes, ranges, expect=None, d_bytes=None):
        torch, libflac, dec = gpu
        self.d_bytes = _upload(torch, buf) if d_bytes is None else d_bytes
        self.d_tab, d_meta, self.d_md5, d_st = dec.scan_streams(self.d_bytes, len(buf), ranges, expect=expect)
        torch.cuda.synchronize()
        n = len(ranges)
        self.table = self.d_tab.cpu().numpy().reshape(n, 4)
        self.meta = libflac.meta_array(d_meta.cpu().numpy())
        md5 = self.d_md5.cpu().numpy()
        self.md5 = [md5[i].tobytes() for i in range(n)]
        self.status = d_st.cpu().numpy().tolist()


def _expect_tuple(sp):
    return (sp.min_blocksize, sp.max_blocksize, sp.sample_rate, sp.channels, sp.bps)


def _assert_equals_ref(sc: Scan, buf: bytes, ranges, expect=None, bad=()):
    """Every output of the scan against ref_scan over each stream's own bytes, and the status"""
    counts = [0, 0, 0]
    for s, (b, e) in enumerate(ranges):
        kind, rec, desc, md5 = ref_scan(buf[b:e] if s not in bad else b"", b, e, bad_range=s in bad,
                                        expect=_expect_tuple(expect) if expect is not None else None)
        counts[kind] += 1
        assert meta_tuple(sc.meta[s]) == rec, s
        assert tuple(int(x) for x in sc.table[s]) == (b, e) + desc, s
        assert sc.md5[s] == md5, s
    bits = (1 if counts[FAILED] else 0) | (2 if counts[DIFFERENT] else 0) | (4 if bad else 0)
    assert sc.status == [bits, counts[KEPT], counts[FAILED], counts[DIFFERENT]]
    return counts


# ------------------------------------------------------------------ 1. parity with the host twin
_PARITY = {}


def _parity(gpu):
    """Every fixture and variant in one buffer (scanned once, shared with the stream API test)"""
    if not _PARITY:
        cases = all_cases()
        names = list(cases)
        buf, ranges = _pack([cases[k] for k in names], (0, 5, 16, 33), lead=1)
        assert sum(b & 1 for b, _ in ranges) > 4 and len({b % 16 for b, _ in ranges}) > 8
        _PARITY.update(names=names, cases=cases, buf=buf, ranges=ranges, scan=Scan(gpu, buf, ranges))
    return _PARITY


def test_parity_with_the_host_twin(gpu):
    torch, libflac, dec = gpu
    m = _parity(gpu)
    sc = m["scan"]
    kept = failed = 0
    for s, (name, (b, e)) in enumerate(zip(m["names"], m["ranges"])):
        meta, md5 = libflac.scan_stream_host(m["cases"][name])
        want = list(meta_tuple(meta))
        want[-1] += b  # first_offset is absolute
        assert meta_tuple(sc.meta[s]) == tuple(want), name
        assert sc.md5[s] == md5, name
        ok = meta.status == OK
        assert tuple(int(x) for x in sc.table[s]) == (b, e, want[-1], meta.sp.total_samples if ok else 0), name
        kept += ok
        failed += not ok
    assert failed >= 9 and sc.status == [1, kept, failed, 0]
    _assert_equals_ref(sc, m["buf"], m["ranges"])


# ------------------------------------------------------------------ 2. cuts with hostile neighbours
def test_cuts_with_hostile_neighbours(gpu):
    """Every cut of the tagged variant as a stream of its own, the bytes that would complete it
    right behind its end"""
    first = ref_scan(TAGGED)[2][0]
    buf, ranges = bytearray(b"\xff"), []
    for k in range(first + 2):
        ranges.append((len(buf), len(buf) + k))
        buf += TAGGED[: first + 40]  # the cut, then the rest of the header and the first frame's start
    assert len(ranges) > 64
    buf = bytes(buf)
    counts = _assert_equals_ref(Scan(gpu, buf, ranges), buf, ranges)
    assert counts == [2, first, 0]  # OK: the cut at first_offset and the one a byte later


# ------------------------------------------------------------------ 3. every alignment of begin
def test_every_alignment(gpu):
    datas = [VARIANTS["tagged_four_blocks"], VARIANTS["streaminfo_37"]] * 8
    buf, ranges = bytearray(), []
    for a, d in enumerate(datas):
        buf += FILL[: (a - len(buf)) % 16]
        ranges.append((len(buf), len(buf) + len(d)))
        buf += d
    assert [b % 16 for b, _ in ranges] == list(range(16))
    buf = bytes(buf)  # the last stream ends exactly at nbytes
    assert _assert_equals_ref(Scan(gpu, buf, ranges), buf, ranges) == [16, 0, 0]


# ------------------------------------------------------------------ 4. wave edges, poisoned tails
def _raw(gpu, d_bytes, nbytes, table, n, expect=None, tail=3):
    """The C call itself on outputs of n + tail poisoned entries -> host copies"""
    torch, libflac, dec = gpu
    tab = np.full((n + tail, 4), POISON64, dtype=np.uint64)
    tab[:n, :2] = np.asarray(table, dtype=np.uint64).reshape(n, 2)
    d_tab = torch.from_numpy(tab.view(np.int64).reshape(-1).copy()).to(DEV)
    d_meta = torch.full(((n + tail) * 64,), POISON, dtype=torch.uint8, device=DEV)
    d_md5 = torch.full(((n + tail) * 16,), POISON, dtype=torch.uint8, device=DEV)
    d_st = torch.full((4 + tail,), POISON, dtype=torch.int32, device=DEV)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = dec.L.bnflac_scan_streams(dec.ctx, vp(d_bytes), nbytes, vp(d_tab), n, ctypes.byref(expect) if expect else None,
                                   vp(d_meta), vp(d_md5), vp(d_st), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return (rc, d_tab.cpu().numpy().view(np.uint64).reshape(n + tail, 4), d_meta.cpu().numpy(), d_md5.cpu().numpy(),
            d_st.cpu().numpy())


def test_wave_edges(gpu):
    torch, libflac, dec = gpu
    pool = [VARIANTS["ends_at_end"], golden_files()["rfc9639_ex1.flac"], VARIANTS["junk_2"][:60], VARIANTS["id3_1"][:90],
            VARIANTS["never_last"]]
    datas = [pool[(i * 7) % len(pool)] for i in range(130)]
    buf, ranges = _pack(datas, (1, 0, 3), lead=3)
    d_bytes = _upload(torch, buf)
    for n in (0, 1, 63, 64, 65, 130):
        rc, tab, meta, md5, st = _raw(gpu, d_bytes, len(buf), ranges[:n], n)
        assert rc == 0
        counts = [0, 0, 0]
        rec = libflac.meta_array(meta[: n * 64])
        for s, (b, e) in enumerate(ranges[:n]):
            kind, want, desc, want_md5 = ref_scan(buf[b:e], b, e)
            counts[kind] += 1
            assert meta_tuple(rec[s]) == want, (n, s)
            assert tuple(int(x) for x in tab[s]) == (b, e) + desc, (n, s)
            assert md5[16 * s:16 * s + 16].tobytes() == want_md5, (n, s)
        assert st[:4].tolist() == [1 if counts[FAILED] else 0, counts[KEPT], counts[FAILED], 0], n
        assert (tab[n:] == POISON64).all() and (meta[n * 64:] == POISON).all() and (md5[n * 16:] == POISON).all(), n
        assert (st[4:] == POISON).all(), n
        if n == 130:
            assert counts[KEPT] > 64 and counts[FAILED] > 32


# ------------------------------------------------------------------ 5. a bad table
def test_bad_table(gpu):
    torch, libflac, dec = gpu
    datas = [VARIANTS["plain"], VARIANTS["id3_1"], VARIANTS["extra_blocks"], VARIANTS["streaminfo_37"], VARIANTS["plain"],
             VARIANTS["ends_at_end"]]
    buf, ranges = _pack(datas, (4, 0, 9))
    buf = buf[: ranges[-1][1]]  # the last stream ends at nbytes
    good = Scan(gpu, buf, ranges)
    assert _assert_equals_ref(good, buf, ranges) == [6, 0, 0]
    bad = list(ranges)
    bad[1] = (ranges[1][1], ranges[1][0])          # reversed
    bad[3] = (ranges[2][1] - 1, ranges[3][1])      # begins inside the previous stream
    bad[5] = (ranges[5][0], len(buf) + 1)          # past nbytes
    sc = Scan(gpu, buf, bad, d_bytes=good.d_bytes)
    assert _assert_equals_ref(sc, buf, bad, bad=(1, 3, 5)) == [3, 3, 0]
    assert sc.status[0] == 5 and [int(x) for x in sc.meta["status"]] == [OK, BAD_RANGE, OK, BAD_RANGE, OK, BAD_RANGE]
    for s in (0, 2, 4):  # the neighbours: as in the good table
        assert sc.meta[s] == good.meta[s] and (sc.table[s] == good.table[s]).all() and sc.md5[s] == good.md5[s]


# ------------------------------------------------------------------ 6. expected parameters
def test_expected_params(gpu):
    torch, libflac, dec = gpu
    g = golden_files()
    names = ["plain", "extra_blocks", "mono_8bit_fixed.flac", "id3_128", "c3_lpc12_ms_wasted.flac", "streaminfo_37"]
    datas = [VARIANTS.get(k, g.get(k)) for k in names]
    c2 = dict(zip(META_FIELDS, ref_scan(VARIANTS["plain"])[1]))
    expect = libflac.StreamParams(1, c2["min_blocksize"], c2["max_blocksize"], c2["sample_rate"], c2["channels"], c2["bps"], 0)
    own = [dict(zip(META_FIELDS, ref_scan(d)[1])) for d in datas]
    assert (own[2]["channels"], own[2]["bps"]) == (1, 8) and own[4]["bps"] == 24
    buf, ranges = _pack(datas, (5, 0, 16, 33), lead=7)
    sc = Scan(gpu, buf, ranges, expect=expect)
    assert _assert_equals_ref(sc, buf, ranges, expect=expect) == [4, 0, 2]
    n = len(datas)
    assert sc.status == [2, n - 2, 0, 2]
    for s in (2, 4):  # emptied, their own values in the record
        b, e = ranges[s]
        assert tuple(int(x) for x in sc.table[s]) == (b, e, e, 0) and sc.md5[s] == bytes(16)
        assert int(sc.meta["flags"][s]) & F_DIFFERS and int(sc.meta["status"][s]) == OK
        for k in ("min_blocksize", "max_blocksize", "sample_rate", "channels", "bps", "total_samples", "min_framesize",
                  "max_framesize"):
            assert int(sc.meta[k][s]) == own[s][k], (s, k)
        assert int(sc.meta["first_offset"][s]) == b + own[s]["first_offset"]
    for s in (0, 1, 3, 5):
        assert not int(sc.meta["flags"][s]) & F_DIFFERS and int(sc.table[s][2]) == ranges[s][0] + own[s]["first_offset"]


# ------------------------------------------------------------------ 7. against the libFLAC stream API
def _stream_api_metadata(libflac, data: bytes):
    """init_stream over memory, process_until_end_of_metadata
    -> (return, get_decode_position, [the 72 leading bytes of each FLAC__StreamMetadata], error events)"""
    L = libflac.load()
    st = {"pos": 0}
    metas, errors = [], []

    def rd(d, buf, nbytes, ud):
        chunk = data[st["pos"]: st["pos"] + min(nbytes[0], 16384)]
        if chunk:
            ctypes.memmove(buf, chunk, len(chunk))
        st["pos"] += len(chunk)
        nbytes[0] = len(chunk)
        return 0 if chunk else 1

    def sk(d, off, ud):
        st["pos"] = int(off)
        return 0

    def tl(d, off, ud):
        off[0] = st["pos"]
        return 0

    def ln(d, n, ud):
        n[0] = len(data)
        return 0

    cbs = (libflac.DecoderReadCallback(rd), libflac.DecoderSeekCallback(sk), libflac.DecoderTellCallback(tl),
           libflac.DecoderLengthCallback(ln), libflac.DecoderEofCallback(lambda d, ud: 1 if st["pos"] >= len(data) else 0),
           libflac.DecoderWriteCallbackWithStatus(lambda d, f, b, ud: 0),
           libflac.Decoder_MetadataCallback(lambda d, m, ud: metas.append(ctypes.string_at(m, 72))),
           libflac.Decoder_ErrorCallback(lambda d, s, ud: errors.append(int(s))))
    dec = L.FLAC__stream_decoder_new()
    try:
        assert L.FLAC__stream_decoder_init_stream(dec, *cbs, None) == 0
        ok = int(L.FLAC__stream_decoder_process_until_end_of_metadata(dec))
        pos = ctypes.c_uint64(0)
        assert L.FLAC__stream_decoder_get_decode_position(dec, ctypes.byref(pos))
    finally:
        L.FLAC__stream_decoder_delete(dec)
    return ok, int(pos.value), metas, errors


def test_against_the_stream_api(gpu):
    torch, libflac, dec = gpu
    m = _parity(gpu)
    sc = m["scan"]
    checked = 0
    for s, (name, (b, e)) in enumerate(zip(m["names"], m["ranges"])):
        if name not in VARIANTS or int(sc.meta["status"][s]) != OK:
            continue
        ok, pos, metas, errors = _stream_api_metadata(libflac, VARIANTS[name])
        assert ok and not errors, name
        assert int(sc.meta["first_offset"][s]) - b == pos, name
        raw = metas[-1]  # the later STREAMINFO where there are two
        assert int.from_bytes(raw[0:4], "little") == 0, name
        u32 = lambda o: int.from_bytes(raw[o:o + 4], "little")
        got = (u32(16), u32(20), u32(24), u32(28), u32(32), u32(36), u32(40), int.from_bytes(raw[48:56], "little"))
        rec = sc.meta[s]
        assert got == tuple(int(rec[k]) for k in ("min_blocksize", "max_blocksize", "min_framesize", "max_framesize",
                                                  "sample_rate", "channels", "bps", "total_samples")), name
        assert raw[56:72] == sc.md5[s], name
        checked += 1
    assert checked == sum(ref_scan(d)[0] == KEPT for d in VARIANTS.values()) >= 14


# ------------------------------------------------------------------ 8. the chain, device tables only
def test_the_chain_on_device_tables(gpu):
    """scan_streams -> index_streams -> parse_frames / decode_parsed -> md5_streams on one
    non-default stream, each step fed by the device tables of the one before; the host reads
    nothing before the end."""
    from birdnest.audio_amd import synth
    torch, libflac, dec = gpu
    shape = [(12, 1001), (1, 14), (7, 0), (3, 13)]  # (frames, last blocksize; 0: a full block)
    syn = [synth.encode(synth.config("C2", nframes=nf, last_blocksize=lb, seed=11 + 7 * i)) for i, (nf, lb) in enumerate(shape)]
    raw = [s.data.tobytes() for s in syn]
    for d, s in zip(raw, syn):
        assert d[:8] == b"fLaC" + bytes([0x80, 0, 0, 34]) and int(s.frame_offsets[0]) == 42
    si = [d[8:42] for d in raw]
    empty_si = si[3][:13] + bytes([si[3][13] & 0xF0]) + bytes(4) + hashlib.md5(b"").digest()  # total_samples 0
    mono = golden_files()["mono_8bit_fixed.flac"]
    datas = [id3_tag(7) + raw[0],                                                                  # 12 frames, tagged
             b"fLaC" + blk(0, si[1]) + APP + SEEK + blk(1, b"", last=True) + raw[1][42:],          # 1 frame, extra blocks
             mono,                                                                                 # not a C2 stream
             b"fLaC" + blk(0, si[2][:18] + bytes(x ^ 0xFF for x in si[2][18:20]) + si[2][20:], last=True) + raw[2][42:],
             b"fLaC" + blk(0, empty_si, last=True),                                                # no frames
             raw[3]]
    heads = [17 + 42, 42 + 9 + 40 + 4, None, 42, 42, 42]
    gen = [syn[0], syn[1], None, syn[2], None, syn[3]]
    buf, ranges = _pack(datas, (0, 5, 16, 33, 1), lead=3)
    sp = libflac.StreamParams.from_synth(synth.config("C2"), 0)
    nframes, total = 23, sum(len(s.pcm) for s in syn)
    want_pcm = np.concatenate([s.pcm for s in syn]).astype("<i2").tobytes()
    d_bytes = _upload(torch, buf)
    d_out = torch.full((total * 4 + 64,), 0xAB, dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    d_tab, d_meta, d_exp, d_scan_st = dec.scan_streams(d_bytes, len(buf), ranges, expect=sp, stream=side)
    d_offs, d_os, d_info, d_sf, d_ss, d_ix_st = dec.index_streams(d_bytes, len(buf), d_tab, sp, 64, stream=side)
    dec.parse_frames(d_bytes, len(buf), d_offs, nframes, sp, d_info, d_out_sample=d_os, stream=side)
    dec.decode_parsed(d_bytes, len(buf), nframes, sp, libflac.OUT_FLACDECODER, d_out, d_info, stream=side)
    d_md5, d_v, d_md5_st = dec.md5_streams(d_out, libflac.OUT_FLACDECODER, sp, d_ss, 6, d_expected=d_exp, pcm_bytes=total * 4,
                                           stream=side)
    side.synchronize()  # the first host wait
    assert d_scan_st.cpu().tolist() == [2, 5, 0, 1]
    assert d_ix_st.cpu().tolist()[0] == 0
    sf, ss = d_sf.cpu().numpy(), d_ss.cpu().numpy()
    assert np.diff(sf).tolist() == [12, 1, 0, 7, 0, 3]
    assert np.diff(ss).tolist() == [len(g.pcm) if g is not None else 0 for g in gen]
    offs = d_offs[:nframes].cpu().numpy()
    for s, (g, (b, e)) in enumerate(zip(gen, ranges)):
        if g is not None:
            assert np.array_equal(offs[sf[s]:sf[s + 1]], g.frame_offsets.astype(np.int64) - 42 + heads[s] + b), s
    rec = libflac.info_array(d_info[: nframes * libflac.FRAME_INFO_BYTES].cpu().numpy())
    assert (rec["status"] == 0).all() and (rec["crc_ok"] == 1).all()
    assert d_out[: total * 4].cpu().numpy().tobytes() == want_pcm
    assert d_v.cpu().tolist() == [0, 0, 2, 1, 0, 0]  # the mono stream is not checked, the corrupted sum differs
    assert d_md5_st.cpu().tolist() == [0, 4, 1, 1]
    # the same frames from a table built on the host
    host_table = [(b, e, b + h, len(g.pcm)) if g is not None else (b, e, e if h is None else b + h, 0)
                  for (b, e), h, g in zip(ranges, heads, gen)]
    assert [tuple(int(x) for x in r) for r in d_tab.cpu().numpy().reshape(6, 4)] == host_table
    h_offs, h_os, h_info, h_sf, h_ss, h_st = dec.index_streams(d_bytes, len(buf), host_table, sp, 64)
    torch.cuda.synchronize()
    assert np.array_equal(h_sf.cpu().numpy(), sf) and np.array_equal(h_ss.cpu().numpy(), ss)
    assert np.array_equal(h_offs[:nframes].cpu().numpy(), offs)
    assert np.array_equal(h_os[:nframes].cpu().numpy(), d_os[:nframes].cpu().numpy())


# ------------------------------------------------------------------ 9. the Python entry points' other inputs
def test_device_table_in_place_and_no_streams(gpu):
    torch, libflac, dec = gpu
    datas = [VARIANTS["id3_127"], VARIANTS["junk_2"], VARIANTS["plain"]]
    buf, ranges = _pack(datas, (3, 0), lead=5)
    d_bytes = _upload(torch, buf)
    tab = np.full((3, 4), POISON64, dtype=np.uint64)  # first_offset and total_samples: whatever was there
    tab[:, :2] = ranges
    d_in = torch.from_numpy(tab.view(np.int64).reshape(-1).copy()).to(DEV)
    d_tab, d_meta, d_md5, d_st = dec.scan_streams(d_bytes, len(buf), d_in)
    torch.cuda.synchronize()
    assert d_tab.data_ptr() == d_in.data_ptr()  # completed in place
    want = [ref_scan(d, b, e) for d, (b, e) in zip(datas, ranges)]
    assert [tuple(int(x) for x in r) for r in d_in.cpu().numpy().reshape(3, 4)] == [(b, e) + w[2] for (b, e), w in zip(ranges, want)]
    assert [meta_tuple(r) for r in libflac.meta_array(d_meta.cpu().numpy())] == [w[1] for w in want]
    assert d_st.cpu().tolist() == [1, 2, 1, 0]
    with pytest.raises(ValueError):
        dec.scan_streams(d_bytes, len(buf), d_in[:6])
    with pytest.raises(ValueError):
        dec.index_streams(d_bytes, len(buf), d_in.to(torch.int32), libflac.StreamParams(1, 4096, 4096, 44100, 2, 16, 0), 8)
    # no streams: a zero status, from a host list and from an empty device table
    for none in ([], d_in[:0]):
        d_tab, d_meta, d_md5, d_st = dec.scan_streams(d_bytes, len(buf), none)
        torch.cuda.synchronize()
        assert d_st.cpu().tolist() == [0, 0, 0, 0] and d_tab.numel() == 0 and d_meta.numel() == 0 and d_md5.numel() == 0
    # the entry point's own checks
    L, vp = dec.L, lambda t: ctypes.c_void_p(t.data_ptr())
    hs = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.bnflac_scan_streams(dec.ctx, ctypes.c_void_p(d_bytes.data_ptr() + 8), 16, vp(d_in), 1, None, None, None, vp(d_st), hs) == -1
    assert b"16-byte aligned" in L.bnflac_last_error()
    assert L.bnflac_scan_streams(dec.ctx, vp(d_bytes), len(buf), None, 1, None, None, None, vp(d_st), hs) == -1
    assert L.bnflac_scan_streams(dec.ctx, vp(d_bytes), len(buf), vp(d_in), 1 << 30, None, None, None, vp(d_st), hs) == -1
    assert L.bnflac_scan_streams(dec.ctx, vp(d_bytes), len(buf), vp(d_in), 3, None, None, None, None, hs) == -1
    # d_meta and d_md5_expected may be NULL
    assert L.bnflac_scan_streams(dec.ctx, vp(d_bytes), len(buf), vp(d_in), 3, None, None, None, vp(d_st), hs) == 0
    torch.cuda.synchronize()
    assert d_st.cpu().tolist() == [1, 2, 1, 0]
