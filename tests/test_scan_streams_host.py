"""The metadata walk of bnflac_scan_streams on the host (bnflac_scan_stream_host, no GPU).

The reference is `ref_walk` / `ref_scan` below: the rule of include/bnflac.h restated in Python,
independent of the library.  Every comparison is exact.  The variants are byte surgery on
tests/golden/c2_lpc8.flac ("fLaC", one STREAMINFO block, frames); tests/test_gpu_scan_streams.py
uses the same variants and the same reference.
"""
import ctypes
import os
import subprocess

import pytest

import oracle
from birdnest.audio_amd import libflac
from birdnest.audio_amd._lib import lib_path

GOLD_DIR = os.path.join(os.path.dirname(__file__), "golden")
OK, NO_MARKER, TRUNCATED, NO_STREAMINFO, TOO_MANY_BLOCKS, BAD_RANGE = range(6)
MAX_BLOCKS = 1024
F_ID3, F_DIFFERS, F_MD5_ZERO, F_SEEKTABLE = 1, 2, 4, 8
KEPT, FAILED, DIFFERENT = 0, 1, 2
META_FIELDS = ("status", "flags", "nblocks", "id3_bytes", "has_stream_info", "min_blocksize", "max_blocksize",
               "sample_rate", "channels", "bps", "total_samples", "min_framesize", "max_framesize", "first_offset")


# ------------------------------------------------------------------ the reference
def ref_walk(b: bytes):
    """-> (status, flags, nblocks, id3_bytes, the last STREAMINFO's 34 bytes or None, bytes walked)"""
    n, p, flags, id3, nblocks, si = len(b), 0, 0, 0, 0, None
    if n >= 3 and b[0:3] == b"ID3":
        if n < 10:
            return TRUNCATED, flags, nblocks, id3, None, 0
        size = 0
        for x in b[6:10]:
            size = (size << 7) | (x & 0x7F)
        p = 10 + size
        flags |= F_ID3
        id3 = p
        if p > n:
            return TRUNCATED, flags, nblocks, id3, None, 0
    if p + 4 > n or b[p:p + 4] != b"fLaC":
        return NO_MARKER, flags, nblocks, id3, None, 0
    p += 4
    while True:
        if nblocks == MAX_BLOCKS:
            return TOO_MANY_BLOCKS, flags, nblocks, id3, None, 0
        if p + 4 > n:
            return TRUNCATED, flags, nblocks, id3, None, 0
        last, typ, length = b[p] >> 7, b[p] & 0x7F, int.from_bytes(b[p + 1:p + 4], "big")
        nblocks += 1
        if typ == 0:
            if length < 34:
                return NO_STREAMINFO, flags, nblocks, id3, None, 0
            if p + 38 > n:
                return TRUNCATED, flags, nblocks, id3, None, 0
            si = b[p + 4:p + 38]
        elif typ == 3:
            flags |= F_SEEKTABLE
        p += 4 + length
        if p > n:
            return TRUNCATED, flags, nblocks, id3, None, 0
        if last:
            break
    if si is None:
        return NO_STREAMINFO, flags, nblocks, id3, None, 0
    return OK, flags, nblocks, id3, si, p


def streaminfo_fields(si: bytes):
    """-> dict of the 34-byte block's fields (RFC 9639 section 8.2)"""
    x = int.from_bytes(si[10:18], "big")
    return dict(min_blocksize=int.from_bytes(si[0:2], "big"), max_blocksize=int.from_bytes(si[2:4], "big"),
                min_framesize=int.from_bytes(si[4:7], "big"), max_framesize=int.from_bytes(si[7:10], "big"),
                sample_rate=x >> 44, channels=((x >> 41) & 7) + 1, bps=((x >> 36) & 31) + 1,
                total_samples=x & ((1 << 36) - 1), md5=bytes(si[18:34]))


def ref_scan(b: bytes, begin=0, end=None, bad_range=False, expect=None):
    """One stream of a scan over its bytes b -> (kind, record as a tuple in META_FIELDS order,
    (first_offset, total_samples) of the descriptor, the 16 md5sum bytes).
    expect: None or (min_blocksize, max_blocksize, sample_rate, channels, bps)."""
    end = begin + len(b) if end is None else end
    status, flags, nblocks, id3, si, p = (BAD_RANGE, 0, 0, 0, None, 0) if bad_range else ref_walk(b)
    if status != OK:
        return FAILED, (status, flags, nblocks, id3) + (0,) * 9 + (end,), (end, 0), bytes(16)
    f = streaminfo_fields(si)
    if f["md5"] == bytes(16):
        flags |= F_MD5_ZERO
    own = (f["min_blocksize"], f["max_blocksize"], f["sample_rate"], f["channels"], f["bps"])
    differs = expect is not None and tuple(expect) != own
    if differs:
        flags |= F_DIFFERS
    rec = (OK, flags, nblocks, id3, 1) + own + (f["total_samples"], f["min_framesize"], f["max_framesize"], begin + p)
    if differs:
        return DIFFERENT, rec, (end, 0), bytes(16)
    return KEPT, rec, (begin + p, f["total_samples"]), f["md5"]


def meta_tuple(m):
    """A StreamMeta or a STREAM_META_DTYPE record -> a tuple in META_FIELDS order"""
    if isinstance(m, libflac.StreamMeta):
        return (m.status, m.flags, m.nblocks, m.id3_bytes, m.sp.has_stream_info, m.sp.min_blocksize, m.sp.max_blocksize,
                m.sp.sample_rate, m.sp.channels, m.sp.bps, m.sp.total_samples, m.min_framesize, m.max_framesize,
                m.first_offset)
    return tuple(int(m[k]) for k in META_FIELDS)


# ------------------------------------------------------------------ the variants
def blk(typ: int, body: bytes, last=False) -> bytes:
    return bytes([typ | (0x80 if last else 0)]) + len(body).to_bytes(3, "big") + body


def id3_tag(payload: int) -> bytes:
    size = bytes([(payload >> 21) & 0x7F, (payload >> 14) & 0x7F, (payload >> 7) & 0x7F, payload & 0x7F])
    return b"ID3\x03\x00\x00" + size + bytes([0x41 + i % 23 for i in range(payload)])


C2 = open(os.path.join(GOLD_DIR, "c2_lpc8.flac"), "rb").read()
assert C2[:4] == b"fLaC" and C2[4:8] == bytes([0x80, 0, 0, 34])
SI, FRAMES = C2[8:42], C2[42:]
# another STREAMINFO: same blocksizes, channels and bps; other frame sizes, rate, total and md5sum
_x = int.from_bytes(SI[10:18], "big")
SI2 = SI[0:4] + bytes([0, 0, 9, 0, 1, 2]) + ((48000 << 44) | (_x & ((1 << 44) - 1) & ~((1 << 36) - 1)) | 777).to_bytes(8, "big") \
    + bytes(range(1, 17))
APP = blk(2, b"test\x01")                                  # APPLICATION of 5 bytes
SEEK = blk(3, (b"\xff" * 8 + bytes(10)) * 2)               # SEEKTABLE of 36: two placeholder points
VC = blk(4, (4).to_bytes(4, "little") + b"test" + bytes(4))  # VORBIS_COMMENT: a vendor string, no comments
TAGGED = id3_tag(5) + b"fLaC" + blk(0, SI) + APP + SEEK + blk(1, b"", last=True) + FRAMES  # a tag and four blocks

VARIANTS = {
    "plain": C2,
    "extra_blocks": b"fLaC" + blk(0, SI) + APP + SEEK + blk(1, b"", last=True) + FRAMES,
    "streaminfo_not_first": b"fLaC" + VC + blk(0, SI, last=True) + FRAMES,
    "streaminfo_37": b"fLaC" + blk(0, SI + b"\xaa\xbb\xcc", last=True) + FRAMES,
    "streaminfo_twice": b"fLaC" + blk(0, SI) + blk(0, SI2, last=True) + FRAMES,
    "id3_0": id3_tag(0) + C2,
    "id3_1": id3_tag(1) + C2,
    "id3_127": id3_tag(127) + C2,
    "id3_128": id3_tag(128) + C2,
    "id3_300": id3_tag(300) + C2,
    "tagged_four_blocks": TAGGED,
    "md5_zero": b"fLaC" + blk(0, SI[:18] + bytes(16), last=True) + FRAMES,
    "blocks_1024": b"fLaC" + blk(0, SI) + blk(1, b"") * 1022 + blk(1, b"", last=True) + FRAMES,
    "ends_at_end": b"fLaC" + blk(0, SI) + blk(1, bytes(7), last=True),
    "streaminfo_33": b"fLaC" + blk(0, SI[:33], last=True) + FRAMES,
    "no_streaminfo": b"fLaC" + blk(1, bytes(8), last=True) + FRAMES,
    "never_last": b"fLaC" + blk(0, SI) + blk(1, bytes(4)),
    "never_last_frames": b"fLaC" + blk(0, SI) + blk(1, b"") + FRAMES,
    "padding_1025": b"fLaC" + blk(0, SI) + blk(1, b"") * 1024 + blk(1, b"", last=True) + FRAMES,
    "id3_twice": id3_tag(5) + id3_tag(5) + C2,
    "junk_2": b"\x00\x01" + C2,
    "id3_cut_header": b"ID3\x03\x00\x00\x00",
    "id3_past_end": id3_tag(300)[:200],
    "empty": b"",
}
WANT_STATUS = {
    "plain": OK, "extra_blocks": OK, "streaminfo_not_first": OK, "streaminfo_37": OK, "streaminfo_twice": OK, "id3_0": OK,
    "id3_1": OK, "id3_127": OK, "id3_128": OK, "id3_300": OK, "tagged_four_blocks": OK, "md5_zero": OK, "blocks_1024": OK,
    "ends_at_end": OK, "streaminfo_33": NO_STREAMINFO, "no_streaminfo": NO_STREAMINFO, "never_last": TRUNCATED,
    "padding_1025": TOO_MANY_BLOCKS, "id3_twice": NO_MARKER, "junk_2": NO_MARKER, "id3_cut_header": TRUNCATED,
    "id3_past_end": TRUNCATED, "empty": NO_MARKER,
}


def golden_files():
    return {f: open(os.path.join(GOLD_DIR, f), "rb").read() for f in sorted(os.listdir(GOLD_DIR))
            if os.path.isfile(os.path.join(GOLD_DIR, f))}


def all_cases():
    """name -> bytes: every file under tests/golden/ and every variant"""
    cases = dict(golden_files())
    cases.update(VARIANTS)
    return cases


def test_the_reference_on_the_variants():
    """The reference itself, against what each variant was built to be"""
    for name, want in WANT_STATUS.items():
        assert ref_walk(VARIANTS[name])[0] == want, name
    kind, rec, desc, md5 = ref_scan(VARIANTS["streaminfo_twice"])
    got = dict(zip(META_FIELDS, rec))
    assert (got["sample_rate"], got["total_samples"], got["nblocks"], md5) == (48000, 777, 2, bytes(range(1, 17)))
    kind, rec, desc, md5 = ref_scan(VARIANTS["extra_blocks"])
    got = dict(zip(META_FIELDS, rec))
    assert got["flags"] == F_SEEKTABLE and got["nblocks"] == 4 and desc[0] == 42 + 9 + 40 + 4
    assert [ref_scan(VARIANTS["id3_%d" % k])[1][3] for k in (0, 1, 127, 128, 300)] == [10, 11, 137, 138, 310]
    assert ref_scan(VARIANTS["ends_at_end"])[2][0] == len(VARIANTS["ends_at_end"])
    assert ref_scan(VARIANTS["md5_zero"])[1][1] == F_MD5_ZERO
    assert ref_scan(VARIANTS["blocks_1024"])[1][2] == 1024 and ref_walk(VARIANTS["padding_1025"])[2] == 1024
    assert ref_walk(golden_files()["rfc9639_ex2_frame1.bin"])[0] == NO_MARKER


# ------------------------------------------------------------------ the ABI
def test_record_layout():
    assert ctypes.sizeof(libflac.StreamMeta) == 64 and libflac.STREAM_META_DTYPE.itemsize == 64
    assert (libflac.StreamMeta.sp.offset, libflac.StreamMeta.min_framesize.offset, libflac.StreamMeta.first_offset.offset) == \
        (16, 48, 56)
    d = libflac.STREAM_META_DTYPE.fields
    assert (d["has_stream_info"][1], d["total_samples"][1], d["min_framesize"][1], d["first_offset"][1]) == (16, 40, 48, 56)
    assert (libflac.SCAN_OK, libflac.SCAN_NO_MARKER, libflac.SCAN_TRUNCATED, libflac.SCAN_NO_STREAMINFO,
            libflac.SCAN_TOO_MANY_BLOCKS, libflac.SCAN_BAD_RANGE) == (0, 1, 2, 3, 4, 5)
    assert libflac.SCAN_MAX_BLOCKS == 1024


def test_symbols_exported():
    names = {"bnflac_scan_streams", "bnflac_scan_stream_host"}
    assert names <= set(libflac.BATCH_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path("libbnflac.so")], capture_output=True, text=True).stdout
    assert names <= {l.split()[-1] for l in out.splitlines() if " T " in l}
    L = libflac.load()
    assert len(L.bnflac_scan_streams.argtypes) == 10 and len(L.bnflac_scan_stream_host.argtypes) == 4


# ------------------------------------------------------------------ the walk
def _assert_host_equals_ref(data: bytes, what):
    meta, md5 = libflac.scan_stream_host(data)
    kind, rec, desc, want_md5 = ref_scan(data)
    assert meta_tuple(meta) == rec, what
    assert md5 == want_md5, what
    return rec


def test_every_fixture_and_variant():
    statuses = {}
    for name, data in all_cases().items():
        statuses[name] = _assert_host_equals_ref(data, name)[0]
    assert statuses["rfc9639_ex2_frame1.bin"] == NO_MARKER
    assert statuses["c2_lpc8.flac"] == OK and statuses["mono_8bit_fixed.flac"] == OK
    for name, want in WANT_STATUS.items():
        assert statuses[name] == want, name


def test_every_cut_of_the_tagged_variant():
    first = ref_scan(TAGGED)[2][0]
    assert first == 15 + 4 + 38 + 9 + 40 + 4
    seen = set()
    for k in range(first + 2):
        seen.add(_assert_host_equals_ref(TAGGED[:k], k)[0])
    assert seen == {OK, NO_MARKER, TRUNCATED}
    assert ref_walk(TAGGED[:first])[0] == OK and ref_walk(TAGGED[:first - 1])[0] == TRUNCATED


def test_null_arguments():
    L = libflac.load()
    assert L.bnflac_scan_stream_host(None, 0, None, None) == -1
    meta = libflac.StreamMeta()
    assert L.bnflac_scan_stream_host(None, 4, ctypes.byref(meta), None) == -1
    assert L.bnflac_scan_stream_host(None, 0, ctypes.byref(meta), None) == 0 and meta.status == NO_MARKER


# ------------------------------------------------------------------ against the CPU oracle
def _streaminfo_events(events):
    """The oracle's leading metadata events (it reports STREAMINFO blocks only)"""
    lead = []
    for e in events:
        if e.kind != oracle.EV_METADATA:
            break
        lead.append(e)
    return lead


def test_ok_cases_against_the_oracle():
    """Where the walk says OK, libFLAC's first event is the STREAMINFO metadata event with the same
    fields.  (With two STREAMINFO blocks it sends two such events and goes on with the later one's
    values, as the walk does: the fields are compared with the last of the leading metadata events,
    which is the first one wherever there is one STREAMINFO.)"""
    nok = 0
    for name, data in all_cases().items():
        kind, rec, desc, md5 = ref_scan(data)
        if rec[0] != OK:
            continue
        nok += 1
        got = dict(zip(META_FIELDS, rec))
        events, _ = oracle.run(data)
        assert events and events[0].kind == oracle.EV_METADATA and events[0].status == 0, name
        lead = _streaminfo_events(events)
        assert len(lead) == (2 if name == "streaminfo_twice" else 1), name
        e = lead[-1]
        assert (e.blocksize, e.sample_rate, e.channels, e.bps, e.sample_number) == \
            (got["max_blocksize"], got["sample_rate"], got["channels"], got["bps"], got["total_samples"]), name
    assert nok >= 14 + 10


def test_junk_and_two_tags_against_the_oracle():
    for name in ("junk_2", "id3_twice"):
        events, _ = oracle.run(VARIANTS[name])
        assert events and events[0].kind == oracle.EV_ERROR, name
