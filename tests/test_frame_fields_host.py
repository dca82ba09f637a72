"""The hand-built frame table (tests/flac_frames.py) against the CPU oracle, without a GPU.

The writer proves itself on RFC 9639's first example, byte for byte.  Every in-spec row must then
decode in the oracle to exactly what restore() computes in unbounded integers, with the header
fields the row was written from and the frame's end on its last byte: two independent decoders,
so a disagreement is a wrong oracle or a row that is not in spec.  For the libFLAC-defined rows
(negative LPC shifts, refused fields) the oracle's verdict is what the GPU tests compare with; it
is pinned here, so a change of the oracle shows.  The table's own promises are counted too: the
share of rows each fast kernel keeps, and how many long frames it holds."""
import collections
import hashlib
import os

import numpy as np
import pytest

import oracle
from tests import flac_frames as F

GOLD_DIR = os.path.join(os.path.dirname(__file__), "golden")
LOST_SYNC, BAD_HEADER, UNPARSEABLE = 0, 1, 3  # FLAC__StreamDecoderErrorStatus


def oracle_params(row):
    return oracle.StreamParams(1, F.SI_BLOCKSIZE, F.SI_BLOCKSIZE, F.SI_RATE, row.channels, row.bps, 0) if row.si else None


def oracle_frame(row):
    """-> (rc, result, [channel][sample] or None)"""
    rc, res, planar = oracle.decode_frame_at(row.data, 0, oracle_params(row))
    pcm = None
    if rc == 0:
        pcm = planar[: res.channels * res.blocksize].reshape(res.channels, res.blocksize).tolist()
    return rc, res, pcm


@pytest.fixture(scope="module")
def decoded():
    return {r.name: oracle_frame(r) for r in F.rows()}


def test_writer_reproduces_rfc9639_example_1():
    data = open(os.path.join(GOLD_DIR, "rfc9639_ex1.flac"), "rb").read()
    subs = [{"type": "verbatim", "wasted": 2, "samples": [25588 >> 2]},
            {"type": "verbatim", "wasted": 4, "samples": [10416 >> 4]}]
    fr = F.frame(subs, 1, 16, number=0, bs_code=6, sr_code=9)
    assert fr == data[42:]
    pcm = F.frame_pcm(subs, 1, 16)
    assert pcm == [[25588], [10416]]
    assert F.stream([fr], [pcm], channels=2, bps=16, min_blocksize=4096, max_blocksize=4096) == data


def test_checksums_and_numbers_known_answers():
    assert F.crc8(b"123456789") == 0xF4 and F.crc16(b"123456789") == 0xFEE8
    assert F.utf8(0) == b"\x00" and F.utf8(0x7F) == b"\x7f" and F.utf8(0x80) == b"\xc2\x80"
    assert F.utf8((1 << 31) - 1) == b"\xfd\xbf\xbf\xbf\xbf\xbf" and F.utf8((1 << 36) - 1) == b"\xfe" + b"\xbf" * 6
    assert F.utf8(0, 2) == b"\xc0\x80"


def test_table_is_deterministic_and_named_once():
    rows = F.rows()
    assert len({r.name for r in rows}) == len(rows)
    rebuilt = F._Table()
    import random
    F._group_d(rebuilt, random.Random(9639 + 3))
    assert [r.data for r in rebuilt.rows] == [r.data for r in rows if r.group == "D"]


def test_in_spec_rows_decode_to_the_exact_restore(decoded):
    n = 0
    for r in F.rows():
        if r.expect != "restore":
            continue
        rc, res, pcm = decoded[r.name]
        assert rc == 0 and res.crc_ok == 1 and res.error == -1, (r.name, rc, res.error)
        assert res.end_off == len(r.data), r.name
        for k, v in r.fields.items():
            assert int(getattr(res, k)) == v, (r.name, k)
        assert pcm == r.pcm, r.name
        n += 1
    assert n >= 450


def test_negative_shift_rows_decode_inside_the_sample_range(decoded):
    """libFLAC-defined, yet ordinary frames: status OK, CRC good, and (what the kept / handed-back
    marks assume) every sample inside the frame's range: int16 in the 16-bit carriers."""
    rows = [r for r in F.rows() if r.group == "E"]
    assert {s["shift"] for r in rows for s in r.subs if s["type"] == "lpc"} >= {-1, -3, -16}
    for r in rows:
        assert r.expect == "oracle" and r.assignment == r.channels - 1
        rc, res, pcm = decoded[r.name]
        assert rc == 0 and res.crc_ok == 1 and res.end_off == len(r.data), r.name
        lo, hi = -(1 << (r.bps - 1)), (1 << (r.bps - 1)) - 1
        for ch, (s, c) in enumerate(zip(r.subs, pcm)):
            w = s.get("wasted", 0)
            assert all(lo <= v <= hi and v & ((1 << w) - 1) == 0 for v in c), (r.name, ch)
            if s["type"] == "lpc" and F.lpc_path(r.bps - w, s["prec"], s["order"]) == "mmx16":
                assert all(-32768 <= v >> w <= 32767 for v in c), (r.name, ch)


# the oracle's verdict on each refused (or, against RFC 9639, accepted) field: error status, or None
H_VERDICTS = {
    "subframe_type": UNPARSEABLE, "precision_code15": LOST_SYNC, "coding_method": UNPARSEABLE,
    "partition_shorter_than_order": LOST_SYNC, "blocksize_below_order": LOST_SYNC,
    "partitions_do_not_divide_blocksize": UNPARSEABLE, "first_bit_set": LOST_SYNC, "wasted_equals_bps": None,
    "wasted_is_bps_plus_1": UNPARSEABLE, "assignment": UNPARSEABLE, "bps_code": UNPARSEABLE, "sr_code15": BAD_HEADER,
    "bs_code0": UNPARSEABLE, "blocksize_65536": None, "reserved_bit": UNPARSEABLE, "padding_not_zero": LOST_SYNC,
    "header_byte": BAD_HEADER, "number_": BAD_HEADER,
}


def test_refused_fields_verdicts(decoded):
    seen = set()
    for r in F.rows():
        if r.expect != "oracle" or r.group == "E":
            continue
        rc, res, pcm = decoded[r.name]
        if r.group == "G":  # codes that point at a STREAMINFO there is none of
            want = UNPARSEABLE
        else:
            key = [k for k in H_VERDICTS if r.name.startswith("H/" + k)]
            assert len(key) == 1, r.name
            seen.add(key[0])
            want = H_VERDICTS[key[0]]
        if want is None:
            assert rc == 0 and res.crc_ok == 1 and res.end_off == len(r.data), (r.name, rc)
            assert res.blocksize == r.blocksize, r.name
            if r.name.startswith("H/wasted"):  # no bits left: every sample is 0
                assert not any(pcm[0]), r.name
        else:
            assert rc == 1 + want and res.error == want, (r.name, rc, res.error)
            assert 3 <= res.end_off <= len(r.data) - 2, r.name  # refused before the frame's end: nothing is cut short
    assert seen == set(H_VERDICTS)


def _stream_of(rows):
    frames = [r.data for r in rows]
    pcm = [r.pcm for r in rows]
    r0 = rows[0]
    # STREAMINFO's total left at "unknown": the rows' frame numbers do not count up, and libFLAC ends a
    # stream at the frame whose number reaches the total
    data = F.stream(frames, pcm, channels=r0.channels, bps=r0.bps, sample_rate=F.SI_RATE, total=0)
    return data, pcm, sum(r.blocksize for r in rows)


STREAMS = {c: (lambda r, c=c: r.carrier == c and r.expect == "restore" and r.blocksize <= 4096 and r.bps == F.CARRIERS[c][1])
           for c in F.CARRIERS}
STREAMS["G_mono"] = lambda r: r.group == "G" and r.expect == "restore" and r.si and r.channels == 1
STREAMS["G_stereo"] = lambda r: r.group == "G" and r.expect == "restore" and r.si and r.channels == 2


@pytest.mark.parametrize("which", sorted(STREAMS))
def test_streams_through_the_oracle(which):
    """Whole streams through the oracle's libFLAC state machine (sync search, STREAMINFO, one write
    per frame): the writes are the concatenated restore() output, and they hash to the STREAMINFO
    MD5 that the stream writer computed from restore()'s samples."""
    rows = [r for r in F.rows() if STREAMS[which](r)]
    if not which.startswith("G"):
        rows = rows[::7]  # a spread over the groups; the G streams hold every header row
    assert len(rows) >= 4 and len({(r.channels, r.bps) for r in rows}) == 1
    data, pcm, total = _stream_of(rows)
    ev, opcm = oracle.run(data)
    assert not [e for e in ev if e.kind == oracle.EV_ERROR], which
    writes = [e for e in ev if e.kind == oracle.EV_WRITE]
    assert [e.blocksize for e in writes] == [r.blocksize for r in rows]
    want = np.concatenate([np.array(p, dtype=np.int64).T for p in pcm]).astype(np.int32)
    got = oracle.interleave(ev, opcm)
    assert got.shape == (total, rows[0].channels) and np.array_equal(got, want)
    nb = (rows[0].bps + 7) // 8
    raw = np.ascontiguousarray(got, dtype="<i4").view(np.uint8).reshape(-1, 4)[:, :nb].tobytes()
    assert hashlib.md5(raw).digest() == data[26:42]


def kept_counts(rows=None):
    """{group: {kernel: (kept, instantiated)}} of the residual and predictor groups"""
    out = collections.OrderedDict()
    for g in "ABCDEF":
        rs = [r for r in (rows or F.rows()) if r.group == g]
        st = [r for r in rs if r.carrier == "S16"]
        sw = [r for r in rs if r.carrier == "S24"]
        out[g] = {"k_decode_st": (sum(r.kernel == "k_decode_st" and r.lane_kept for r in st), len(st)),
                  "k_decode_sw": (sum(r.kernel == "k_decode_sw" and r.lane_kept for r in sw), len(sw)),
                  "k_decode_sys": (sum(r.sys_kept for r in rs), len(rs))}
    return out


def test_each_fast_kernel_keeps_at_least_half_of_its_rows():
    """A hand-back must not hide a broken fast path: in every group the rows built for k_decode_st
    (carrier S16), k_decode_sw (S24) and k_decode_sys (all) are mostly rows those kernels keep."""
    for g, per in kept_counts().items():
        for kernel, (kept, n) in per.items():
            assert n > 0 and 2 * kept >= n, (g, kernel, kept, n)
    # ... and the table also holds rows each of them must hand back, so that mark is tested as well
    for kernel in ("k_decode_st", "k_decode_sw", "k_decode_sys"):
        assert sum(n - kept for per in kept_counts().values() for k, (kept, n) in per.items() if k == kernel) >= 5, kernel


def test_carriers_reach_their_kernels():
    by = collections.Counter((r.carrier, r.kernel) for r in F.rows() if r.marks)
    for carrier, (_, _, _, kernel) in F.CARRIERS.items():
        n = sum(v for (c, _), v in by.items() if c == carrier)
        assert by[(carrier, kernel)] >= n - 2, (carrier, by)  # all but the VERBATIM rows of group F


def test_table_size():
    rows = F.rows()
    assert 300 <= len(rows) <= 700
    long_coded = [r.name for r in rows if r.blocksize >= 4096 and r.coded]
    assert len(long_coded) <= 6, long_coded  # residual-coded frames; the long header rows hold one CONSTANT each
    assert sum(r.blocksize < 200 for r in rows) >= 0.93 * len(rows)
    assert not [r.name for r in rows if r.group in "ABDEF" and not 16 <= r.blocksize <= 192]
