"""tests/decoy_streams.py certified on the CPU: no GPU code is touched.

Every row goes through the CPU oracle, which must deliver exactly the row's true frames (blocksize,
sample number, PCM) and no error, and every decoy is checked to be what its class claims with
flac_frames' own CRC-8 / CRC-16.  One row is libFLAC-defined instead: behind trailing junk, with
STREAMINFO's total unknown, libFLAC reports the lost sync and decodes the frame in the junk too;
oracle_frames() returns what it delivered and the GPU test takes that as the expectation.
"""
import numpy as np
import pytest

from tests import decoy_streams as D
from tests.flac_frames import crc8, crc16, utf8

ROWS = D.rows()
NAMES = [r.name for r in ROWS]


def oracle_frames(data):
    """-> ([(sample number, blocksize, pcm[channel][sample] as lists)], number of error callbacks)"""
    import oracle
    ev, pcm = oracle.run(data)
    out = []
    for e in ev:
        if e.kind == oracle.EV_WRITE:
            n = e.blocksize * e.channels
            out.append((int(e.sample_number), int(e.blocksize),
                        pcm[e.pcm_offset: e.pcm_offset + n].reshape(e.channels, e.blocksize).tolist()))
    return out, sum(e.kind == oracle.EV_ERROR for e in ev)


def truth(r):
    out, n = [], 0
    for p in r.pcm:
        out.append((n, len(p[0]), p))
        n += len(p[0])
    return out


def header_len(data, off):
    """length of the frame header at off, by its codes (RFC 9639 section 9.1)"""
    lead = data[off + 4]
    nnum = 1 if lead < 0x80 else 8 - (lead ^ 0xFF).bit_length()
    bs_code, sr_code = data[off + 2] >> 4, data[off + 2] & 15
    return 4 + nnum + {6: 1, 7: 2}.get(bs_code, 0) + {12: 1, 13: 2, 14: 2}.get(sr_code, 0) + 1


def crc8_ok(data, off):
    n = header_len(data, off)
    return crc8(data[off: off + n - 1]) == data[off + n - 1]


def last_subframe(r, k):
    """byte offset of the header byte of frame k's last subframe"""
    plen = r.blocksize * r.bps // 8
    return r.frame_ends[k] - 2 - plen - 1


@pytest.mark.parametrize("name", NAMES)
def test_oracle_delivers_the_true_frames(name):
    r = D.row(name)
    got, errors = oracle_frames(r.data)
    want = truth(r)
    if name == "S16/tail_total_0":  # libFLAC-defined: the row records the oracle's answer
        assert got[: len(want)] == want and errors == 1
        # the tail frame, at its header's frame number times STREAMINFO's blocksize
        assert [(n, bs) for n, bs, _ in got[len(want):]] == [(4 * r.blocksize, D.NESTED_BS)]
        return
    assert errors == 0
    assert [(n, bs) for n, bs, _ in got] == [(n, bs) for n, bs, _ in want]
    assert got == want


@pytest.mark.parametrize("name", NAMES)
def test_decoys_are_what_their_class_claims(name):
    r = D.row(name)
    data = r.data
    pairs = D.sync_pairs(data).tolist()
    assert all(o in pairs for o in r.frame_offsets)
    assert 3 <= len(r.frame_offsets) <= 12
    if r.kind not in ("window-under", "window-over", "seam"):  # nothing else looks like a frame start
        assert pairs == sorted(r.frame_offsets + [d.offset for d in r.decoys])
    for d in r.decoys:
        off, cls = d.offset, d.cls
        assert off in pairs and off not in r.frame_offsets
        if cls == "window":
            lo, hi = r.frame_offsets[0], r.frame_ends[0]
            inside = sum(lo < p < hi for p in pairs)
            assert inside == d.inside == (D.CHAIN_WIN - 1 if r.kind == "window-under" else D.CHAIN_WIN)
            assert pairs[pairs.index(lo) + inside + 1] == r.frame_offsets[1]
            continue
        if cls == "pair":
            assert data[off + 3] & 1 and crc8_ok(data, off)  # only the reserved bit stops it
            continue
        if cls == "crc8":
            assert not crc8_ok(data, off) and not data[off + 3] & 1 and not data[off + 1] & 2
            continue
        assert crc8_ok(data, off)
        n = header_len(data, off)
        stereo = data[off + 3] >> 4 == 1
        if cls == "walk":
            assert stereo and data[off + n: off + n + 1] == D.SUB_RESERVED
        elif cls == "trunc":
            assert stereo and data[off + 2] >> 4 == 15 and d.frame == len(r.frame_offsets) - 1
            assert off + n + 1 + 32768 * 2 > len(data) and data[off + n: off + n + 1] == D.SUB_VERBATIM
        elif cls == "straddle":
            assert stereo and off >= r.frame_ends[-1] and off + n + 1 + 256 * 2 > len(data)
        else:
            assert data[off + 3] >> 4 == 0  # mono: no subframe to walk
        if cls in ("meta", "tail", "straddle"):
            if cls == "meta":
                assert off + D.NESTED_LEN == r.first == r.frame_offsets[0] and crc16(data[off: r.first]) == 0
            if cls == "tail":
                assert off + D.NESTED_LEN == len(data) and crc16(data[off:]) == 0
                assert crc16(data[r.frame_offsets[-1]: off]) != 0  # the junk keeps the chain from closing at it
            continue
        # inside frame d.frame's payload
        k = d.frame
        assert r.frame_offsets[k] < off < r.frame_ends[k] - 2
        closes = crc16(D.decoy_frame_bytes(r, d)) == 0
        assert closes == d.tuned == (cls not in ("valid", "walk", "trunc"))
        if cls == "close-early":
            assert off + n <= last_subframe(r, k)
        if cls in ("close-last", "nested", "nested-n"):
            assert off > last_subframe(r, k)
        if cls in ("nested", "nested-n"):
            assert crc16(data[off: r.frame_ends[k]]) == 0 and off + D.NESTED_LEN == r.frame_ends[k]
        if cls in ("nested", "nested-n", "close-last", "close-early"):
            assert data[off + 4: off + 4 + len(utf8(d.number))] == utf8(d.number)
        if cls == "nested" or r.kind == "close-last":
            assert d.number == k + 1
        if cls == "nested-n" or r.kind == "nested-n":
            assert d.number != k + 1


def test_damage_variants_keep_every_length():
    """Every damage variant of every row: one CRC-16 failure, every frame still delivered at its
    place and the damaged one as zeros; a variant a row lacks has its reason written down."""
    count = 0
    for r in ROWS:
        have, absent = D.damage_variants(r)
        assert set(have) | set(absent) == {"before", "behind"} and not set(have) & set(absent), r.name
        assert all(absent.values())
        for where in have:
            count += 1
            data, lost = D.damaged(r, where)
            assert len(data) == len(r.data) and D.sync_pairs(data).tolist()[:8] == D.sync_pairs(r.data).tolist()[:8]
            if not r.kind.startswith("window"):
                assert D.sync_pairs(data).tolist() == D.sync_pairs(r.data).tolist()
            got, errors = oracle_frames(data)
            want = truth(r)
            assert errors == 1 and [(n, bs) for n, bs, _ in got] == [(n, bs) for n, bs, _ in want], (r.name, where)
            for k, (g, w) in enumerate(zip(got, want)):
                assert (not np.any(g[2])) if k == lost else g == w, (r.name, where, k)
            d = r.decoys[0]
            if isinstance(d.frame, int) and d.cls != "window":  # the damage lies outside [frame start, decoy)
                assert (crc16(D.decoy_frame_bytes(r, d)) == 0) == d.tuned
    # every must-equal row with a carrier frame has at least one variant, all but `trunc` (the last frame) both
    for r in ROWS:
        have, absent = D.damage_variants(r)
        if not r.limit and r.kind != "trunc":
            assert have, r.name
            if isinstance(r.decoys[0].frame, int) and r.decoys[0].frame >= 1:
                assert set(have) == {"before", "behind"}, r.name
    assert count == sum(len(D.damage_variants(r)[0]) for r in ROWS) > len(ROWS)


def test_batch_layout():
    buf, ranges, members, loose = D.batch()
    pairs = D.sync_pairs(buf).tolist()
    assert any(m is None for m in members) and any(b & 1 for b, _ in ranges)
    for (b, e), m in zip(ranges, members):
        assert buf[b:e] == (m.data if m else b"")
    (off, cls), = loose
    assert cls == "gapdecoy" and off in pairs and crc8_ok(buf, off) and crc16(buf[off: off + D.NESTED_LEN]) == 0
    assert not any(b <= off < e for b, e in ranges)
    s = [m.name if m else None for m in members].index("S16/straddle")
    d = members[s].decoys[0]
    at = ranges[s][0] + d.offset
    assert ranges[s + 1][0] == ranges[s][1]  # its subframe 0 would end inside the next stream
    assert at + header_len(buf, at) + 1 + 512 > ranges[s][1] and at + 2 <= ranges[s][1]
