"""The frame indexers and what is built on them against decoy frame starts (tests/decoy_streams.py).

The indexers never decode a frame to find its end: they link sync candidates by CRC-16 algebra
(k_chain_succ / k_ms_succ).  libFLAC decodes the frame and goes on where it ends.  The rows put
sync codes inside payloads, metadata, junk and gaps, up to whole valid frames, and where the class
says so the CRC-16 from the carrying frame's start closes at them.  The rule for every consumer and
row: libFLAC's answer, or an explicit refusal or status, never a silently different frame list.

The references are independent of the product: the rows' own frame offsets and PCM
(flac_frames.frame_pcm) and the CPU oracle, both certified by tests/test_decoy_streams_host.py.
Everything is exact.  Non-vacuity is a condition of every row: the decoy is a sync candidate of
bnflac_index_frames, and carries the VALID flag of the candidate table exactly when its class says
that it parses.  Damaged bytes are ordinary input: no test provokes a device fault.

The stated limits ("Decoys"), pinned here as they are:
  * window-over: more than CHAIN_WIN candidates inside one frame.  The plain chain ends at that
    frame; the stream's samples stay short of STREAMINFO's total, and the reader refuses to open.
    index_streams_resync resumes at the next frame and flags the stream RESYNCED.
  * close-last / nested with a continuing number: a decoy in the last subframe whose header number
    continues the carrier's.  Nothing short of decoding the last subframe tells it from the
    successor, so the plain indexers take it for the next frame: the stream's samples then differ
    from STREAMINFO's total (the caller's tell), index_streams_resync ends the stream with
    CONTRADICTION, and the reader refuses to open.
  * tail-total0: a whole valid frame behind junk that follows the last frame, STREAMINFO's total 0.
    libFLAC reports the lost sync and decodes that frame too; the three indexers end at the junk
    with the true frames and no flag.  The tell is a VALID candidate behind the chain's last frame
    in the candidate table; the reader refuses to open by the same test, and the stream API gives
    libFLAC's sequence.
"""
import numpy as np
import pytest

from tests import decoy_streams as D
from tests.conftest import gpu_available
from tests.test_decoy_streams_host import oracle_frames, truth
from tests.test_gpu_index_resync import CONTRADICTION, RESYNCED, RBatch, assert_geometry, assert_plan
from tests.test_gpu_index_streams import Batch, _stream_params, _upload

pytestmark = pytest.mark.gpu

ROWS = D.rows()
NAMES = [r.name for r in ROWS]
EQUAL = [r.name for r in ROWS if not r.limit]
LIMIT = [r.name for r in ROWS if r.limit]


@pytest.fixture(scope="module")
def gpu():
    if not gpu_available():
        pytest.skip("no GPU")
    import torch
    from birdnest.audio_amd import libflac
    return torch, libflac, libflac.BatchDecoder(0)


def _truth_pcm(r):
    """[samples, channels] of the row's true frames"""
    return np.concatenate([np.array(p, dtype=np.int32).T for p in r.pcm])


def _expected(r):
    """(frame offsets, out_sample of each, total samples) libFLAC's frame list gives"""
    sizes = [len(p[0]) for p in r.pcm]
    return r.frame_offsets, np.concatenate([[0], np.cumsum(sizes)])[:-1].tolist(), sum(sizes)


@pytest.fixture(scope="module")
def ctx(gpu):
    """row -> that row indexed alone by all three indexers, once; the device buffers go with the module"""
    cache = {}

    def get(r):
        if r.name not in cache:
            cache[r.name] = _index_alone(gpu, r)
        return cache[r.name]
    yield get
    cache.clear()


def _index_alone(gpu, r):
    torch, libflac, dec = gpu
    data = r.data
    sp = _stream_params(libflac, data)
    table = [(0, len(data), r.first, int(sp.total_samples))]
    cap = len(data) // 16 + 16
    d_bytes = _upload(torch, data)
    d_offs = torch.zeros(cap * 16, dtype=torch.int64, device="cuda:0")
    d_cnt = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    dec.index_frames(d_bytes, len(data), d_offs, d_cnt)
    torch.cuda.synchronize()
    sync = d_offs[: int(d_cnt[0].item())].cpu().numpy()
    offs, os_, info, nf = dec.index_stream(d_bytes, len(data), r.first, sp, cap)
    assert nf <= cap
    alone = (offs[:nf].cpu().numpy(), os_[:nf].cpu().numpy(),
             libflac.info_array(info[: nf * libflac.FRAME_INFO_BYTES].cpu().numpy()))
    sp0 = _stream_params(libflac, data, 0)  # a batch keeps the totals in its table
    cand_cap = len(sync) + 64  # the window rows hold more candidates than the default bound
    plain = Batch(gpu, data, table, sp0, cand_cap=cand_cap, d_bytes=d_bytes)
    rb = RBatch(gpu, data, table, sp0, cand_cap=cand_cap)
    return dict(sync=sync, alone=alone, plain=plain, rb=rb, sp=sp)


def _flag_of(cands, offset):
    k = np.flatnonzero(cands["offset"].astype(np.int64) == offset)
    assert len(k) == 1, "the decoy is no candidate of the table"
    return int(cands["flags"][k[0]]) & 1, int(k[0])


# ------------------------------------------------------------------ 1. non-vacuity
@pytest.mark.parametrize("name", NAMES)
def test_decoys_are_candidates(gpu, ctx, name):
    """A condition, not a result: a row that fails here is a broken fixture."""
    r = D.row(name)
    c = ctx(r)
    assert np.array_equal(c["sync"], D.sync_pairs(r.data))
    cands = c["rb"].cands
    for off in r.frame_offsets:
        assert _flag_of(cands, off)[0] == 1
    for d in r.decoys:
        assert d.offset in c["sync"]
        valid, k = _flag_of(cands, d.offset)
        assert valid == int(d.valid), (name, d.cls)
        if r.kind == "seam":
            assert k == r.seam_index


# ------------------------------------------------------------------ 2. the three indexers, intact rows
def _assert_frames(r, offs, os_, total, what):
    want_offs, want_os, want_total = _expected(r)
    assert list(map(int, offs)) == want_offs, what
    assert list(map(int, os_)) == want_os, what
    assert int(total) == want_total, what


@pytest.mark.parametrize("name", EQUAL)
def test_indexers_give_the_true_frames(gpu, ctx, name):
    torch, libflac, dec = gpu
    r = D.row(name)
    c = ctx(r)
    a_offs, a_os, a_rec = c["alone"]
    plain, rb = c["plain"], c["rb"]
    _assert_frames(r, a_offs, a_os, a_rec["blocksize"].sum(), "index_stream")
    _assert_frames(r, plain.offs, plain.os, plain.ss[1], "index_streams")
    _assert_frames(r, rb.offs, rb.os, rb.ss[1], "index_streams_resync")
    assert plain.status[0] == 0 and np.array_equal(plain.sf, [0, len(r.frame_offsets)])
    # one stream at offset 0: the three write the same records
    assert plain.rec.tobytes() == a_rec.tobytes()
    assert rb.rec.tobytes() == plain.rec.tobytes() and rb.status.tolist() == plain.status.tolist()
    assert np.array_equal(rb.sf, plain.sf) and np.array_equal(rb.ss, plain.ss.astype(np.int64))
    assert int(rb.rs["flags"][0]) & (RESYNCED | CONTRADICTION) == 0 and int(rb.rs["flags"][0]) == 0
    assert int(rb.rs["gap_frames"][0]) == 0 and int(rb.rs["segments"][0]) == 1
    assert_plan(gpu, rb)
    pcm, rec = rb.decode(gpu)
    assert (rec["status"] == 0).all() and (rec["crc_ok"] == 1).all()
    assert np.array_equal(pcm, _truth_pcm(r))


# ------------------------------------------------------------------ 3. the stated limits
@pytest.mark.parametrize("name", LIMIT)
def test_indexers_at_the_stated_limits(gpu, ctx, name):
    """Not libFLAC's frame list, but one the caller can tell from it (module docstring)."""
    r = D.row(name)
    c = ctx(r)
    a_offs, a_os, a_rec = c["alone"]
    plain, rb = c["plain"], c["rb"]
    want_offs, want_os, want_total = _expected(r)
    assert_plan(gpu, rb)
    if r.kind == "window-over":
        for offs, total in ((a_offs, a_rec["blocksize"].sum()), (plain.offs, plain.ss[1])):
            assert list(map(int, offs)) == want_offs[:1] and int(total) == r.blocksize < want_total
        # the resync variant takes the missing link for damage and resumes at frame 1: the true frames, flagged
        assert list(map(int, rb.offs)) == want_offs and list(map(int, rb.os)) == want_os and int(rb.ss[1]) == want_total
        assert int(rb.rs["flags"][0]) == RESYNCED and rb.status[0] == 8 and rb.status[3] == 0
        return
    d = r.decoys[0]
    if r.kind == "tail-total0":
        # libFLAC (host-certified): the four frames, one lost-sync error for the junk, then the frame in
        # the junk, 64 samples at its header's number.  An index ends at junk as at any damage, and the
        # resync rule resumes only at a frame of the stream's blocksize that has a successor.
        got, errors = oracle_frames(r.data)
        assert errors == 1 and [(n, bs) for n, bs, _ in got[len(want_offs):]] == [(4 * r.blocksize, D.NESTED_BS)]
        for offs, total in ((a_offs, a_rec["blocksize"].sum()), (plain.offs, plain.ss[1]), (rb.offs, rb.ss[1])):
            assert list(map(int, offs)) == want_offs and int(total) == want_total
        assert plain.status[0] == 0 and rb.status[0] == 0 and int(rb.rs["flags"][0]) == 0
        # the tell, with no total to compare with: a candidate that parses as a frame start lies behind
        # the chain's last frame, in the table index_streams_resync leaves (the reader refuses by it)
        valid, k = _flag_of(rb.cands, d.offset)
        last = _flag_of(rb.cands, want_offs[-1])[1]
        assert valid == 1 and k > last and rb.cands["succ"][last] == -1 and rb.cands["stream"][k] == 0
        return
    k = d.frame
    # The decoy is taken for frame k + 1.  From it the CRC-16 closes at frame k + 1 and at frame k + 2;
    # frame k + 2 carries the number that continues the decoy's, so it is the successor.
    with_decoy = want_offs[: k + 1] + [d.offset] + want_offs[k + 2:]
    assert k + 2 < len(want_offs)
    for offs, total in ((a_offs, a_rec["blocksize"].sum()), (plain.offs, plain.ss[1])):
        assert list(map(int, offs)) == with_decoy
        assert int(total) == want_total - r.blocksize + D.NESTED_BS != r.total  # the caller's tell
    # the resync variant checks the positions across every link: the stream ends behind the decoy, flagged
    assert list(map(int, rb.offs)) == with_decoy[: k + 2]
    assert int(rb.rs["flags"][0]) == CONTRADICTION and rb.status[0] == 16


# ------------------------------------------------------------------ 4. damage next to the decoy
def _damage_batches():
    """{carrier: [(row, 'before' | 'behind')]}: every variant decoy_streams.damage_variants gives"""
    out = {}
    for r in ROWS:
        for w in D.damage_variants(r)[0]:
            out.setdefault(r.carrier, []).append((r, w))
    return out


@pytest.mark.parametrize("carrier", sorted(_damage_batches()))
def test_resync_never_keeps_a_decoy(gpu, carrier):
    """One body byte flipped in the frame before the carrier, and in the carrier behind the decoy,
    for every row that has the frames (decoy_streams.damage_variants says why a row lacks one).  The
    oracle delivers every frame at its place, the damaged one as zeros (host-certified), and so do
    the records: no placeholder, no decoy, one resync step.
    The rows at the last-subframe limit run 'before' only and pin the limit after a resync step:
    the carrier is resumed at, the decoy follows it as at the intact row, and the link out of the
    decoy ends the stream with CONTRADICTION."""
    torch, libflac, dec = gpu
    cases = [(r, w) + D.damaged(r, w) for r, w in _damage_batches()[carrier]]
    buf, ranges = bytearray(), []
    for n, (r, w, data, lost) in enumerate(cases):
        ranges.append((len(buf), len(buf) + len(data)))
        buf += data + bytes([0xF8, 0xFF] * 8)[: (3 * n) % 16]
    buf = bytes(buf)
    table = [(b, e, b + r.first, r.total) for (b, e), (r, w, data, lost) in zip(ranges, cases)]
    sp = _stream_params(libflac, cases[0][2], 0)
    rb = RBatch(gpu, buf, table, sp, cand_cap=len(D.sync_pairs(buf)) + 64)
    assert_plan(gpu, rb)
    pcm, rec = rb.decode(gpu)
    for s, (r, w, data, lost) in enumerate(cases):
        n, bs, begin, d = len(r.frame_offsets), r.blocksize, table[s][0], r.decoys[0]
        sl = rb.stream(s)
        got = [int(x) - begin for x in rb.offs[sl]]
        flags = int(rb.rs["flags"][s])
        if r.limit:
            k = d.frame
            assert got == r.frame_offsets[: k + 1] + [d.offset], (r.name, w)
            assert flags == RESYNCED | CONTRADICTION and not rb.gap(s).any()
            assert int(rb.ss[s + 1] - rb.ss[s]) == (k + 1) * bs + D.NESTED_BS
            continue
        assert got == r.frame_offsets, (r.name, w, flags)  # never the decoy
        assert [int(x) - int(rb.ss[s]) for x in rb.os[sl]] == [k * bs for k in range(n)]
        assert int(rb.ss[s + 1] - rb.ss[s]) == n * bs and not rb.gap(s).any() and int(rb.rs["gap_frames"][s]) == 0
        if bs == 256:
            assert_geometry(rb, s, begin, r.frame_offsets + [len(data)], [True] * n)
        # the last frame damaged (a decoy in trailing junk): still a chain member, nothing to resume at
        resumed = lost < n - 1
        assert (flags, int(rb.rs["segments"][s])) == ((RESYNCED, 2) if resumed else (0, 1)), (r.name, w)
        want = _truth_pcm(r)
        want[lost * bs: (lost + 1) * bs] = 0
        assert np.array_equal(pcm[int(rb.ss[s]): int(rb.ss[s + 1])], want), (r.name, w)
        ok = rec["crc_ok"][sl]
        assert ok[lost] == 0 and np.delete(ok, lost).all() and (rec["status"][sl] == 0).all()


# ------------------------------------------------------------------ 5. a batch, gaps and the scan seams
def test_batch_of_rows(gpu):
    """Ten streams in one buffer: junk gaps, an empty stream, a header straddling a stream's end and a
    whole valid frame in a gap."""
    torch, libflac, dec = gpu
    buf, ranges, members, loose = D.batch()
    table = [(b, e, b + (m.first if m else 0), m.total if m else 0) for (b, e), m in zip(ranges, members)]
    sp = _stream_params(libflac, members[0].data, 0)
    plain = Batch(gpu, buf, table, sp)
    rb = RBatch(gpu, buf, table, sp)
    assert_plan(gpu, rb)
    assert np.array_equal(rb.cands["offset"].astype(np.int64), D.sync_pairs(buf))
    for off, cls in loose:  # in a gap: a candidate that belongs to no stream
        valid, k = _flag_of(rb.cands, off)
        assert valid == 0 and rb.cands["stream"][k] == -1 and rb.cands["succ"][k] == -1
    for s, m in enumerate(members):
        for d in (m.decoys if m else []):
            valid, k = _flag_of(rb.cands, ranges[s][0] + d.offset)
            assert valid == int(d.valid) and rb.cands["stream"][k] == s, (m.name, d.cls)
    want_n = [len(m.frame_offsets) if m else 0 for m in members]
    assert np.diff(plain.sf).tolist() == want_n and plain.status[0] == 0
    assert rb.rec.tobytes() == plain.rec.tobytes() and np.array_equal(rb.sf, plain.sf)
    assert np.array_equal(rb.ss, plain.ss.astype(np.int64)) and not rb.rs["flags"].any() and rb.status[0] == 0
    for s, m in enumerate(members):
        if m:
            sl = plain.stream(s)
            assert [int(x) - ranges[s][0] for x in plain.offs[sl]] == m.frame_offsets, m.name
            assert [int(x) - int(plain.ss[s]) for x in plain.os[sl]] == _expected(m)[1], m.name
    pcm, rec = rb.decode(gpu)
    assert (rec["status"] == 0).all() and (rec["crc_ok"] == 1).all()
    assert np.array_equal(pcm, np.concatenate([_truth_pcm(m) for m in members if m]))


@pytest.mark.parametrize("index", [1023, 1024])
def test_decoy_on_a_scan_seam(gpu, index):
    """The tuned decoy is candidate 1,023 / 1,024 of the buffer, where one workgroup's part of the
    1,024-wide key scan ends and the next begins; a second stream follows."""
    torch, libflac, dec = gpu
    r, other = D.row(f"S16/seam_{index}"), D.row("S16/valid_ch0")
    buf = r.data + b"\xf8\xff\xf8" + other.data
    ranges = [(0, len(r.data)), (len(r.data) + 3, len(buf))]
    table = [(b, e, b + m.first, m.total) for (b, e), m in zip(ranges, (r, other))]
    sp = _stream_params(libflac, r.data, 0)
    plain = Batch(gpu, buf, table, sp)
    rb = RBatch(gpu, buf, table, sp)
    assert_plan(gpu, rb)
    valid, k = _flag_of(rb.cands, r.decoys[0].offset)
    assert (valid, k) == (1, index) and rb.status[1] > 1024
    assert np.diff(plain.sf).tolist() == [3, 4] and rb.rec.tobytes() == plain.rec.tobytes()
    assert [int(x) for x in plain.offs] == r.frame_offsets + [o + ranges[1][0] for o in other.frame_offsets]
    assert not rb.rs["flags"].any() and rb.status[0] == 0
    pcm, rec = rb.decode(gpu)
    assert (rec["crc_ok"] == 1).all() and np.array_equal(pcm, np.concatenate([_truth_pcm(r), _truth_pcm(other)]))


def test_a_splice_keeps_its_links(gpu):
    """Frames numbered 0..4, then 0..2: libFLAC does not compare the numbers and decodes all eight
    (the oracle, below), so a number that does not continue must not cost a link when nothing else
    closes.  This is the other side of the number test that settles nested-n."""
    import random
    from tests.flac_frames import frame_pcm, stream
    torch, libflac, dec = gpu
    rng = random.Random(5)
    fr = [D.carrier_frame(rng, "S16", n)[:2] for n in (0, 1, 2, 3, 4, 0, 1, 2)]
    pcm = [frame_pcm(s, 256, 16) for _, s in fr]
    data = stream([f for f, _ in fr], pcm, channels=2, bps=16)
    offs = [42 + sum(len(f) for f, _ in fr[:k]) for k in range(8)]
    got, errors = oracle_frames(data)
    assert errors == 0 and [p for _, _, p in got] == pcm  # eight writes, each at its header's number
    sp = _stream_params(libflac, data)
    o, os_, info, nf = dec.index_stream(_upload(torch, data), len(data), 42, sp, 64)
    assert nf == 8 and o[:nf].cpu().numpy().tolist() == offs
    assert os_[:nf].cpu().numpy().tolist() == [256 * k for k in range(8)]
    b = Batch(gpu, data, [(0, len(data), 42, 8 * 256)], _stream_params(libflac, data, 0))
    assert np.diff(b.sf).tolist() == [8] and b.offs.tolist() == offs and b.status[0] == 0


# ------------------------------------------------------------------ 6. the reader and the stream API
READER_REFUSES = set(LIMIT)  # rows at a stated limit: open refuses (module docstring)


@pytest.mark.parametrize("name", NAMES)
def test_reader_matches_flacdecoder(gpu, name):
    """libflac.Reader in OUT_FLACDECODER with a window of 2 frames: the bytes of
    oracle.flacdecoder_copyto, or a refusal with a reason where the oracle refuses or the row is at
    a stated limit."""
    import oracle
    torch, libflac, dec = gpu
    r = D.row(name)
    rc, want, msg, fmt = oracle.flacdecoder_copyto(r.data)
    try:
        rd = libflac.Reader(r.data, libflac.OUT_FLACDECODER, window_frames=2)
    except RuntimeError as e:
        assert str(e)
        assert rc != 0 or name in READER_REFUSES, "refused a stream that FLACDecoder reads"
        return
    try:
        got = rd.read_all(16384)
    finally:
        rd.close()
    assert name not in READER_REFUSES
    assert rc == 0 and got == want


@pytest.mark.parametrize("name", NAMES)
def test_stream_api_matches_oracle(gpu, name):
    """FLAC__stream_decoder_* over the whole stream: the oracle's events and PCM.  It decodes frame
    after frame, as libFLAC does, so it has no limit rows."""
    import oracle
    from birdnest.audio_amd import harness
    r = D.row(name)
    ev, pcm = harness.run(r.data)
    oev, opcm = oracle.run(r.data)
    assert ev == harness.oracle_events_as_tuples(oev)
    assert np.array_equal(pcm, opcm)
    writes = [(e[8], e[3]) for e in ev if e[0] == harness.EV_WRITE]  # (sample number, blocksize)
    want = [(n, bs) for n, bs, _ in truth(r)]
    if r.kind == "tail-total0":  # host-certified: the lost sync, then the frame in the junk as well
        want.append((4 * r.blocksize, D.NESTED_BS))
    assert writes == want and sum(e[0] == harness.EV_ERROR for e in ev) == (r.kind == "tail-total0")
