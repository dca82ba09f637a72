"""Every route of the decode launch, pinned (bnf_launch_decode, bnf_launch_parse).

A decode does not run one way: from the class counts the previous decode on the device left in
host memory it chooses the side grids or k_decode_seg, one k_decode<8> launch or two, and (in the
parse) whether the CRC-16 hand-off is produced.  A wrong guess may only cost time.  Here each
history state (a primer decode, then a synchronize; tests/decode_routes.py) is crossed with each
batch composition, both layouts with their own k_decode_st translation unit, and the ablation
words that reroute frames: the PCM must be the generator's source PCM, the records those of the
k_decode_sys route outside the path bits of `flags`, and bnflac_debug_last_route must report the
route the primer arms -- a cell that does not reach its route fails.

Outputs are filled with 0xAB before every decode, so a frame no kernel took cannot pass.
The last two tests take k_decode_seg and k_decode_list through a second trip of their
grid-stride loops, which needs more than 512 * fpb frames: the frame table names a few encoded
frames again and again at different output positions."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import gpu_available

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_MIXED_TYPES = ("mixed65", "c4_700")  # the batches the fresh-process primer runs on


@pytest.fixture(scope="module")
def gpu():
    if not gpu_available():
        pytest.skip("no GPU")
    from tests import decode_routes as R
    return R.Device()


@pytest.fixture(autouse=True)
def _switches():
    """the lane kernels and k_parse (the kernel that hands over) for every test; restored after it"""
    if not gpu_available():
        yield
        return
    from birdnest.audio_amd import libflac
    L = libflac.load()
    L.bnflac_debug_set_decode_sys(0)
    L.bnflac_debug_set_parse_wave(0)
    L.bnflac_debug_set_crc_mode(-1)
    L.bnflac_debug_set_ablate(0)
    try:
        yield
    finally:
        L.bnflac_debug_set_decode_sys(-1)
        L.bnflac_debug_set_parse_wave(-1)
        L.bnflac_debug_set_crc_mode(-1)
        L.bnflac_debug_set_ablate(0)


_refs = {}


def _reference(gpu, b, fmt):
    """the records of the k_decode_sys route (its PCM checked on the way), once per batch and layout"""
    from birdnest.audio_amd import libflac
    from tests import decode_routes as R
    if (b.name, fmt) not in _refs:
        gpu.L.bnflac_debug_set_decode_sys(1)
        try:
            d_out, info = gpu.decode(b, fmt)
        finally:
            gpu.L.bnflac_debug_set_decode_sys(0)
        assert libflac.last_route()["sys"]
        exp = gpu.expected(b, fmt)
        assert gpu.torch.equal(d_out, exp), f"k_decode_sys route, {b.name}/{fmt}: {R.first_difference(d_out, exp)}"
        good = np.ones(b.nframes, dtype=bool)
        good[list(b.damaged)] = False
        assert (info["status"][good] == 0).all() and (info["crc_ok"][good] == 1).all(), b.name
        for k in b.damaged:  # the damage took: the frame is not delivered
            assert info["status"][k] != 0 or info["crc_ok"][k] == 0, (b.name, k, info[k])
        if b.name == "damaged":
            hdr, st, w16, cut = b.damaged
            assert info["status"][hdr] != 0 and info["sub_start"][hdr][0] == 0, info[hdr]  # no range: nothing written
            assert info["status"][cut] == 2 and info["sub_start"][cut][0] != 0, info[cut]   # truncated inside a subframe
            assert info["flags"][st] & R.FL_ST and info["flags"][w16] & R.FL_W16, (info["flags"][st], info["flags"][w16])
        if b.name == "c4_700":  # class 0 spans whole blocks beyond the one that straddles classes 0 and 1
            assert ((info["flags"] & R.FL_ST) != 0).sum() > 3 * R.fpb(2), info["flags"]
        _refs[(b.name, fmt)] = info
    return _refs[(b.name, fmt)]


def _check_cell(gpu, cell, b, fmt, ab, want, hist, before, r, d_out, info):
    from tests import decode_routes as R
    R.check_route(r, want, hist, ab, before)
    exp = gpu.expected(b, fmt)
    assert gpu.torch.equal(d_out, exp), f"{cell}: {R.first_difference(d_out, exp)}"
    bad = R.records_differ(info, _reference(gpu, b, fmt))
    assert not bad, f"{cell}: records differ from the k_decode_sys route in {bad}"
    R.check_split(r, want, ab)
    if b.name == "handback" and not ab & 0x400:
        assert (info["flags"] & R.FL_REDO).any(), f"{cell}: the batch should hold handed-back stereo frames"


@pytest.mark.parametrize("bname", ["plain16", "handback", "wide", "class1", "mixed65", "c4_700", "one", "fpb",
                                   "fpb_plus_1", "damaged"])
@pytest.mark.parametrize("pname", ["none", "class1", "wide", "wide_few", "all"])
def test_route_matrix(gpu, pname, bname):
    """primer x batch, and inside: layout x ablation word"""
    from birdnest.audio_amd import libflac
    from tests import decode_routes as R
    b, want = R.batch(bname), R.PRIMERS[pname]
    for fmt in R.FORMATS:
        _reference(gpu, b, fmt)
        for ab in R.ABLATES:
            hist = gpu.prime(pname)
            before = libflac.last_route()
            gpu.L.bnflac_debug_set_ablate(ab)
            try:
                d_out, info = gpu.decode(b, fmt)
            finally:
                gpu.L.bnflac_debug_set_ablate(0)
            _check_cell(gpu, f"{pname}/{bname}/{fmt}/{ab:#x}", b, fmt, ab, want, hist, before, libflac.last_route(), d_out, info)


_UNKNOWN_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import torch
from birdnest.audio_amd import libflac
from tests import decode_routes as R
bname, fmt, ab = sys.argv[2], sys.argv[3], int(sys.argv[4], 0)
g = R.Device()
g.L.bnflac_debug_set_decode_sys(0)
g.L.bnflac_debug_set_parse_wave(0)
g.L.bnflac_debug_set_ablate(ab)
b = R.batch(bname)
exp = g.expected(b, fmt)
before = libflac.last_route()
d_out, info = g.decode(b, fmt)  # the first decode of the process
res = {"before": before, "route": libflac.last_route(), "pcm_ok": bool(torch.equal(d_out, exp)),
       "diff": R.first_difference(d_out, exp)}
sys.stdout.buffer.write(json.dumps(res).encode() + b"\n" + info.tobytes())
"""


@pytest.mark.parametrize("fmt", ["OUT_INTERLEAVED32", "OUT_FLACDECODER"])
@pytest.mark.parametrize("bname", _MIXED_TYPES)
@pytest.mark.parametrize("ab", [0, 0x400, 0x100000])
def test_route_unknown_history(gpu, ab, bname, fmt):
    """Before the first decode on a device all four history words are ~0u: side grids, the split
    armed, the hand-off kept.  Only a process's first decode runs in that state, so each cell is
    the one decode of a fresh child process (one child at a time)."""
    from birdnest.audio_amd import libflac
    from tests import decode_routes as R
    b = R.batch(bname)
    ref = _reference(gpu, b, fmt)
    p = subprocess.run([sys.executable, "-c", _UNKNOWN_CHILD, ROOT, bname, fmt, hex(ab)], capture_output=True, timeout=100)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    head, _, raw = p.stdout.partition(b"\n")
    res = json.loads(head)
    info = libflac.info_array(np.frombuffer(raw, dtype=np.uint8))
    r = {k: tuple(v) if isinstance(v, list) else v for k, v in res["route"].items()}
    cell = f"unknown/{bname}/{fmt}/{ab:#x}"
    assert res["before"]["ndecode"] == 0 and res["before"]["nparse"] == 0, res["before"]
    R.check_route(r, R.UNKNOWN, R.UNKNOWN["hist"], ab, res["before"])
    assert res["pcm_ok"], f"{cell}: {res['diff']}"
    bad = R.records_differ(info, ref)
    assert not bad, f"{cell}: records differ from the k_decode_sys route in {bad}"
    R.check_split(r, R.UNKNOWN, ab)


def test_asynchronous_history(gpu):
    """Three decodes enqueued back to back: which history the second and third read is not
    defined (the first one's k_order_scan may or may not have run), all three must be right."""
    from tests import decode_routes as R
    gpu.prime("none")
    bs = [R.batch("mixed65"), R.batch("plain16"), R.batch("mixed65")]
    for b in bs:  # uploads and expectations first: nothing but the decodes between the enqueues
        gpu.upload(b)
        gpu.expected(b, "OUT_INTERLEAVED32")
    gpu.torch.cuda.synchronize()
    outs = [gpu.enqueue(b) for b in bs]
    gpu.torch.cuda.synchronize()
    for i, (b, (d_out, d_info)) in enumerate(zip(bs, outs)):
        from birdnest.audio_amd import libflac
        exp = gpu.expected(b, "OUT_INTERLEAVED32")
        assert gpu.torch.equal(d_out, exp), f"decode {i} ({b.name}): {R.first_difference(d_out, exp)}"
        info = libflac.info_array(d_info.cpu().numpy())
        assert (info["status"] == 0).all() and (info["crc_ok"] == 1).all(), (i, b.name)


@pytest.mark.parametrize("fmt", ["OUT_INTERLEAVED32", "OUT_FLACDECODER"])
def test_handoff_dropped_by_history(gpu, fmt):
    """After a decode with a quarter or more W16 / W32 frames the next 16-bit parse produces no
    CRC-16 hand-off (cm 0) and k_decode_st checks every frame itself; after one with few it
    hands the prefix over (cm 1).  Same verdicts, same PCM: one frame's CRC-16 fails."""
    from birdnest.audio_amd import libflac
    from tests import decode_routes as R
    from tests.test_gpu_decode_classes import _plain_c2
    data, offs, osmp, pcm, total = _plain_c2(16)
    data = bytearray(data)
    data[int(offs[5]) + (int(offs[6]) - int(offs[5])) // 2] ^= 0x01
    b = R.Batch("plain_crc", data, offs, osmp, pcm, total, zero=[(5 * R.BS, R.BS)], damaged=(5,))
    exp = gpu.expected(b, fmt)
    got = {}
    for pname, cm in (("wide", 0), ("wide_few", 1)):
        hist = gpu.prime(pname)
        d_out, info = gpu.decode(b, fmt)
        r = libflac.last_route()
        assert r["parse_hist_read"] and r["parse_hist"] == hist[:3] and not r["parse_wave"], r
        assert r["cm"] == cm, (pname, r)
        assert (info["flags"] & R.FL_ST).all() and (info["status"] == 0).all(), info["flags"]
        assert info["crc_ok"].tolist() == [1] * 5 + [0] + [1] * 10, (pname, info["crc_ok"])
        assert gpu.torch.equal(d_out, exp), f"after {pname}: {R.first_difference(d_out, exp)}"
        got[pname] = info
    assert not R.records_differ(got["wide"], got["wide_few"])


def _same_as_first(torch, rows, period):
    """rows [n, w]: row i equals row i % period"""
    n = rows.shape[0]
    full = n // period * period
    v = rows[:full].view(-1, period, rows.shape[1])
    return torch.equal(v[1:], v[:1].expand_as(v[1:])) and torch.equal(rows[full:], rows[:n - full])


@pytest.mark.parametrize("channels", [2, 8])
def test_seg_grid_second_trip(gpu, channels):
    """k_decode_seg strides at most 512 workgroups over the W16 + W32 segment of the decode order
    (bnf_launch_decode_seg), fpb = 64 / lanes_for(channels) frames a block: 32 for stereo, 8 for 8
    channels.  512 * fpb + 2 * fpb + 3 wide frames give workgroups 0 and 1 a second whole block
    and workgroup 2 a partial one, each reusing its LDS ring and row buffer; 5 narrow frames in
    front put the segment's first frame inside a block.  Every repeat of a frame must equal its
    first copy, and that the source PCM."""
    from birdnest.audio_amd import libflac
    from tests import decode_routes as R
    torch = gpu.torch
    b, nwide, lead = R.seg_trip_batch(channels)
    f = R.fpb(channels)
    assert nwide >= R.STRIDE_WGS * f + 2 * f and lead % f != 0
    hist = gpu.prime("none")
    d_out, info = gpu.decode(b)
    r = libflac.last_route()
    assert r["seg_only"] and r["hist"] == hist and not r["sys"], r
    assert (info["status"] == 0).all() and (info["crc_ok"] == 1).all()
    wide = (info["flags"] & (R.FL_W16 | R.FL_W32)) != 0
    assert wide[:nwide].all() and not wide[nwide:].any(), "the table's wide frames first, the narrow ones last"
    bs = b.sp.max_blocksize
    rows = d_out.view(torch.int32).view(b.nframes, bs * channels)
    src = torch.from_numpy(np.ascontiguousarray(b.pcm[:8 * bs])).to(rows.device).view(8, bs * channels)
    assert torch.equal(rows[:8], src), "the first copy of the wide frames differs from the source PCM"
    assert _same_as_first(torch, rows[:nwide], 8), "a repeat of a wide frame differs from its first copy"
    tail = torch.from_numpy(np.ascontiguousarray(b.pcm[nwide * bs:])).to(rows.device).view(lead, bs * channels)
    assert torch.equal(rows[nwide:], tail), "the narrow frames differ from the source PCM"


LIST_HAND = "E/S16/wide_shift-16"  # tests/flac_frames.py: a 64-bit-path shift of 32 or more, which k_decode_sys hands back


def test_list_grid_second_trip(gpu):
    """k_decode_list strides at most 512 workgroups over k_decode_sys's hand-back list
    (bnf_launch_decode_list), 32 stereo frames a block.  One frame that k_decode_sys hands back is
    named 512 * 32 + 2 * 32 + 3 times, between four frames that it keeps: BNF_FL_WAVE_REDO on
    exactly its repeats, every repeat equal to the first copy, and that the reference PCM.

    No stream of the generator holds such a frame: test_mmx16_leaving_int16_handed_back's fixture
    (loud, weakly correlated stereo) has none handed back at blocksize 256 or 4096 under stereo
    modes 0, 1 and 3 (measured: no BNF_FL_WAVE_REDO in any of its 8 frames), and cannot: the
    generator clips its samples to 16 bits and an MMX16 subframe is one of at most 16 bits (the
    17-bit side channel takes the 32-bit path), so none leaves int16.  The frames
    here are hand-built ones (tests/flac_frames.py, 16-bit stereo, blocksize 64): the handed-back
    one is libFLAC-defined (its PCM is the CPU oracle's), the kept ones' PCM is the exact-integer
    reference of their writer."""
    from birdnest.audio_amd import libflac
    from tests import decode_routes as R
    from tests import flac_frames as F
    from tests.test_frame_fields_host import oracle_frame
    torch = gpu.torch
    rows = [r for r in F.rows() if (r.channels, r.bps, r.si) == (2, 16, True)]
    hand = next(r for r in rows if r.name == LIST_HAND)
    bs = hand.blocksize
    kept = [r for r in rows if r.sys_kept and r.expect == "restore" and r.blocksize == bs][:4]
    assert not hand.sys_kept and len(kept) == 4
    rc, _, hand_pcm = oracle_frame(hand)
    assert rc == 0
    frames = [hand] + kept
    data = b"".join(r.data for r in frames)
    offs = np.cumsum([0] + [len(r.data) for r in frames[:-1]]).astype(np.int64)
    pcm = np.stack([np.array(p, dtype=np.int64).T for p in [hand_pcm] + [r.pcm for r in kept]]).astype(np.int32)  # [5, bs, 2]
    nhand = R.stride_trip_frames(2)
    assert nhand > R.STRIDE_WGS * R.fpb(2) + 2 * R.fpb(2)
    is_hand = R.list_trip_table(nhand)
    table = np.where(is_hand, 0, 1 + (np.arange(2 * nhand) // 2) % 4)
    n = len(table)
    src = pcm[table].reshape(n * bs, 2)
    b = R.Batch("list_trip", data, offs[table], np.arange(n, dtype=np.int64) * bs, src, n * bs,
                sp=libflac.StreamParams(1, F.SI_BLOCKSIZE, F.SI_BLOCKSIZE, F.SI_RATE, 2, 16, 0))
    gpu.L.bnflac_debug_set_decode_sys(1)
    try:
        d_out, info = gpu.decode(b)
        assert libflac.last_route()["sys"]
    finally:
        gpu.L.bnflac_debug_set_decode_sys(0)
    assert (info["status"] == 0).all() and (info["crc_ok"] == 1).all()
    assert np.array_equal((info["flags"] & R.FL_WAVE_REDO) != 0, is_hand), "hand-backs: exactly the repeats of the hand-back frame"
    out = d_out.view(torch.int32).view(n, bs * 2)
    first = torch.from_numpy(np.ascontiguousarray(src[:8 * bs])).to(out.device).view(8, bs * 2)
    assert torch.equal(out[:8], first), "the first copies differ from the reference PCM"
    assert _same_as_first(torch, out, 8), "a repeat differs from its first copy"
