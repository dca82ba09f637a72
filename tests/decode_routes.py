"""Batches, primers and the decode helper of tests/test_gpu_decode_routes.py (the builders run
without a GPU: tests/test_decode_routes_host.py).

bnf_launch_decode chooses its kernels and streams from the class counts the previous decode on
the device left in host memory (the "history": W16 frames, W32 frames, all frames, class-1 frames
of that decode order), bnf_launch_parse its CRC-16 hand-off mode.  A *primer* is a small batch
whose decode, followed by a synchronize, leaves a known history; a *batch* is what is decoded
under it.  Every expectation is exact and comes from the generator's source PCM
(synth.encode(...).pcm), which does not depend on the decoder:

    a frame of the table that decodes      its source samples at its output position
    a frame whose CRC-16 fails, or whose   zeros (include/bnflac.h: libFLAC writes a CRC-failed
    subframes fail or are cut short        frame as zeros; an ERROR / TRUNC frame with a parsed
                                           header is zero-filled)
    a frame whose header fails             nothing is written: the fill byte stays
    samples no frame of the table covers   the fill byte stays
"""
import numpy as np

from birdnest.audio_amd import libflac, synth
from tests.test_gpu_decode_classes import _mixed_batch, _plain_c2

FILL = 0xAB
DEC_LANES = 64   # csrc/bnf_residual.h: lanes of a decode workgroup, one subframe each
STRIDE_WGS = 512  # bnf_launch_decode_seg / bnf_launch_decode_list: at most this many workgroups stride over the blocks
FL_W32, FL_ST, FL_REDO, FL_W16, FL_WAVE_REDO = 16, 32, 64, 128, 512  # csrc/bnflac_device.h
OUTCOME_BITS = 6  # include/bnflac.h: flags bits 1 and 2 are the outcome; every other bit records the path
BS = 4096         # blocksize of every fixed-blocksize batch here
ABLATES = (0, 0x400, 0x100000)  # none; k_decode_st off, all stereo to k_decode<8>; k_decode<8> as one launch
FORMATS = ("OUT_INTERLEAVED32", "OUT_FLACDECODER")


def lanes_for(channels):
    """bnflac_runtime.cpp: lanes of a frame's lane group"""
    l = 1
    while l < channels:
        l <<= 1
    return min(l, 8)


def fpb(channels):
    """frames per decode block"""
    return DEC_LANES // lanes_for(channels)


class Batch:
    """One decode call's input and its exact output.

    offs / osmp: the frame table (osmp None: frames at their header's sample numbers);
    pcm: int32 [total, channels], the source; nbytes: what the call is told the buffer holds;
    zero / keep: (first sample, samples) ranges that come out as zeros / keep the fill byte;
    damaged: table indices of the frames the builder damaged."""

    def __init__(self, name, data, offs, osmp, pcm, total, sp=None, nbytes=None, zero=(), keep=(), damaged=()):
        self.name, self.data = name, bytes(data)
        self.offs = np.ascontiguousarray(offs, dtype=np.int64)
        self.osmp = None if osmp is None else np.ascontiguousarray(osmp, dtype=np.int64)
        self.pcm, self.total = pcm, int(total)
        self.channels = int(pcm.shape[1])
        self.sp = sp if sp is not None else libflac.StreamParams(1, BS, BS, 44100, self.channels, 16, self.total)
        self.nbytes = len(self.data) if nbytes is None else int(nbytes)
        self.zero, self.keep, self.damaged = tuple(zero), tuple(keep), tuple(damaged)
        assert pcm.shape[0] == self.total and len(self.offs) > 0
        assert self.osmp is None or len(self.osmp) == len(self.offs)

    @property
    def nframes(self):
        return len(self.offs)

    def expected(self, fmt_name):
        """the whole output buffer, bytes (uint8 array)"""
        if fmt_name == "OUT_INTERLEAVED32":
            out = np.ascontiguousarray(self.pcm.astype("<i4")).view(np.uint8).reshape(self.total, -1).copy()
        else:  # FLACDecoder.WriteCallback: 16-bit stereo as int16 pairs
            assert self.channels == 2 and fmt_name == "OUT_FLACDECODER"
            out = np.ascontiguousarray((self.pcm.astype(np.int64) & 0xFFFF).astype("<u2")).view(np.uint8).reshape(self.total, -1).copy()
        for s, n in self.zero:
            out[s:s + n] = 0
        for s, n in self.keep:
            out[s:s + n] = FILL
        return out.reshape(-1)


def concat(parts):
    """_mixed_batch's layout for any fixed-blocksize parts: the streams' bytes one after the other,
    every frame at its own place in one output, the table part by part"""
    data, offs, osmp, pcm = bytearray(), [], [], []
    base = 0
    for s in parts:
        bs = s.params.blocksize
        assert s.nsamples == bs * len(s.frame_offsets)
        offs.append(s.frame_offsets.astype(np.int64) + len(data))
        osmp.append(base + np.arange(len(s.frame_offsets), dtype=np.int64) * bs)
        pcm.append(s.pcm)
        data += s.data.tobytes()
        base += s.nsamples
    return bytes(data), np.concatenate(offs), np.concatenate(osmp), np.concatenate(pcm), base


def _c2(nframes, **kw):
    return synth.encode(synth.config("C2", nframes=nframes, **kw))


def _wide_parts(n12, n32, blocksize=BS, channels=2):
    return [_c2(n12, order=12, seed=42, blocksize=blocksize, channels=channels),
            _c2(n32, order=32, partition_order=-1, seed=43, blocksize=blocksize, channels=channels)]


def _class1_parts(n):
    """narrow frames k_decode_st cannot take (VERBATIM / CONSTANT subframes): decode class 1 only"""
    return [_c2(n, subframe_mode=synth.SUB_VERBATIM, seed=46), _c2(n, subframe_mode=synth.SUB_CONSTANT, seed=47)]


# ------------------------------------------------------------------ primers
# name -> what the decode after it must report: seg_only, the split armed (class-1 count != 0 with
# the side grids), the hand-off mode of a 16-bit parse under the default crc_mode, and the history
# words where the content fixes them (None: taken from the primer's own records)
PRIMERS = {
    "none": dict(seg_only=True, split=False, cm=1, hist=(0, 0, 8, 0)),
    "class1": dict(seg_only=True, split=False, cm=1, hist=(0, 0, 8, 8)),
    "wide": dict(seg_only=False, split=False, cm=0, hist=(4, 4, 8, 0)),
    "wide_few": dict(seg_only=False, split=False, cm=1, hist=(1, 1, 32, 0)),
    "all": dict(seg_only=False, split=True, cm=0, hist=None),  # over a quarter of its frames are W16 / W32
}
UNKNOWN = dict(seg_only=False, split=True, cm=1, hist=(0xFFFFFFFF,) * 4)  # a fresh process


def primer(name):
    if name == "none":
        return Batch(name, *_plain_c2(8))
    if name == "class1":
        # the decode classes of a SUB_MIXED batch include W16 / W32 (its LPC orders go to 32), which
        # would arm the side grids like `all`; VERBATIM / CONSTANT frames alone leave W16 = W32 = 0
        # with class 1 recorded
        return Batch(name, *concat(_class1_parts(4)))
    if name == "wide":
        return Batch(name, *concat(_wide_parts(4, 4)))
    if name == "wide_few":
        return Batch(name, *concat([_c2(30, seed=44)] + _wide_parts(1, 1)))
    if name == "all":
        return Batch(name, *_mixed_batch(13, class1=True))
    raise KeyError(name)


def history_of(info):
    """the four words k_order_scan leaves after a decode with these records (order_key's classes)"""
    fl, ok = info["flags"], info["status"] == 0
    w32 = ok & ((fl & FL_W32) != 0)
    w16 = ok & ~w32 & ((fl & FL_W16) != 0)
    st = ok & ~w32 & ~w16 & ((fl & FL_ST) != 0)
    return int(w16.sum()), int(w32.sum()), len(info), int(len(info) - w16.sum() - w32.sum() - st.sum())


# ------------------------------------------------------------------ batches under test
def _damaged():
    """a mixed batch with one frame of each kind of damage.  _mixed_batch's table holds frame i
    of each part in turn: parts 0 hand-back stereo, 1 order 12 (W16), 2 order 32, 3 plain stereo,
    4 SUB_MIXED, so (part p, frame i) is entry 5 i + p."""
    n = 6
    data, offs, osmp, pcm, total = _mixed_batch(n, class1=True)
    data = bytearray(data)
    assert len(offs) == 5 * n
    ends = np.sort(np.concatenate([offs, [len(data)]]))

    def length(k):
        return int(ends[np.searchsorted(ends, offs[k]) + 1] - offs[k])

    hdr, st, w16, cut = 5 * 1 + 3, 5 * 2 + 3, 5 * 2 + 1, 5 * (n - 1) + 4
    data[offs[hdr] + 2] ^= 0x10           # blocksize code: the header's CRC-8 fails, nothing is written
    data[offs[st] + length(st) // 2] ^= 0x01   # a residual byte of a stereo fast-path frame
    data[offs[w16] + length(w16) // 2] ^= 0x01  # ... and of a W16 frame
    assert offs[cut] == offs.max()        # the last frame of the buffer: cut short by nbytes,
    nbytes = len(data) - 3                # by its CRC-16 and the last byte of its last subframe
    return Batch("damaged", data, offs, osmp, pcm, total, nbytes=nbytes,
                 zero=[(int(osmp[k]), BS) for k in (st, w16, cut)], keep=[(int(osmp[hdr]), BS)],
                 damaged=(hdr, st, w16, cut))


def _first(name, k):
    """the first k table entries of a 35-frame mixed batch: the other frames' samples keep the fill"""
    data, offs, osmp, pcm, total = _mixed_batch(7, class1=True)
    return Batch(name, data, offs[:k], osmp[:k], pcm, total, keep=[(int(o), BS) for o in osmp[k:]])


def _c4_700():
    """BASELINE C4's shape (variable blocksize, every decode class).  About one frame in six of
    this mix is a stereo fast-path frame (300 frames hold 52), and class 0 has to span several whole
    blocks beyond the one that straddles classes 0 and 1: 700 frames give more than 3 * fpb of them,
    which the GPU module asserts from the records."""
    p = synth.config("C4", nframes=700, last_blocksize=0)
    s = synth.encode(p)
    return Batch("c4_700", s.data.tobytes(), s.frame_offsets.astype(np.int64), None, s.pcm, s.nsamples,
                 sp=libflac.StreamParams.from_synth(p, s.nsamples))


BATCHES = {
    "plain16": lambda: Batch("plain16", *_plain_c2(16)),
    "handback": lambda: Batch("handback", *concat([_c2(16, stereo_mode=3, level=0.9, noise=0.5, seed=41)])),
    "wide": lambda: Batch("wide", *concat(_wide_parts(9, 8))),
    "class1": lambda: Batch("class1", *concat(_class1_parts(6))),
    "mixed65": lambda: Batch("mixed65", *_mixed_batch(13, class1=True)),
    "c4_700": _c4_700,
    "one": lambda: Batch("one", *_plain_c2(1)),
    "fpb": lambda: _first("fpb", fpb(2)),
    "fpb_plus_1": lambda: _first("fpb_plus_1", fpb(2) + 1),
    "damaged": _damaged,
}
_cache = {}


def batch(name):
    """a batch under test or (as "primer:<name>") a primer, encoded once per process"""
    if name not in _cache:
        _cache[name] = primer(name[7:]) if name.startswith("primer:") else BATCHES[name]()
    return _cache[name]


# ------------------------------------------------------------------ the second trip of the stride loops
def stride_trip_frames(channels):
    """more than STRIDE_WGS * fpb frames by two whole blocks and a partial one: the strided
    workgroups 0 and 1 take a second block and workgroup 2 a partial one"""
    return STRIDE_WGS * fpb(channels) + 2 * fpb(channels) + 3


def seg_trip_batch(channels, blocksize=256, lead=5):
    """k_decode_seg's second trip: 4 order-12 and 4 order-32 frames named over and over, each
    time at another output position, behind `lead` narrow frames (decode classes 0 / 1, which the
    order puts first: the segment then starts inside a block).  -> (Batch, nwide, lead)"""
    wide = _wide_parts(4, 4, blocksize, channels)
    plain = _c2(lead, seed=44, blocksize=blocksize, channels=channels)
    data, offs, _, pcm, _ = concat(wide + [plain])
    nwide = stride_trip_frames(channels)
    table = np.concatenate([np.arange(nwide) % 8, 8 + np.arange(lead)])  # the narrow frames last in the table
    total = len(table) * blocksize
    sp = libflac.StreamParams(1, blocksize, blocksize, 44100, channels, 16, total)
    src = pcm.reshape(8 + lead, blocksize, channels)[table].reshape(total, channels)
    b = Batch(f"seg_trip_{channels}ch", data, offs[table], np.arange(len(table), dtype=np.int64) * blocksize, src, total, sp=sp)
    return b, nwide, lead


def list_trip_table(nhand):
    """k_decode_list's second trip: the table's even entries name the handed-back frame, the odd
    ones cycle through the frames that are not -> (is_hand bool[2 nhand])"""
    is_hand = np.zeros(2 * nhand, dtype=bool)
    is_hand[0::2] = True
    return is_hand


# ------------------------------------------------------------------ decoding (GPU)
class Device:
    """uploads of the batches (once each) and the decode call"""

    def __init__(self):
        import torch
        self.torch, self.dev = torch, torch.device("cuda:0")
        self.L = libflac.load()
        self.dec = libflac.BatchDecoder(0)
        self._up, self._exp = {}, {}

    def upload(self, b):
        if id(b) not in self._up:
            t = self.torch
            n = len(b.data)
            d_bytes = t.zeros((n + 15) // 16 * 16 + 64, dtype=t.uint8, device=self.dev)
            d_bytes[:n] = t.frombuffer(bytearray(b.data), dtype=t.uint8).to(self.dev)
            d_os = t.from_numpy(b.osmp).to(self.dev) if b.osmp is not None else None
            self._up[id(b)] = (b, d_bytes, t.from_numpy(b.offs).to(self.dev), d_os)
        return self._up[id(b)][1:]

    def expected(self, b, fmt_name):
        k = (id(b), fmt_name)
        if k not in self._exp:
            self._exp[k] = (b, self.torch.from_numpy(b.expected(fmt_name)).to(self.dev))
        return self._exp[k][1]

    def enqueue(self, b, fmt_name="OUT_INTERLEAVED32"):
        """parse + decode into a fresh output filled with FILL; no synchronize -> (d_out, d_info)"""
        t = self.torch
        d_bytes, d_offs, d_os = self.upload(b)
        fmt = getattr(libflac, fmt_name)
        d_out = t.full((b.total * libflac.out_stride(fmt, b.sp),), FILL, dtype=t.uint8, device=self.dev)
        d_info = t.zeros(b.nframes * libflac.FRAME_INFO_BYTES, dtype=t.uint8, device=self.dev)
        self.dec.decode_frames(d_bytes, b.nbytes, d_offs, b.nframes, b.sp, fmt, d_out, d_info, d_out_sample=d_os)
        return d_out, d_info

    def decode(self, b, fmt_name="OUT_INTERLEAVED32"):
        """-> (d_out on the device, records on the host), synchronized"""
        d_out, d_info = self.enqueue(b, fmt_name)
        self.torch.cuda.synchronize()
        return d_out, libflac.info_array(d_info.cpu().numpy())

    def prime(self, name):
        """decode primer `name` with the lane kernels and synchronize -> the history it leaves"""
        b = batch("primer:" + name)
        d_out, info = self.decode(b)
        assert self.torch.equal(d_out, self.expected(b, "OUT_INTERLEAVED32")), f"primer {name}: wrong PCM"
        assert (info["status"] == 0).all() and (info["crc_ok"] == 1).all(), f"primer {name}"
        h = history_of(info)
        want = PRIMERS[name]
        assert want["hist"] is None or h == want["hist"], (name, h)
        assert (h[0] == 0 and h[1] == 0) == want["seg_only"] and (h[3] != 0 and not want["seg_only"]) == want["split"], (name, h)
        assert (4 * (h[0] + h[1]) >= h[2]) == (want["cm"] == 0), (name, h)
        return h


def records_differ(a, b):
    """the fields in which two routes' records differ; the path bits of flags are not compared"""
    bad = [n for n in a.dtype.names if n != "flags" and not np.array_equal(a[n], b[n])]
    if not np.array_equal(a["flags"] & OUTCOME_BITS, b["flags"] & OUTCOME_BITS):
        bad.append("flags & 6")
    return bad


def first_difference(d_out, d_exp):
    """where and how an output differs, for the assertion message"""
    ne = (d_out != d_exp).nonzero().flatten()
    if ne.numel() == 0:
        return ""
    i = int(ne[0])
    got = d_out[i:i + 8].cpu().numpy().tolist()
    return f"{int(ne.numel())} bytes differ, first at byte {i}: got {got}, expected {d_exp[i:i + 8].cpu().numpy().tolist()}"


def check_route(r, want, hist, ablate, before):
    """the route the decode reported (libflac.last_route) against the primed state; the split bit
    is checked by check_split after the comparisons"""
    assert r["ndecode"] == before["ndecode"] + 1 and r["nparse"] == before["nparse"] + 1, (r, before)
    assert not r["sys"] and not r["sw"] and not r["parse_wave"], r
    assert r["hist_read"] and r["hist"] == tuple(hist), (r, hist)
    assert r["seg_only"] == want["seg_only"], r
    if not want["seg_only"]:
        assert r["fork_before"] or r["fork_after"], r
    assert r["parse_hist_read"] and r["parse_hist"] == tuple(hist[:3]) and r["cm"] == want["cm"], r


def check_split(r, want, ablate):
    assert r["w8split"] == (want["split"] and ablate == 0), (r, hex(ablate))
