"""Where bnflac_decode_frames writes: frames, placement plans and the byte model shared by
tests/test_out_placement_host.py (no GPU) and tests/test_gpu_out_placement.py.

The decode kernels choose a frame's store path from the absolute address of its output range
(16-byte, 4-byte or byte stores; whole 64- and 128-byte lines where every run of a wave starts on
one), so what is pinned here is placement: frames of the blocksizes at which the chunk loops have
whole, ragged and single chunks, put at every reachable start residue with gaps between them,
inside an allocation whose every byte is compared.

Nothing here comes from the project: the frames are written by tests/flac_frames.py, their PCM is
frame_pcm() (RFC 9639 in unbounded integers), and the model of the output is the contract of
include/bnflac.h restated in Python integers:

    stride = the layout's bytes per sample, limit = out_bytes // stride
    a frame of blocksize b at position p is in range iff 0 <= p, p <= limit and b <= limit - p
    in range and decoded: its bytes at p * stride; in range, ERROR / TRUNC with its header parsed:
    zeros; out of range: nothing; every other byte of the allocation keeps the fill byte.
"""
import math
import random

import numpy as np

from tests import flac_frames as F

FILL = 0xAB
U64 = 1 << 64
SEED = 963917
B = (16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 95, 96, 97, 127, 128, 129, 159, 160, 161, 192)
COPIES = 8
CHUNK = {"k_decode_st": 32, "k_decode_sw": 16, "k_decode<8>": 32, "k_decode<16>": 32, "k_decode<32>": 32}
LAYOUT_CODE = {"OUT_PLANAR32": 0, "OUT_INTERLEAVED32": 1, "OUT_FLACDECODER": 2, "OUT_FILEREADER": 3}  # include/bnflac.h
ALL4 = ("OUT_INTERLEAVED32", "OUT_FLACDECODER", "OUT_FILEREADER", "OUT_PLANAR32")
WIDE3 = ("OUT_FILEREADER", "OUT_INTERLEAVED32", "OUT_PLANAR32")
LAYOUTS_OF = {"S16": ALL4, "S24": WIDE3, "M16": ALL4, "T24": WIDE3, "W32": ALL4}  # what a carrier's kernel writes
LEGS = [(c, l) for c in F.CARRIERS for l in LAYOUTS_OF[c]]
PLANS = ("line", "al16", "mixed")
HEADER_BASE = (1 << 36) - (1 << 20)  # base_sample of the header-number runs: the numbers take the 7-byte coding
SI_FIXED = 192                       # STREAMINFO min == max blocksize of the fixed-blocksize run
ASSIGNMENTS = (1, F.LEFT_SIDE, F.RIGHT_SIDE, F.MID_SIDE)  # by copy; 1: two independent channels


def blocksizes(carrier):
    return tuple(b for b in B if b >= 32) if carrier == "W32" else B


def stride_of(layout, channels, bps):
    """bnflac_out_stride, restated (the host test compares it with the library's)"""
    if layout in ("OUT_PLANAR32", "OUT_INTERLEAVED32"):
        return 4 * channels
    if layout == "OUT_FLACDECODER":
        return 4 if channels == 2 else 2
    return channels * (3 if bps == 24 else 2)


def line_of(carrier, layout):
    """M: the line that governs a leg's store paths"""
    channels, bps = F.CARRIERS[carrier][:2]
    if carrier == "S16" and layout in ("OUT_FLACDECODER", "OUT_FILEREADER"):
        return 128  # k_decode_st's flush line
    if carrier == "S24" and layout == "OUT_FILEREADER":
        return 64   # k_decode_sw's line
    return 16


# ------------------------------------------------------------------ the frames
class Frame:
    """One frame of a carrier: its subframes, exact PCM, and its bytes under any header numbering."""

    def __init__(self, carrier, blocksize, copy):
        self.carrier, self.blocksize, self.copy = carrier, blocksize, copy
        self.channels, self.bps, _, self.kernel = F.CARRIERS[carrier]
        rng = random.Random(f"{SEED}/{carrier}/{blocksize}/{copy}")
        subs = [F.lpc_sub(rng, 17, 12, 11)] if carrier == "W32" else F.default_subs(rng, carrier)
        cap = F.sample_cap(carrier)
        for s in subs:
            porder = 1 if blocksize % 2 == 0 and (blocksize >> 1) > s["order"] else 0
            F._from_signal(rng, s, F._signal(rng, blocksize, 1 << (cap - 3), 40), blocksize, porder)
        self.subs = subs
        self.assignment = ASSIGNMENTS[copy % 4] if self.channels == 2 else self.channels - 1
        self.samples = []  # per channel, the subframes' samples (what st_keeps / sys_keeps judge)
        self.pcm = F.frame_pcm(subs, blocksize, self.bps, self.assignment, self.samples)
        self._bytes = {}

    def data(self, number=0, variable=False):
        key = (number, variable)
        if key not in self._bytes:
            self._bytes[key] = F.frame(self.subs, self.blocksize, self.bps, number=number, variable=variable,
                                       assignment=self.assignment)
        return self._bytes[key]

    @property
    def record_assignment(self):
        return {F.LEFT_SIDE: 1, F.RIGHT_SIDE: 2, F.MID_SIDE: 3}.get(self.assignment, 0)


_FRAMES = {}


def frames(carrier):
    """The carrier's frames in plan order (blocksize, then copy), built once."""
    if carrier not in _FRAMES:
        _FRAMES[carrier] = [Frame(carrier, b, c) for b in blocksizes(carrier) for c in range(COPIES)]
    return _FRAMES[carrier]


def pack(layout, pcm, bps):
    """the bytes of one frame's [channel][sample] PCM in a layout (== test_gpu_frame_fields._pack)"""
    a = np.array(pcm, dtype=np.int64)
    if layout == "OUT_PLANAR32":
        return a.astype("<i4").tobytes()
    v = np.ascontiguousarray(a.T).reshape(-1)
    if layout == "OUT_INTERLEAVED32":
        return v.astype("<i4").tobytes()
    if layout == "OUT_FLACDECODER" or bps != 24:
        return (v & 0xFFFF).astype("<u2").tobytes()
    return np.stack([v & 0xFF, (v >> 8) & 0xFF, (v >> 16) & 0xFF], axis=1).astype(np.uint8).tobytes()


# ------------------------------------------------------------------ the plans
def next_pos(at_least, stride, mod, residue):
    """the smallest position p >= at_least whose first byte p * stride is residue modulo mod"""
    assert residue % math.gcd(stride, mod) == 0
    p = at_least
    while (p * stride) % mod != residue:
        p += 1
    return p


def residues(stride, mod):
    """the start residues a leg can reach: the multiples of gcd(stride, mod) below mod"""
    return list(range(0, mod, math.gcd(stride, mod)))


_PLANS = {}


def plan(carrier, layout, kind):
    """-> the position (in samples) of each of frames(carrier), ascending and disjoint.
    line: every start on the leg's line (on 64 bytes where the line is 16).  al16: every start on 16
    bytes, the residues modulo 64 in turn.  mixed: the reachable residues modulo the line in turn
    -- one turn for the blocksizes that are whole chunks and one for the others, so every residue
    meets both -- each frame at the smallest gap of at least one sample that hits its residue."""
    key = (carrier, layout, kind)
    if key in _PLANS:
        return _PLANS[key]
    channels, bps = F.CARRIERS[carrier][:2]
    stride, M = stride_of(layout, channels, bps), line_of(carrier, layout)
    chunk = CHUNK[F.CARRIERS[carrier][3]]
    if kind == "line":
        mod, turn = max(M, 64), [0]
    elif kind == "al16":
        mod, turn = 64, [16, 32, 48, 0]
    else:  # the residues from both ends inwards: the step from one target to the next keeps changing, and so do the gaps
        r = residues(stride, M)
        mod, turn = M, [r[k // 2] if k % 2 == 0 else r[-(k + 1) // 2] for k in range(len(r))]
    count = {True: 0, False: 0}
    out, end = [], 0
    for fr in frames(carrier):
        whole = kind == "mixed" and fr.blocksize % chunk == 0
        p = next_pos(end + (1 if kind == "mixed" else 0), stride, mod, turn[count[whole] % len(turn)])
        count[whole] += 1
        out.append(p)
        end = p + fr.blocksize
    _PLANS[key] = out
    return out


# ------------------------------------------------------------------ the model
def in_range(p, blocksize, stride, out_bytes):
    """the contract's rule in unbounded integers; p is the position before it is taken modulo 2^64"""
    limit = out_bytes // stride
    return 0 <= p and p <= limit and blocksize <= limit - p


def parent_store_range(p, blocksize, stride, out_bytes):
    """What the arithmetic this rule replaces did: the check (out_sample + blocksize) * stride >
    out_bytes and the address out + out_sample * stride, both modulo 2^64.
    -> the byte range relative to d_out that a decoded frame was written to, or None when the check held"""
    x = p % U64
    if (((x + blocksize) % U64) * stride) % U64 > out_bytes:
        return None
    start = (x * stride) % U64
    if start >= 1 << 63:
        start -= U64  # the pointer wraps: a displacement before d_out
    return start, start + blocksize * stride


def parent_fill_range(p, blocksize, stride, out_bytes):
    """the same for k_fill_bad's zero-fill of an ERROR / TRUNC frame: start = out_sample * stride
    modulo 2^64, filled when start <= out_bytes and the length fits behind it"""
    start = ((p % U64) * stride) % U64
    n = blocksize * stride
    if start <= out_bytes and n <= out_bytes - start:
        return start, start + n
    return None


def case_a(d):
    """a position that wraps below zero: one frame too many in front of a window"""
    return -d


def case_b(stride):
    """the first position whose byte offset passes 2^64"""
    return -(-U64 // stride)


def guard_bytes(carrier, layout):
    """front and back guard: at least 4096 bytes and twice the largest frame, a multiple of 256"""
    channels, bps = F.CARRIERS[carrier][:2]
    need = max(4096, 2 * max(blocksizes(carrier)) * stride_of(layout, channels, bps))
    return (need + 255) // 256 * 256


class Item:
    """One entry of a decode call: a frame, the position the contract assigns it (an unbounded
    integer: negative when a header number lies below base_sample), and whether its bytes are cut."""

    def __init__(self, frame, p, *, number=0, variable=False, truncated=False, shares=None):
        self.frame, self.p, self.number, self.variable = frame, p, number, variable
        self.truncated = truncated  # "first" / "last": the batch's last frame in the buffer, cut by nbytes inside that subframe
        self.shares = shares        # index of the item whose bytes this one points at (the cut frame, twice)


def expected(items, layout, stride, out_bytes, front, total):
    """-> (the whole allocation's bytes, per item: 'pcm' | 'zeros' | 'out')"""
    buf = np.full(total, FILL, dtype=np.uint8)
    verdicts = []
    for it in items:
        fr = it.frame
        if not in_range(it.p, fr.blocksize, stride, out_bytes):
            verdicts.append("out")
            continue
        a = front + it.p * stride
        n = fr.blocksize * stride
        assert a + n <= total
        if it.truncated:
            buf[a:a + n] = 0
            verdicts.append("zeros")
        else:
            b = np.frombuffer(pack(layout, fr.pcm, fr.bps), dtype=np.uint8)
            assert len(b) == n
            buf[a:a + n] = b
            verdicts.append("pcm")
    return buf, verdicts


def ranges_inside(items, stride, out_bytes, front, total):
    """Every range a launch can touch lies inside the allocation: the one the contract assigns, and
    the one the wrapping arithmetic this rule replaces would hit.  A batch that fails this is a
    mistake in the test and must not be launched: a kernel that still wraps then fails by
    comparison, never by a fault."""
    bad = []
    for k, it in enumerate(items):
        n = it.frame.blocksize * stride
        cand = []
        if in_range(it.p, it.frame.blocksize, stride, out_bytes):
            cand.append((it.p * stride, it.p * stride + n))
        olds = [parent_store_range(it.p, it.frame.blocksize, stride, out_bytes)]  # a cut frame may be stored in part first
        if it.truncated:
            olds.append(parent_fill_range(it.p, it.frame.blocksize, stride, out_bytes))
        cand += [o for o in olds if o is not None]
        for a, b in cand:
            if not (0 <= front + a and front + b <= total):
                bad.append((k, it.p, a, b))
    return bad


def buffer_of(items, cut=None):
    """-> (the call's frame bytes, the offset of each item, nbytes).  Every item has bytes of its
    own, except one that shares another's; cut: how many bytes of the last frame nbytes keeps."""
    data, offs = bytearray(), []
    for it in items:
        if it.shares is None:
            offs.append(len(data))
            data += it.frame.data(it.number, it.variable)
        else:
            offs.append(None)
    for k, it in enumerate(items):
        if it.shares is not None:
            offs[k] = offs[it.shares]
    nbytes = len(data)
    if cut is not None:
        own = [k for k, it in enumerate(items) if it.shares is None]
        last = own[-1]
        assert items[last].truncated and all(not items[k].truncated or offs[k] == offs[last] for k in range(len(items)))
        nbytes = offs[last] + cut
    else:
        assert not any(it.truncated for it in items)
    return bytes(data), offs, nbytes


def truncation_cut(frame, number, where):
    """Bytes of a frame to keep so that nbytes ends in the middle of its first or its last
    subframe.  The parse walks every subframe but the last (the decode kernel walks that one), so
    it marks the frame TRUNC itself only when the cut lies before the last subframe."""
    code = F.BS_CODE.get(frame.blocksize, 6 if frame.blocksize <= 256 else 7)
    head = 4 + len(F.utf8(number)) + {6: 1, 7: 2}.get(code, 0) + 1  # sync and codes, number, blocksize, CRC-8
    w, edges = F.BitWriter(), [0]
    for ch, sub in enumerate(frame.subs):
        F.write_subframe(w, sub, frame.blocksize, F.sub_bps(frame.bps, frame.assignment, ch))
        edges.append(w.bits())
    lo, hi = (edges[0], edges[1]) if where == "first" else (edges[-2], edges[-1])
    cut = head + (lo + hi) // 16
    assert 8 * head + lo + 64 < 8 * cut < 8 * head + hi - 64 and cut < len(frame.data(number)) - 2
    return cut


def parse_sees_cut(item):
    """the parse itself marks a cut frame TRUNC: the cut lies in a subframe it walks"""
    return item.truncated == "first" and item.frame.channels > 1


# ------------------------------------------------------------------ the batches
class Batch:
    """One bnflac_decode_frames call: its items, out_bytes, and how positions are given --
    table: through d_out_sample, else through the header numbers minus base_sample under the
    STREAMINFO si ('si': min == max == 4096, 'fixed': min == max == SI_FIXED, None: no STREAMINFO)."""

    def __init__(self, carrier, layout, items, out_bytes, *, table=True, base_sample=0, si="si", cut=None):
        self.carrier, self.layout, self.items, self.out_bytes = carrier, layout, items, out_bytes
        self.table, self.base_sample, self.si, self.cut = table, base_sample, si, cut
        self.channels, self.bps = F.CARRIERS[carrier][:2]
        self.stride = stride_of(layout, self.channels, self.bps)
        self.front = self.back = guard_bytes(carrier, layout)
        self.total = self.front + out_bytes + self.back

    def expected(self):
        return expected(self.items, self.layout, self.stride, self.out_bytes, self.front, self.total)

    def unsafe(self):
        return ranges_inside(self.items, self.stride, self.out_bytes, self.front, self.total)

    def buffer(self):
        return buffer_of(self.items, self.cut)

    def header_sample(self, it):
        """the sample number the contract reads from an item's header"""
        if it.variable:
            return it.number
        return it.number * (SI_FIXED if self.si == "fixed" else it.frame.blocksize if self.si is None else F.SI_BLOCKSIZE)


def _leg(carrier, layout):
    channels, bps = F.CARRIERS[carrier][:2]
    return frames(carrier), stride_of(layout, channels, bps)


def pick(carrier, blocksize, copy):
    return next(f for f in frames(carrier) if f.blocksize == blocksize and f.copy == copy)


def batch_table(carrier, layout, kind):
    """a: a plan through d_out_sample; out_bytes ends with the last frame"""
    frs, stride = _leg(carrier, layout)
    pos = plan(carrier, layout, kind)
    items = [Item(f, p, number=i) for i, (f, p) in enumerate(zip(frs, pos))]
    return Batch(carrier, layout, items, (pos[-1] + frs[-1].blocksize) * stride)


def batch_header_variable(carrier, layout):
    """b: the mixed plan through the headers' 36-bit sample numbers (7-byte coding) minus base_sample"""
    frs, stride = _leg(carrier, layout)
    pos = plan(carrier, layout, "mixed")
    items = [Item(f, p, number=HEADER_BASE + p, variable=True) for f, p in zip(frs, pos)]
    return Batch(carrier, layout, items, (pos[-1] + frs[-1].blocksize) * stride, table=False, base_sample=HEADER_BASE)


def batch_header_fixed(carrier, layout, si):
    """b: fixed-blocksize frames, the position number * blocksize (no STREAMINFO) or number *
    min_blocksize (STREAMINFO min == max) minus a base_sample that is not 0: each frame takes the
    first frame number that puts it behind the previous frame"""
    frs, stride = _leg(carrier, layout)
    base, end, items = 1000, 0, []
    for f in frs:
        unit = SI_FIXED if si == "fixed" else f.blocksize
        number = -(-(end + base) // unit)
        p = number * unit - base
        items.append(Item(f, p, number=number))
        end = p + f.blocksize
    return Batch(carrier, layout, items, end * stride, table=False, base_sample=base, si=si)


def batch_cut(carrier, layout):
    """c: the mixed plan, then -- around limit = out_bytes // stride -- a truncated frame in range
    (zero-filled), a frame that ends exactly at limit (written), one that ends one sample past it,
    one that starts at limit, one that starts past it, and the truncated frame again across the
    cut (untouched).  out_bytes is not a multiple of the stride."""
    frs, stride = _leg(carrier, layout)
    pos = plan(carrier, layout, "mixed")
    items = [Item(f, p, number=i) for i, (f, p) in enumerate(zip(frs, pos))]
    end = pos[-1] + frs[-1].blocksize
    t, x, y, z, z2 = (pick(carrier, b, c) for b, c in ((97, 0), (64, 1), (33, 2), (96, 3), (129, 4)))
    p_t = end + 3
    p_x = p_t + t.blocksize + 2
    limit = p_x + x.blocksize
    n = len(items)
    items += [Item(x, p_x, number=n), Item(y, limit + 1 - y.blocksize, number=n + 1), Item(z, limit + 1, number=n + 2),
              Item(z2, limit, number=n + 3), Item(t, p_t, number=n + 4, truncated="first")]
    items.append(Item(t, limit - t.blocksize // 2, number=n + 4, truncated="first", shares=len(items) - 1))
    return Batch(carrier, layout, items, limit * stride + stride - 1, cut=truncation_cut(t, n + 4, "first"))


WRAP_LEGS = [("M16", "OUT_FLACDECODER"), ("W32", "OUT_FILEREADER"), ("S16", "OUT_FLACDECODER"), ("S16", "OUT_FILEREADER"),
             ("S24", "OUT_FILEREADER"), ("S24", "OUT_PLANAR32"), ("S16", "OUT_INTERLEAVED32"), ("T24", "OUT_FILEREADER"),
             ("T24", "OUT_INTERLEAVED32")]  # strides 2, 2, 4, 4, 6, 8, 8, 9, 12: every kernel, every stride in use


def batch_wrap_table(carrier, layout):
    """d: every fifth frame of the mixed plan, and through the table: three case A positions
    (2^64 - d for d = 1, d = blocksize and a d between), a case B position (ceil(2^64 / stride)),
    and a truncated frame at the case B position.  All five are out of range."""
    frs, stride = _leg(carrier, layout)
    pos = plan(carrier, layout, "mixed")
    items = [Item(f, p, number=i) for i, (f, p) in enumerate(zip(frs, pos))][::5]
    a1, a2, a3, b, t = (pick(carrier, bs, c) for bs, c in ((64, 1), (33, 2), (129, 3), (96, 4), (97, 5)))
    items += [Item(a1, case_a(1), number=200), Item(a2, case_a(a2.blocksize), number=201), Item(a3, case_a(60), number=202),
              Item(b, case_b(stride), number=203), Item(t, case_b(stride), number=204, truncated="last")]
    return Batch(carrier, layout, items, (pos[-1] + frs[-1].blocksize) * stride, cut=truncation_cut(t, 204, "last"))


def batch_wrap_header(carrier, layout):
    """d: every fifth frame of the mixed plan by its header's sample number, and two frames whose
    number lies below base_sample by d = 1 and by d = blocksize (case A through the header)"""
    frs, stride = _leg(carrier, layout)
    pos = plan(carrier, layout, "mixed")
    items = [Item(f, p, number=HEADER_BASE + p, variable=True) for f, p in zip(frs, pos)][::5]
    a1, a2 = pick(carrier, 64, 1), pick(carrier, 33, 2)
    items += [Item(a1, case_a(1), number=HEADER_BASE - 1, variable=True),
              Item(a2, case_a(a2.blocksize), number=HEADER_BASE - a2.blocksize, variable=True)]
    return Batch(carrier, layout, items, (pos[-1] + frs[-1].blocksize) * stride, table=False, base_sample=HEADER_BASE)


FIXED_LEGS = [("S16", "OUT_FLACDECODER"), ("S24", "OUT_FILEREADER"), ("M16", "OUT_FILEREADER"), ("T24", "OUT_PLANAR32"),
              ("W32", "OUT_INTERLEAVED32")]  # the fixed-blocksize header runs: one layout per carrier


def all_batches():
    """every batch tests/test_gpu_out_placement.py launches, by name"""
    out = {}
    for carrier, layout in LEGS:
        for kind in PLANS:
            out[f"a/{carrier}/{layout}/{kind}"] = batch_table(carrier, layout, kind)
        out[f"b/{carrier}/{layout}/variable"] = batch_header_variable(carrier, layout)
        out[f"c/{carrier}/{layout}"] = batch_cut(carrier, layout)
    for carrier, layout in FIXED_LEGS:
        out[f"b/{carrier}/{layout}/fixed_no_streaminfo"] = batch_header_fixed(carrier, layout, None)
        out[f"b/{carrier}/{layout}/fixed_streaminfo"] = batch_header_fixed(carrier, layout, "fixed")
    for carrier, layout in WRAP_LEGS:
        out[f"d/{carrier}/{layout}/table"] = batch_wrap_table(carrier, layout)
        out[f"d/{carrier}/{layout}/header"] = batch_wrap_header(carrier, layout)
    return out
