"""A field-explicit FLAC frame writer, an exact-integer reference, and the table of hand-built
frames at the bitstream's limits (tests/test_frame_fields_host.py, tests/test_gpu_frame_fields.py).

Nothing here comes from the project: Python integers, a bit writer, CRC-8 / CRC-16 written out
bit by bit, hashlib for the STREAMINFO MD5.  The writer takes every field as given (RFC 9639
section 9), also fields that contradict each other, so the table can hold what no optimising
encoder writes: every Rice parameter, escapes of every width, partition orders up to 15, LPC
precisions and shifts at their ends (negative shifts included), every header code, and the field
values a decoder must refuse.

restore() is the decoder of RFC 9639 in unbounded integers.  It raises RangeError when a value
leaves what the frame's arithmetic can hold (a sample outside its subframe's width, a predictor sum
outside the 32- or 64-bit accumulator of the path libFLAC picks, a negative shift): rows it accepts
are "in spec" and their PCM is restore()'s; the rest are "libFLAC-defined" and the CPU oracle says
what they decode to.
"""
import hashlib
import random
from types import SimpleNamespace


class RangeError(ValueError):
    """the frame leaves what RFC 9639 defines"""


# ------------------------------------------------------------------ bits and checksums
class BitWriter:
    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.n = 0

    def write(self, v, nbits):
        if nbits <= 0:
            return
        self.acc = (self.acc << nbits) | (v & ((1 << nbits) - 1))
        self.n += nbits
        if self.n >= 64:
            r = self.n & 7
            self.buf += (self.acc >> r).to_bytes((self.n - r) >> 3, "big")
            self.acc &= (1 << r) - 1
            self.n = r

    def unary(self, q):
        """q zeros and a one"""
        self.write(1, q + 1)

    def bits(self):
        return 8 * len(self.buf) + self.n

    def pad(self, value=0):
        r = -self.bits() & 7
        self.write(value, r)
        return r

    def getvalue(self):
        assert self.n % 8 == 0, "not byte aligned"
        return bytes(self.buf) + (self.acc.to_bytes(self.n >> 3, "big") if self.n else b"")


def crc8(data):
    """CRC-8, polynomial x^8 + x^2 + x + 1, initial value 0"""
    c = 0
    for byte in data:
        c ^= byte
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xFF if c & 0x80 else (c << 1) & 0xFF
    return c


def crc16(data):
    """CRC-16, polynomial x^16 + x^15 + x^2 + 1, initial value 0"""
    c = 0
    for byte in data:
        c ^= byte << 8
        for _ in range(8):
            c = ((c << 1) ^ 0x8005) & 0xFFFF if c & 0x8000 else (c << 1) & 0xFFFF
    return c


def utf8(v, nbytes=None):
    """The frame / sample number, 1..7 bytes (36 bits); nbytes forces a longer coding than v needs."""
    if nbytes is None:
        nbytes = 1 if v < 0x80 else next(n for n in range(2, 8) if v < 1 << (5 * n + 1))
    if nbytes == 1:
        assert v < 0x80
        return bytes([v])
    assert 2 <= nbytes <= 7 and v < 1 << (5 * nbytes + 1)
    first = (0xFF << (8 - nbytes)) & 0xFF
    out = [first | (v >> (6 * (nbytes - 1)))]
    for i in range(nbytes - 2, -1, -1):
        out.append(0x80 | ((v >> (6 * i)) & 0x3F))
    return bytes(out)


def ilog2(v):
    return v.bit_length() - 1


def fits(v, bits):
    return bits > 0 and -(1 << (bits - 1)) <= v < (1 << (bits - 1)) or (bits <= 0 and v == 0)


def zigzag(r):
    return (r << 1) if r >= 0 else ((-r) << 1) - 1


def unzig(u):
    return (u >> 1) ^ -(u & 1)


# ------------------------------------------------------------------ the frame writer
BS_CODE = {192: 1, 576: 2, 1152: 3, 2304: 4, 4608: 5, 256: 8, 512: 9, 1024: 10, 2048: 11, 4096: 12, 8192: 13,
           16384: 14, 32768: 15}
BS_OF_CODE = {c: b for b, c in BS_CODE.items()}
SR_OF_CODE = {1: 88200, 2: 176400, 3: 192000, 4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000, 9: 44100, 10: 48000,
              11: 96000}
BPS_CODE = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6}
LEFT_SIDE, RIGHT_SIDE, MID_SIDE = 8, 9, 10  # channel codes of the stereo decorrelations (independent: channels - 1)
TYPE_CODE = {"constant": lambda s: 0, "verbatim": lambda s: 1, "fixed": lambda s: 8 + s["order"],
             "lpc": lambda s: 32 + s["order"] - 1}


def sub_bps(bps, assignment, ch):
    """the side channel is one bit wider"""
    return bps + 1 if (assignment in (LEFT_SIDE, MID_SIDE) and ch == 1) or (assignment == RIGHT_SIDE and ch == 0) else bps


def partition_counts(blocksize, order, porder):
    if porder == 0:
        return [max(blocksize - order, 0)]
    ps = blocksize >> porder
    return [max(ps - order, 0)] + [ps] * ((1 << porder) - 1)


def write_subframe(w, sub, blocksize, sbps):
    """One subframe, field by field.  sub: type ('constant' | 'verbatim' | 'fixed' | 'lpc'), wasted,
    value (constant), samples (verbatim), order, warm, prec, shift, coef, rice2, porder,
    parts = [(k, esc_bits | None), ...], res.  Sample values are those of the bitstream (before the
    wasted bits are put back).  Raw overrides: first_bit, type_code, prec_code, method."""
    t = sub["type"]
    wasted = sub.get("wasted", 0)
    w.write(sub.get("first_bit", 0), 1)
    w.write(sub["type_code"] if "type_code" in sub else TYPE_CODE[t](sub), 6)
    w.write(1 if wasted else 0, 1)
    if wasted:
        w.unary(wasted - 1)
    eb = sbps - wasted
    if t == "constant":
        w.write(sub["value"], eb)
        return
    if t == "verbatim":
        for v in sub["samples"]:
            w.write(v, eb)
        return
    order = sub["order"]
    assert len(sub["warm"]) == order
    for v in sub["warm"]:
        w.write(v, eb)
    if t == "lpc":
        prec = sub["prec"]
        w.write(sub["prec_code"] if "prec_code" in sub else prec - 1, 4)
        w.write(sub["shift"], 5)
        assert len(sub["coef"]) == order
        for c in sub["coef"]:
            w.write(c, prec)
    rice2 = sub.get("rice2", 0)
    w.write(sub["method"] if "method" in sub else rice2, 2)
    porder = sub["porder"]
    w.write(porder, 4)
    plen, pesc = (5, 31) if rice2 else (4, 15)
    res = sub["res"]
    counts = partition_counts(blocksize, order, porder)
    parts = sub["parts"]
    assert len(parts) == len(counts), (len(parts), len(counts))
    i = 0
    for (k, esc), cnt in zip(parts, counts):
        if esc is None:
            assert k < pesc
            w.write(k, plen)
            for r in res[i:i + cnt]:
                u = zigzag(r)
                w.unary(u >> k)
                w.write(u, k)
        else:
            w.write(pesc, plen)
            w.write(esc, 5)
            for r in res[i:i + cnt]:
                w.write(r, esc)
        i += cnt


def frame(subs, blocksize, bps, *, number=0, variable=False, assignment=None, bs_code=None, sr_code=9, sr_extra=0,
          bps_code=None, reserved1=0, reserved2=0, number_bytes=None, number_raw=None, pad_bits=0, crc8_value=None,
          crc16_value=None):
    """One frame from its fields.  assignment: the 4-bit channel code (default: len(subs) - 1);
    bs_code / bps_code default to the code of blocksize / bps (6 or 7, and 0, when there is none);
    number_raw replaces the coded number's bytes; padding and both CRCs are computed unless given."""
    if assignment is None:
        assignment = len(subs) - 1
    if bs_code is None:
        bs_code = BS_CODE.get(blocksize, 6 if blocksize <= 256 else 7)
    if bps_code is None:
        bps_code = BPS_CODE.get(bps, 0)
    h = bytearray([0xFF, 0xF8 | (reserved1 << 1) | (1 if variable else 0), (bs_code << 4) | sr_code,
                   (assignment << 4) | (bps_code << 1) | reserved2])
    h += number_raw if number_raw is not None else utf8(number, number_bytes)
    if bs_code == 6:
        h.append((blocksize - 1) & 0xFF)
    elif bs_code == 7:
        h += ((blocksize - 1) & 0xFFFF).to_bytes(2, "big")
    if sr_code == 12:
        h.append(sr_extra & 0xFF)
    elif sr_code in (13, 14):
        h += (sr_extra & 0xFFFF).to_bytes(2, "big")
    h.append(crc8(h) if crc8_value is None else crc8_value)
    w = BitWriter()
    for ch, sub in enumerate(subs):
        write_subframe(w, sub, blocksize, sub_bps(bps, assignment, ch))
    w.pad(pad_bits)
    body = bytes(h) + w.getvalue()
    return body + (crc16(body) if crc16_value is None else crc16_value).to_bytes(2, "big")


# ------------------------------------------------------------------ the exact reference
FIXED_ROWS = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}


def lpc_path(eb, prec, order):
    """the restore routine libFLAC 1.2.1 picks (read_subframe_lpc_): 16-bit MMX, 32-bit, 64-bit"""
    if eb + prec + ilog2(order) <= 32:
        return "mmx16" if eb <= 16 and prec <= 16 and order >= 4 else "ia32"
    return "wide"


def predict(sub, x, n):
    """(sum of coefficient * history, shift) for sample n of a FIXED / LPC subframe with samples x[:n]"""
    if sub["type"] == "fixed":
        c, shift = FIXED_ROWS[sub["order"]], 0
    else:
        c, shift = sub["coef"], sub["shift"]
    return sum(c[j] * x[n - 1 - j] for j in range(len(c))), shift


def restore(sub, blocksize, sbps):
    """The samples of one subframe (wasted bits put back) in unbounded integers:
    x[n] = r[n] + (sum_j c[j] * x[n-1-j] >> shift), FIXED as its coefficient rows.  RangeError when
    the subframe leaves what RFC 9639 defines or what its libFLAC path can hold."""
    t = sub["type"]
    wasted = sub.get("wasted", 0)
    eb = sbps - wasted
    if eb < 0 or (eb == 0 and t != "constant" and t != "verbatim"):
        raise RangeError("no bits left after the wasted bits")
    if t == "constant":
        x = [sub["value"]] * blocksize
    elif t == "verbatim":
        x = list(sub["samples"])
        assert len(x) == blocksize
    else:
        order = sub["order"]
        if order > blocksize:
            raise RangeError("order above the blocksize")
        if t == "lpc":
            if sub["shift"] < 0:
                raise RangeError("negative shift")
            if not all(fits(c, sub["prec"]) for c in sub["coef"]):
                raise RangeError("coefficient outside its precision")
            lim = 63 if lpc_path(eb, sub["prec"], order) == "wide" else 31
        else:
            lim = 31
        x = list(sub["warm"])
        res = sub["res"]
        if len(res) != blocksize - order:
            raise RangeError("residual count")
        for r in res:
            if not -(1 << 31) < r < (1 << 31):
                raise RangeError("residual outside 32 bits")
            s, shift = predict(sub, x, len(x))
            if not -(1 << lim) <= s < (1 << lim):
                raise RangeError("predictor sum outside the path's accumulator")
            x.append(r + (s >> shift))
    for v in x:
        if not fits(v, eb):
            raise RangeError(f"sample {v} outside {eb} bits")
    return [v << wasted for v in x]


def decorrelate(assignment, a, b):
    if assignment == LEFT_SIDE:
        return a, [l - s for l, s in zip(a, b)]
    if assignment == RIGHT_SIDE:
        return [s + r for s, r in zip(a, b)], b
    if assignment == MID_SIDE:
        left, right = [], []
        for m, s in zip(a, b):
            m = (m << 1) | (s & 1)
            left.append((m + s) >> 1)
            right.append((m - s) >> 1)
        return left, right
    return a, b


def frame_pcm(subs, blocksize, bps, assignment=None, keep=None):
    """[channel][sample] of a frame, or RangeError.  keep: a list that receives the subframes' samples"""
    if assignment is None:
        assignment = len(subs) - 1
    ch = [restore(s, blocksize, sub_bps(bps, assignment, i)) for i, s in enumerate(subs)]
    if keep is not None:
        keep += ch
    if assignment >= 8:
        ch = list(decorrelate(assignment, ch[0], ch[1]))
    for c in ch:
        for v in c:
            if not fits(v, bps):
                raise RangeError(f"sample {v} outside {bps} bits after decorrelation")
    return ch


def encode_residual(sub, signal):
    """Fill warm and res of a FIXED / LPC subframe so that it restores to signal (bitstream values)."""
    order = sub["order"]
    sub["warm"] = list(signal[:order])
    res = []
    for n in range(order, len(signal)):
        s, shift = predict(sub, signal, n)
        res.append(signal[n] - (s >> shift))
    sub["res"] = res
    return sub


def md5_of(pcm_frames, bps):
    """STREAMINFO's MD5: the samples interleaved, little-endian, in whole bytes"""
    nb = (bps + 7) // 8
    m = hashlib.md5()
    for chans in pcm_frames:
        buf = bytearray()
        for i in range(len(chans[0])):
            for c in chans:
                buf += (c[i] & ((1 << (8 * nb)) - 1)).to_bytes(nb, "little")
        m.update(bytes(buf))
    return m.digest()


def stream(frames, pcm_frames, *, channels, bps, sample_rate=44100, min_blocksize=None, max_blocksize=None,
           total=None, md5=None):
    """fLaC + STREAMINFO (the last metadata block) + the frames.  total: STREAMINFO's sample count
    (default: the frames' sum; 0 says "unknown")"""
    sizes = [len(c[0]) for c in pcm_frames]
    total = sum(sizes) if total is None else total
    mn = min(sizes) if min_blocksize is None else min_blocksize
    mx = max(sizes) if max_blocksize is None else max_blocksize
    si = mn.to_bytes(2, "big") + mx.to_bytes(2, "big")
    si += min(len(f) for f in frames).to_bytes(3, "big") + max(len(f) for f in frames).to_bytes(3, "big")
    si += ((sample_rate << 44) | ((channels - 1) << 41) | ((bps - 1) << 36) | total).to_bytes(8, "big")
    si += md5_of(pcm_frames, bps) if md5 is None else md5
    return b"fLaC" + b"\x80\x00\x00\x22" + si + b"".join(frames)


# ------------------------------------------------------------------ which kernel takes a frame, and keeps it
# The rules are those written in the kernels: k_parse's class flags (bnflac_kernels.hip, "decode
# instance"), st_setup and k_decode_st's range check, sw_setup, and k_decode_sys's header comment.
def _lpc_orders(subs):
    return [s["order"] for s in subs if s["type"] == "lpc"]


def lane_kernel(subs, channels, bps):
    mo = max(_lpc_orders(subs), default=0)
    raw = any(s["type"] in ("constant", "verbatim") for s in subs)
    if channels == 2 and 16 < bps <= 24 and 0 < mo <= 12 and not raw:
        return "k_decode_sw"
    if mo > 16:
        return "k_decode<32>"
    if mo > 8 or (mo > 0 and bps > 16):
        return "k_decode<16>"
    if channels == 2 and bps <= 16 and not raw:
        return "k_decode_st"
    return "k_decode<8>"


def _paths(subs, bps, assignment):
    out = []
    for ch, s in enumerate(subs):
        eb = sub_bps(bps, assignment, ch) - s.get("wasted", 0)
        out.append(lpc_path(eb, s["prec"], s["order"]) if s["type"] == "lpc" else None)
    return out


def st_keeps(subs, bps, assignment, samples):
    """k_decode_st: FIXED / LPC below the 64-bit path, every bitstream sample inside int16.
    samples: per channel, the subframe's samples before the wasted bits go back (None: in range)"""
    for ch, (s, p) in enumerate(zip(subs, _paths(subs, bps, assignment))):
        if p == "wide" or sub_bps(bps, assignment, ch) - s.get("wasted", 0) > 17:
            return False
        if samples is not None and not all(-32768 <= v <= 32767 for v in samples[ch]):
            return False
    return True


def sw_keeps(subs, bps, assignment):
    """k_decode_sw: orders <= 12, no MMX16 subframe, no 64-bit shift of 32 or more"""
    for s, p in zip(subs, _paths(subs, bps, assignment)):
        if s.get("order", 0) > 12 or p == "mmx16" or (p == "wide" and s["shift"] < 0):
            return False
    return True


def sys_keeps(subs, bps, assignment, samples):
    """k_decode_sys: no 64-bit shift of 32 or more, no MMX16 subframe leaving int16"""
    for ch, (s, p) in enumerate(zip(subs, _paths(subs, bps, assignment))):
        if p == "wide" and s["shift"] < 0:
            return False
        if p == "mmx16" and samples is not None and not all(-32768 <= v <= 32767 for v in samples[ch]):
            return False
    return True


# ------------------------------------------------------------------ the case table
CARRIERS = {  # name: (channels, bps, largest LPC order, the lane kernel it is built for)
    "S16": (2, 16, 8, "k_decode_st"),
    "S24": (2, 24, 12, "k_decode_sw"),
    "M16": (1, 16, 8, "k_decode<8>"),
    "T24": (3, 24, 16, "k_decode<16>"),
    "W32": (1, 16, 32, "k_decode<32>"),
}
SI_BLOCKSIZE, SI_RATE = 4096, 44100  # the STREAMINFO every "with STREAMINFO" row is decoded under
ASSIGN_NAME = {LEFT_SIDE: "ls", RIGHT_SIDE: "rs", MID_SIDE: "ms"}
DROPPED = []  # (name, reason): variants that are not legal in a carrier's frame shape


def lpc_sub(rng, order, prec, shift, wasted=0):
    """An LPC subframe header with gain sum|c| / 2^shift <= 1/2 where the precision allows it
    (shift 0: [1, -1, 0, ...], gain at most 1 per step; the rows keep their residuals tiny)."""
    hi, lo = (1 << (prec - 1)) - 1, -(1 << (prec - 1))
    c = [0] * order
    if shift <= 0:
        if prec >= 2 and order >= 2:
            c[0], c[1] = 1, -1
        else:
            c[0] = -1
    else:
        budget = (1 << shift) >> 1
        per = budget // order
        if per >= 1:
            for j in range(order):
                c[j] = max(lo, min(hi, rng.randint(-per, per)))
            if c[0] == 0:
                c[0] = max(lo, -per)
            if c[-1] == 0:
                c[-1] = max(lo, -1)
        else:
            for j in rng.sample(range(order), max(budget, 1)):
                c[j] = -1
    return {"type": "lpc", "order": order, "prec": prec, "shift": shift, "coef": c, "wasted": wasted}


def fixed_sub(order, wasted=0):
    return {"type": "fixed", "order": order, "wasted": wasted}


def default_subs(rng, carrier):
    """the carrier's usual predictors: between them the MMX16, 32-bit and 64-bit paths"""
    if carrier == "S16":
        return [lpc_sub(rng, 8, 12, 11), lpc_sub(rng, 2, 10, 9)]
    if carrier == "S24":
        return [lpc_sub(rng, 12, 14, 13), lpc_sub(rng, 4, 5, 4)]
    if carrier == "M16":
        return [lpc_sub(rng, 6, 12, 11)]
    if carrier == "T24":
        return [lpc_sub(rng, 12, 14, 13), lpc_sub(rng, 3, 6, 5), fixed_sub(0)]
    return [lpc_sub(rng, 20, 12, 11)]


def sample_cap(carrier, wasted=0):
    """bits the carrier's bitstream samples may use, the side channel's too: its extra bit stays
    unused, so that an S16 row leaves int16 only where it says so"""
    return CARRIERS[carrier][1] - wasted


def fill_rice(rng, sub, blocksize, porder, ks, kind, cap_bits, rice2, targets=()):
    """parts / res of a Rice-coded subframe.  kind: 'q0' quotients all 0, 'q3' quotients 0..3,
    'big' one codeword per partition with q + k + 1 = a target (the rest near zero).
    -> False when the carrier's sample range does not allow the variant."""
    counts = partition_counts(blocksize, sub["order"], porder)
    ucap = 1 << (cap_bits - 2)  # |r| <= 2^(bits-3): a gain of 1/2 keeps |x| <= 2^(bits-2)
    ubig = 1 << (cap_bits - 1)  # one |r| <= 2^(bits-2) per partition, the others near zero
    parts, res = [], []
    for p, cnt in enumerate(counts):
        k = ks[p % len(ks)]
        parts.append((k, None))
        if kind == "q0":
            us = [rng.randrange(min(1 << k, ucap)) for _ in range(cnt)]
        elif kind == "q3":
            if (4 << k) > ucap:
                return False
            us = [(rng.randrange(4) << k) | rng.randrange(1 << k) for _ in range(cnt)]
        else:
            ok = [t for t in targets if t - k - 1 >= 0 and ((t - k) << k) <= ubig]
            if not ok:
                return False
            us = [rng.randrange(min(1 << k, 32)) for _ in range(cnt)]
            if cnt:
                t = ok[p % len(ok)]
                us[rng.randrange(cnt)] = ((t - k - 1) << k) | rng.randrange(1 << k)
        res += [unzig(u) for u in us]
    sub.update(rice2=rice2, porder=porder, parts=parts, res=res)
    return True


def warm_for(rng, sub, cap_bits, small=False):
    m = 8 if small else 1 << (cap_bits - 3)
    sub["warm"] = [rng.randint(-m, m - 1) for _ in range(sub["order"])]


def layout(rng, order, porder):
    """a blocksize in 16..192 that 2^porder divides, partition 0 not empty"""
    ok = [b for b in (16, 24, 40, 48, 64, 72, 80, 96, 104, 112, 120, 128, 144, 152, 160, 176, 192)
          if b % (1 << porder) == 0 and (b >> porder) > order]
    if porder == 0:
        ok += [b for b in (17, 33, 50, 99, 150, 191) if b > order]
    return rng.choice(ok)


class _Table:
    def __init__(self):
        self.rows = []
        self.names = set()

    def add(self, name, group, carrier, subs, blocksize, bps, *, expect="restore", si=True, assignment=None,
            hdr=None, pre=None, pre_samples=None, **kw):
        """expect: 'restore' (in spec: PCM is restore()'s), 'oracle' (libFLAC-defined: the oracle's
        PCM or refusal).  hdr: the header fields a row is about, checked against what the writer was given."""
        assert name not in self.names, name
        self.names.add(name)
        channels = len(subs)
        if assignment is None:
            assignment = channels - 1
        data = frame(subs, blocksize, bps, assignment=assignment, **kw)
        pcm = samples = None
        if expect == "restore":
            samples = []
            pcm = pre or frame_pcm(subs, blocksize, bps, assignment, samples)
            samples = [[v >> s.get("wasted", 0) for v in c] for s, c in zip(subs, pre_samples or samples)]
        kern = lane_kernel(subs, channels, bps)
        lane_kept = (st_keeps(subs, bps, assignment, samples) if kern == "k_decode_st"
                     else sw_keeps(subs, bps, assignment) if kern == "k_decode_sw" else True)
        coded = any(s["type"] in ("fixed", "lpc") for s in subs)
        src = kw.get("sr_code", 9)
        fields = {"blocksize": blocksize, "channels": channels, "bps": bps,
                  "assignment": {LEFT_SIDE: 1, RIGHT_SIDE: 2, MID_SIDE: 3}.get(assignment, 0),
                  "sample_rate": SI_RATE if src == 0 else SR_OF_CODE[src] if src in SR_OF_CODE
                  else kw.get("sr_extra", 0) * {12: 1000, 13: 1, 14: 10}.get(src, 0),
                  "number_type": int(bool(kw.get("variable"))), "number": kw.get("number", 0)}
        assert all(fields[k] == v for k, v in (hdr or {}).items()), (name, hdr, fields)
        self.rows.append(SimpleNamespace(
            name=name, group=group, carrier=carrier, data=data, channels=channels, bps=bps, blocksize=blocksize,
            subs=subs, assignment=assignment, si=si, expect=expect, pcm=pcm, fields=fields, kernel=kern,
            lane_kept=lane_kept, sys_kept=sys_keeps(subs, bps, assignment, samples), coded=coded,
            marks=group in "ABCDEF"))

    def add_stereo(self, name, group, carrier, subs, blocksize, bps, idx, **kw):
        """a 2-channel carrier row under the idx-th stereo assignment; independent when the
        decorrelated samples would leave the sample range"""
        for a in ((1, LEFT_SIDE, RIGHT_SIDE, MID_SIDE)[idx % 4], 1):  # 1: two independent channels
            try:
                samples = []
                pcm = frame_pcm(subs, blocksize, bps, a, samples)
            except RangeError:
                continue
            return self.add(f"{name}/{ASSIGN_NAME.get(a, 'indep')}", group, carrier, subs, blocksize, bps, assignment=a,
                            pre=pcm, pre_samples=samples, **kw)
        raise AssertionError(f"{name}: not in range under any assignment")

    def put(self, name, group, carrier, subs, blocksize, idx, **kw):
        channels, bps = CARRIERS[carrier][:2]
        if channels == 2 and "assignment" not in kw:
            return self.add_stereo(name, group, carrier, subs, blocksize, bps, idx, **kw)
        return self.add(name, group, carrier, subs, blocksize, bps, **kw)


def _group_a(T, rng):
    ks4, ks5 = (0, 1, 9, 10, 11, 14), (0, 14, 15, 16, 30)
    for carrier in CARRIERS:
        cap = sample_cap(carrier)
        n = 0
        for rice2, ks in ((0, ks4), (1, ks5)):
            for k in ks:
                for kind in ("q0", "q3", "big"):
                    name = f"A/{carrier}/rice{'2' if rice2 else ''}_k{k}_{kind}"
                    subs = default_subs(rng, carrier)
                    porder = 3 if kind == "big" else rng.choice((0, 1, 2))
                    bs = layout(rng, max(s["order"] for s in subs), porder)
                    ok = True
                    for s in subs:
                        warm_for(rng, s, cap, small=kind == "big")
                        ok = ok and fill_rice(rng, s, bs, porder, [k], kind, cap, rice2, (31, 32, 33, 40, 70))
                    if not ok:
                        DROPPED.append((name, f"the codewords leave {cap}-bit samples"))
                        continue
                    T.put(name, "A", carrier, subs, bs, n)
                    n += 1
        subs = default_subs(rng, carrier)  # the bulk / plain choice and the lanes' k change inside a subframe
        bs = layout(rng, max(s["order"] for s in subs), 3)
        for s in subs:
            warm_for(rng, s, cap)
            assert fill_rice(rng, s, bs, 3, [0, 14], "q0", cap, 0)
        T.put(f"A/{carrier}/rice_k0_k14_alternating", "A", carrier, subs, bs, n)


def fill_parts(rng, sub, blocksize, porder, spec, cap_bits, rice2):
    """spec: per partition a Rice parameter k, or ('esc', width)"""
    counts = partition_counts(blocksize, sub["order"], porder)
    assert len(spec) == len(counts)
    rmax = 1 << (cap_bits - 3)
    parts, res = [], []
    for sp, cnt in zip(spec, counts):
        if isinstance(sp, tuple):
            n = sp[1]
            parts.append((0, n))
            lo, hi = (0, 0) if n == 0 else (max(-(1 << (n - 1)), -rmax), min((1 << (n - 1)) - 1, rmax - 1))
            res += [rng.randint(lo, hi) for _ in range(cnt)]
        else:
            parts.append((sp, None))
            res += [unzig(rng.randrange(min(2 << sp, 2 * rmax))) for _ in range(cnt)]
    sub.update(rice2=rice2, porder=porder, parts=parts, res=res)


def _group_b(T, rng):
    for carrier, (channels, bps, maxo, _) in CARRIERS.items():
        cap = sample_cap(carrier)
        n = 0
        for rice2 in (0, 1):
            tag = "rice2" if rice2 else "rice"

            def row(desc, spec, porder=2, bs=None):
                nonlocal n
                subs = default_subs(rng, carrier)
                b = bs or layout(rng, max(s["order"] for s in subs), porder)
                for s in subs:
                    warm_for(rng, s, cap)
                    fill_parts(rng, s, b, porder, spec, cap, rice2)
                T.put(f"B/{carrier}/{tag}_{desc}", "B", carrier, subs, b, n)
                n += 1

            for w in (0, 1, 2, 16, 25, 31):  # in-range values, sign-extended to the width
                row(f"esc{w}_middle", [3, ("esc", w), 2, 4])
            if channels == 2:  # an escape of bps + 1 bits needs the side channel's extra bit (S16: the side leaves int16)
                full = 1 << (bps - 1)
                left = [rng.randint(-full + 500, full - 500) for _ in range(64)]
                right = [rng.randint(-full + 500, full - 500) for _ in range(64)]
                side = fixed_sub(0)
                side.update(warm=[], res=[l - r for l, r in zip(left, right)], rice2=rice2, porder=0, parts=[(0, bps + 1)])
                assert any(not fits(v, bps) for v in side["res"])
                first = _from_signal(rng, default_subs(rng, carrier)[0], left, 64, 2, rice2)
                T.add(f"B/{carrier}/{tag}_esc{bps + 1}_side", "B", carrier, [first, side], 64, bps, assignment=LEFT_SIDE)
            row("esc0_first", [("esc", 0), 3, 2, 4])
            row("esc0_last", [3, 2, 4, ("esc", 0)])
            row("esc_every", [("esc", w) for w in (5, 9, 1, 13, 0, 11, 7, 2)], porder=3)
            row("esc_alternating", [("esc", 6), 3, ("esc", 10), 0, ("esc", 3), 5, ("esc", 12), 1], porder=3)
            o = max(s["order"] for s in default_subs(rng, carrier))
            row("esc_after_empty", [4, ("esc", 9), 2, ("esc", 4)], bs=4 * o)  # partition 0 of the longest predictor is empty


def _signal(rng, n, amp, step):
    """a bounded walk: |x| <= amp, |x[n] - x[n-1]| <= step"""
    x, v = [], 0
    for _ in range(n):
        v = max(-amp, min(amp - 1, v + rng.randint(-step, step)))
        x.append(v)
    return x


def code_partitions(rng, sub, blocksize, porder, rice2=0, esc_every=0):
    """parts for residuals already in sub['res']: per partition the smallest k that keeps every
    quotient below 8, every esc_every-th partition escaped at its exact width"""
    counts = partition_counts(blocksize, sub["order"], porder)
    parts, i = [], 0
    for p, cnt in enumerate(counts):
        rs = sub["res"][i:i + cnt]
        i += cnt
        if esc_every and p % esc_every == esc_every - 1:
            parts.append((0, max((r.bit_length() + 1 for r in rs if r), default=0)))
        else:
            m = max((zigzag(r) for r in rs), default=0)
            parts.append((min(max(m.bit_length() - 3, 0), 30 if rice2 else 14), None))
    sub.update(rice2=rice2, porder=porder, parts=parts)


def _group_c(T, rng):
    big = 0
    for carrier, (channels, bps, maxo, _) in CARRIERS.items():
        cap = sample_cap(carrier)
        n = 0
        # order 0
        subs = default_subs(rng, carrier)
        bs = layout(rng, max(s["order"] for s in subs), 0)
        for s in subs:
            warm_for(rng, s, cap)
            fill_parts(rng, s, bs, 0, [6], cap, n & 1)
        T.put(f"C/{carrier}/porder0", "C", carrier, subs, bs, n)
        n += 1
        # one sample per partition: FIXED-0 where the class allows it, else order 1 (partition 0 empty)
        if carrier != "W32":
            for bs, porder in ((16, 4), (4096, 12)):
                if bs >= 4096 and carrier == "T24":
                    continue
                subs = []
                for ch in range(channels):
                    first = ch == 0 and carrier in ("S16", "M16")
                    s = fixed_sub(0) if first else lpc_sub(rng, 1, 12, 11) if ch < 2 else fixed_sub(1)
                    encode_residual(s, _signal(rng, bs, 1 << (cap - 3), 40))
                    code_partitions(rng, s, bs, porder, rice2=ch & 1, esc_every=5)
                    subs.append(s)
                T.put(f"C/{carrier}/bs{bs}_porder{porder}", "C", carrier, subs, bs, n)
                n += 1
                big += bs >= 4096
        # partition 0 empty: order == blocksize >> porder
        for order, bs, porder in ((1, 32, 5), (4, 64, 4), (8, 64, 3), (12, 96, 3), (20, 160, 3)):
            legal = order <= maxo and (order >= 17) == (carrier == "W32")
            if not legal:
                continue
            subs = default_subs(rng, carrier)
            subs[0] = lpc_sub(rng, order, 12, 11) if bps == 16 else lpc_sub(rng, order, 14, 13)
            if len(subs) > 1 and subs[1]["order"] > order:
                subs[1] = lpc_sub(rng, 1, 5, 4)
            for s in subs:
                warm_for(rng, s, cap)
                fill_parts(rng, s, bs, porder, [rng.choice((0, 2, 5, ("esc", 7))) for _ in range(1 << porder)], cap, n & 1)
            T.put(f"C/{carrier}/empty_first_order{order}_porder{porder}", "C", carrier, subs, bs, n)
            n += 1
    # partition order 15: 32767 one-sample partitions behind an empty one
    for carrier, types in (("M16", ["fixed"]), ("S16", ["fixed", "lpc"])):
        subs = []
        for t in types:
            s = fixed_sub(1) if t == "fixed" else lpc_sub(rng, 1, 12, 11)
            encode_residual(s, _signal(rng, 32768, 4000, 40))
            code_partitions(rng, s, 32768, 15, rice2=len(subs), esc_every=7)
            subs.append(s)
        T.put(f"C/{carrier}/bs32768_porder15", "C", carrier, subs, 32768, 3)
        big += 1
    assert big <= 6, big


def lpc_frame(T, rng, name, group, carrier, spec, idx, *, ch=0, assignment=None, small=False, expect="restore",
              full_coef=False):
    """A carrier frame whose channel ch holds the LPC subframe spec = (order, prec, shift, wasted);
    the other channels keep the carrier's usual predictors."""
    order, prec, shift, wasted = spec
    channels, bps = CARRIERS[carrier][:2]
    subs = default_subs(rng, carrier)
    s = lpc_sub(rng, order, prec, shift, wasted)
    if full_coef:
        s["coef"] = [rng.randint(-(1 << (prec - 1)), (1 << (prec - 1)) - 1) for _ in range(order)]
    subs[ch] = s
    for o in subs:  # a class of its own (orders above 8 / 12 / 16) is the row's, not the neighbours'
        if o is not s and o["type"] == "lpc" and o["order"] > order:
            o.update(lpc_sub(rng, min(order, 2), 5, 4))
    porder = rng.choice((0, 1, 2))
    bs = layout(rng, max(x["order"] for x in subs), porder)
    for x in subs:
        cap = sample_cap(carrier, x.get("wasted", 0))
        warm_for(rng, x, cap, small=small and x is s)
        fill_parts(rng, x, bs, porder, [rng.choice((1, 3, 4)) if small and x is s else rng.choice((5, 7, 8))
                                       for _ in range(1 << porder)], 6 if small and x is s else cap, idx & 1)
    # independent unless the row says otherwise: a side channel's extra bit would change the path
    T.put(name, group, carrier, subs, bs, idx, expect=expect, assignment=channels - 1 if assignment is None else assignment)


D_SPECS = {  # carrier: [(description, (order, prec, shift, wasted), options)]
    "S16": [("prec1", (2, 1, 1, 0), {}), ("prec2", (2, 2, 1, 0), {}), ("prec15", (2, 15, 14, 0), {}),
            ("shift0", (4, 4, 0, 0), {"small": True}), ("shift15", (2, 15, 15, 0), {}),
            ("order1", (1, 12, 11, 0), {}), ("order3", (3, 12, 11, 0), {}), ("order4", (4, 12, 11, 0), {}),
            ("order8", (8, 12, 11, 0), {}),
            ("path_mmx16", (8, 12, 11, 0), {}), ("path_ia32", (3, 12, 11, 0), {}), ("path_wide", (8, 15, 14, 0), {}),
            ("sum32_side17_order1", (1, 15, 14, 0), {"ch": 1, "assignment": LEFT_SIDE}),
            ("sum33_side17_order2", (2, 15, 14, 0), {"ch": 1, "assignment": LEFT_SIDE}),
            ("sum32_order8_prec13", (8, 13, 12, 0), {}), ("sum33_order8_prec14", (8, 14, 13, 0), {})],
    "S24": [("prec1", (12, 1, 1, 0), {}), ("prec2", (12, 2, 1, 0), {}), ("prec15", (12, 15, 14, 0), {}),
            ("shift0", (4, 4, 0, 0), {"small": True}), ("shift15", (12, 15, 15, 0), {}),
            ("order1", (1, 14, 13, 0), {}), ("order3", (3, 14, 13, 0), {}), ("order4", (4, 14, 13, 0), {}),
            ("order8", (8, 14, 13, 0), {}), ("order9", (9, 14, 13, 0), {}), ("order12", (12, 14, 13, 0), {}),
            ("path_wide", (8, 14, 13, 0), {}), ("path_ia32", (4, 5, 4, 0), {}), ("path_mmx16", (4, 10, 9, 8), {}),
            ("sum32_order1_prec8", (1, 8, 7, 0), {}), ("sum33_order1_prec9", (1, 9, 8, 0), {})],
    "M16": [("prec1", (6, 1, 1, 0), {}), ("prec2", (6, 2, 1, 0), {}), ("prec15", (6, 15, 14, 0), {}),
            ("shift0", (4, 4, 0, 0), {"small": True}), ("shift15", (6, 15, 15, 0), {}),
            ("order1", (1, 12, 11, 0), {}), ("order3", (3, 12, 11, 0), {}), ("order4", (4, 12, 11, 0), {}),
            ("order8", (8, 12, 11, 0), {}),
            ("path_mmx16", (6, 12, 11, 0), {}), ("path_ia32", (2, 12, 11, 0), {}), ("path_wide", (8, 15, 14, 0), {}),
            ("sum32_order4_prec14", (4, 14, 13, 0), {}), ("sum33_order4_prec15", (4, 15, 14, 0), {})],
    "T24": [("prec1", (12, 1, 1, 0), {}), ("prec2", (12, 2, 1, 0), {}), ("prec15", (12, 15, 14, 0), {}),
            ("shift0", (4, 4, 0, 0), {"small": True}), ("shift15", (12, 15, 15, 0), {}),
            ("order1", (1, 14, 13, 0), {}), ("order3", (3, 14, 13, 0), {}), ("order4", (4, 14, 13, 0), {}),
            ("order8", (8, 14, 13, 0), {}), ("order9", (9, 14, 13, 0), {}), ("order12", (12, 14, 13, 0), {}),
            ("order13", (13, 14, 13, 0), {}), ("order16", (16, 14, 13, 0), {}),
            ("path_wide", (12, 14, 13, 0), {}), ("path_ia32", (3, 6, 5, 0), {}), ("path_mmx16", (4, 10, 9, 8), {}),
            ("sum32_order2_prec7", (2, 7, 6, 0), {}), ("sum33_order2_prec8", (2, 8, 7, 0), {})],
    "W32": [("prec1", (20, 1, 1, 0), {}), ("prec2", (20, 2, 1, 0), {}), ("prec15", (20, 15, 14, 0), {}),
            ("shift0", (17, 4, 0, 0), {"small": True}), ("shift15", (20, 15, 15, 0), {}),
            ("order17", (17, 12, 11, 0), {}), ("order32", (32, 12, 11, 0), {}),
            ("path_mmx16", (20, 12, 11, 0), {}), ("path_wide", (20, 13, 12, 0), {}),
            ("sum32_order20_prec12", (20, 12, 11, 0), {}), ("sum33_order20_prec13", (20, 13, 12, 0), {})],
}


def _group_d(T, rng):
    for carrier, specs in D_SPECS.items():
        for n, (desc, spec, opt) in enumerate(specs):
            lpc_frame(T, rng, f"D/{carrier}/{desc}", "D", carrier, spec, n, **opt)
    # the 64-bit path with a true sum beyond 2^31: a 17-bit side channel near +-64000, coefficients
    # near +-16383, shift 15 (a 32-bit accumulator gives another answer)
    for order in (4, 8):
        bs = 96
        c = [16383 if j % 2 == 0 else -16381 for j in range(order)]
        side = [(64000 - 37 * n) * (1 if n % 2 == 0 else -1) for n in range(bs)]
        s = {"type": "lpc", "order": order, "prec": 15, "shift": 15, "coef": c, "wasted": 0}
        encode_residual(s, side)
        assert any(abs(predict(s, side, n)[0]) >= 1 << 31 for n in range(order, bs))
        code_partitions(rng, s, bs, 2, rice2=0, esc_every=2)
        left = lpc_sub(rng, 2, 10, 9)
        encode_residual(left, [32000 * (1 if n % 2 == 0 else -1) + rng.randint(-60, 60) for n in range(bs)])
        code_partitions(rng, left, bs, 2)
        T.add(f"D/S16/wide_sum_beyond_2^31_order{order}", "D", "S16", [left, s], bs, 16, assignment=LEFT_SIDE)


E_SPECS = {  # carrier: [(path, (order, prec, wasted))]
    "S16": [("mmx16", (8, 12, 0)), ("ia32", (3, 12, 0)), ("wide", (8, 15, 0))],
    "S24": [("wide", (12, 14, 0)), ("ia32", (4, 5, 0)), ("ia32_order1", (1, 8, 0)), ("ia32_order3", (3, 7, 0)),
            ("ia32_order8", (8, 5, 0)), ("mmx16", (4, 10, 8))],
    "M16": [("mmx16", (6, 12, 0)), ("ia32", (2, 12, 0)), ("wide", (8, 15, 0))],
    "T24": [("wide", (12, 14, 0)), ("ia32", (3, 6, 0)), ("mmx16", (4, 10, 8))],
    "W32": [("mmx16", (20, 12, 0)), ("wide", (20, 13, 0))],
}


def _group_e(T, rng):
    for carrier, specs in E_SPECS.items():
        n = 0
        for path, (order, prec, wasted) in specs:
            for shift in (-1, -3, -16):
                # full-range coefficients: a 32-bit sum >> (shift & 31) is then more than a sign
                lpc_frame(T, rng, f"E/{carrier}/{path}_shift{shift}", "E", carrier, (order, prec, shift, wasted), n,
                          assignment=CARRIERS[carrier][0] - 1, expect="oracle", full_coef=True)
                n += 1


def _from_signal(rng, sub, signal, bs, porder=1, rice2=0, esc_every=0):
    encode_residual(sub, signal)
    code_partitions(rng, sub, bs, porder, rice2, esc_every)
    return sub


def _group_f(T, rng):
    for carrier, (channels, bps, maxo, _) in CARRIERS.items():
        n = 0
        bs = 80
        # a 1-bit subframe (wasted = bps - 1) in channel 0, as VERBATIM, FIXED and LPC
        for t in ("verbatim", "fixed", "lpc"):
            one = [rng.choice((-1, 0)) for _ in range(bs)]
            w = bps - 1
            if t == "verbatim":
                s = {"type": "verbatim", "wasted": w, "samples": one}
            elif t == "fixed":
                s = _from_signal(rng, fixed_sub(2, w), one, bs)
            else:  # orders below 4 stay off the MMX16 path, which k_decode_sw declines
                o = 17 if carrier == "W32" else 2
                s = _from_signal(rng, lpc_sub(rng, o, 2, 1, w), one, bs)
            subs = default_subs(rng, carrier)
            subs[0] = s
            if carrier == "W32" and t != "lpc":  # the class needs an order above 16 somewhere: mono has one subframe
                DROPPED.append((f"F/{carrier}/wasted{w}_{t}", "a mono frame of order 17..32 holds one LPC subframe"))
                continue
            for x in subs[1:]:
                warm_for(rng, x, sample_cap(carrier))
                fill_parts(rng, x, bs, 1, [6, 7], sample_cap(carrier), 0)
            T.put(f"F/{carrier}/wasted{w}_{t}", "F", carrier, subs, bs, n, assignment=channels - 1)
            n += 1
        if channels != 2:
            continue
        # wasted bits on one channel only, under each assignment
        for a in (1, LEFT_SIDE, RIGHT_SIDE, MID_SIDE):
            for ch in (0, 1):
                w = rng.randint(1, 5)
                subs = default_subs(rng, carrier)
                subs[ch]["wasted"] = w
                for i, x in enumerate(subs):
                    cap = sample_cap(carrier, x.get("wasted", 0)) - 1
                    warm_for(rng, x, cap)
                    fill_parts(rng, x, bs, 2, [5, 6, 4, 7], cap, i)
                T.add(f"F/{carrier}/wasted{w}_ch{ch}_{ASSIGN_NAME.get(a, 'indep')}", "F", carrier, subs, bs, bps,
                      assignment=a)
        # the side channel with all but one of its bits wasted
        subs = default_subs(rng, carrier)
        # (one bit of 2^bps: L - R stays inside the sample range only when that bit is 0)
        subs[1] = _from_signal(rng, lpc_sub(rng, 2, 2, 1, bps), [0] * bs, bs)
        warm_for(rng, subs[0], bps - 2)
        fill_parts(rng, subs[0], bs, 1, [6, 7], bps - 2, 0)
        T.add(f"F/{carrier}/wasted{bps}_side{bps + 1}", "F", carrier, subs, bs, bps, assignment=LEFT_SIDE)
        # mid/side with odd negative sums
        left = [-(2 * rng.randint(0, 3000)) - 1 - (i & 1) for i in range(bs)]
        right = [-(2 * rng.randint(0, 3000)) - (i & 1) for i in range(bs)]
        assert all((l + r) & 1 and l + r < 0 for l, r in zip(left, right))
        mid = [(l + r) >> 1 for l, r in zip(left, right)]
        side = [l - r for l, r in zip(left, right)]
        subs = default_subs(rng, carrier)
        _from_signal(rng, subs[0], mid, bs, 2)
        _from_signal(rng, subs[1], side, bs, 2, 1)
        T.add(f"F/{carrier}/mid_side_odd_negative", "F", carrier, subs, bs, bps, assignment=MID_SIDE)
        assert T.rows[-1].pcm == [left, right]
    # L / R alternating between +full scale and -full scale
    for bps in (8, 12, 16, 20, 24):
        carrier = "S16" if bps <= 16 else "S24"
        hi, lo = (1 << (bps - 1)) - 1, -(1 << (bps - 1))
        bs = 48
        left = [hi if i % 2 == 0 else lo for i in range(bs)]
        right = [lo if i % 2 == 0 else hi for i in range(bs)]
        for a in (LEFT_SIDE, RIGHT_SIDE, MID_SIDE):
            side = [l - r for l, r in zip(left, right)]
            mid = [(l + r) >> 1 for l, r in zip(left, right)]
            c0, c1 = {LEFT_SIDE: (left, side), RIGHT_SIDE: (side, right), MID_SIDE: (mid, side)}[a]
            s0 = _from_signal(rng, fixed_sub(0), c0, bs, 1, 1)
            s1 = _from_signal(rng, {"type": "lpc", "order": 2, "prec": 4, "shift": 2, "coef": [-4, 0], "wasted": 0}, c1, bs, 2)
            T.add(f"F/{carrier}/full_scale_{bps}bit_{ASSIGN_NAME[a]}", "F", carrier, [s0, s1], bs, bps, assignment=a)
            assert T.rows[-1].pcm == [left, right]


def _const(value=0):
    return {"type": "constant", "value": value}


def _verb(rng, n, bits):
    return {"type": "verbatim", "samples": [rng.randint(-(1 << (bits - 1)), (1 << (bits - 1)) - 1) for _ in range(n)]}


def _group_g(T, rng):
    def tiny(bs):
        return [_verb(rng, bs, 16)] if bs <= 17 else [_const(rng.randint(-30000, 30000))]

    for code in range(1, 16):
        if code in (6, 7):
            continue  # the two forms below
        bs = BS_OF_CODE[code]
        T.add(f"G/bs_code{code}", "G", None, tiny(bs), bs, 16, bs_code=code, hdr={"blocksize": bs})
    for bs in (1, 2, 15, 17, 255, 256):
        T.add(f"G/bs8_{bs}", "G", None, tiny(bs), bs, 16, bs_code=6, hdr={"blocksize": bs})
    for bs in (1, 2, 15, 17, 255, 256, 257, 65535):
        T.add(f"G/bs16_{bs}", "G", None, tiny(bs), bs, 16, bs_code=7, hdr={"blocksize": bs})
    for code in range(1, 12):
        T.add(f"G/sr_code{code}", "G", None, tiny(16), 16, 16, sr_code=code, hdr={"sample_rate": SR_OF_CODE[code]})
    for code, mul, extras in ((12, 1000, (0, 255)), (13, 1, (0, 255, 65535)), (14, 10, (0, 255, 65535))):
        for x in extras:
            T.add(f"G/sr_code{code}_{x}", "G", None, tiny(16), 16, 16, sr_code=code, sr_extra=x,
                  hdr={"sample_rate": x * mul})
    T.add("G/sr_code0_streaminfo", "G", None, tiny(16), 16, 16, sr_code=0, hdr={"sample_rate": SI_RATE})
    T.add("G/sr_code0_no_streaminfo", "G", None, tiny(16), 16, 16, sr_code=0, si=False, expect="oracle")
    for a in (1, LEFT_SIDE, RIGHT_SIDE, MID_SIDE):
        subs = [_verb(rng, 16, 14), _verb(rng, 16, 14)]
        T.add(f"G/bps_code0_streaminfo_{ASSIGN_NAME.get(a, 'indep')}", "G", None, subs, 16, 16, bps_code=0, assignment=a,
              hdr={"bps": 16})
    T.add("G/bps_code0_no_streaminfo", "G", None, [_verb(rng, 16, 14), _verb(rng, 16, 14)], 16, 16, bps_code=0,
          si=False, expect="oracle")
    for a in (1, LEFT_SIDE, RIGHT_SIDE, MID_SIDE):
        subs = [_verb(rng, 16, 14), _verb(rng, 16, 14)]
        T.add(f"G/no_streaminfo_{ASSIGN_NAME.get(a, 'indep')}", "G", None, subs, 16, 16, assignment=a, si=False)
    fixed = [0, 127, 128, 2047, 2048, 65535, 65536, (1 << 21) - 1, 1 << 21, (1 << 26) - 1, 1 << 26, (1 << 31) - 1]
    for v in fixed:
        T.add(f"G/frame_number_{v}", "G", None, tiny(16), 16, 16, number=v, hdr={"number": v, "number_type": 0})
    for v in fixed + [1 << 31, (1 << 36) - 1]:
        T.add(f"G/sample_number_{v}", "G", None, tiny(16), 16, 16, number=v, variable=True,
              hdr={"number": v, "number_type": 1})
    for nb in (2, 7):
        T.add(f"G/number_0_in_{nb}_bytes", "G", None, tiny(16), 16, 16, number=0, number_bytes=nb, variable=nb == 7,
              hdr={"number": 0, "number_type": int(nb == 7)})


def _group_h(T, rng):
    """Frames a field of which libFLAC refuses, or takes although RFC 9639 forbids it.  Whole
    frames with good CRCs; the field under test sits in the frame header or in a subframe header.
    Subframe rows come as a stereo frame with the field in channel 0 (k_parse walks that subframe)
    and as a mono frame (the decode kernels meet it)."""
    def coded(order=2, bs=32, porder=1, **over):
        s = lpc_sub(rng, order, 8, 7)
        s["warm"] = [rng.randint(-50, 50) for _ in range(order)]
        counts = partition_counts(bs, order, porder)
        s.update(rice2=0, porder=porder, parts=[(3, None)] * len(counts),
                 res=[rng.randint(-9, 9) for _ in range(sum(counts))])
        s.update(over)
        return s

    def good(bs):
        return {"type": "verbatim", "samples": [rng.randint(-99, 99) for _ in range(bs)]}

    def sub_rows(desc, sub_of, bs=32):
        T.add(f"H/{desc}_ch0_of_2", "H", None, [sub_of(), good(bs)], bs, 16, expect="oracle")
        T.add(f"H/{desc}_mono", "H", None, [sub_of()], bs, 16, expect="oracle")

    for code in (2, 7, 13, 31):
        sub_rows(f"subframe_type{code}", lambda: dict(good(32), type_code=code))
    sub_rows("precision_code15", lambda: coded(prec_code=15))
    for m in (2, 3):
        sub_rows(f"coding_method{m}", lambda: coded(method=m))
    sub_rows("partition_shorter_than_order", lambda: coded(order=8, bs=32, porder=3))
    sub_rows("blocksize_below_order", lambda: coded(order=8, bs=4, porder=0), bs=4)
    sub_rows("partitions_do_not_divide_blocksize", lambda: coded(order=2, bs=100, porder=3), bs=100)
    sub_rows("first_bit_set", lambda: dict(_const(5), first_bit=1))
    sub_rows("wasted_equals_bps", lambda: dict(_const(0), wasted=16))
    sub_rows("wasted_is_bps_plus_1", lambda: dict(_const(0), wasted=17))
    hdr = [_const(77)]
    for a in range(11, 16):
        T.add(f"H/assignment{a}", "H", None, [_const(1), _const(2)], 16, 16, assignment=a, expect="oracle")
    for code in (3, 7):
        T.add(f"H/bps_code{code}", "H", None, hdr, 16, 16, bps_code=code, expect="oracle")
    T.add("H/sr_code15", "H", None, hdr, 16, 16, sr_code=15, expect="oracle")
    T.add("H/bs_code0", "H", None, hdr, 16, 16, bs_code=0, expect="oracle")
    T.add("H/blocksize_65536", "H", None, hdr, 65536, 16, bs_code=7, expect="oracle")
    T.add("H/reserved_bit_byte1", "H", None, hdr, 16, 16, reserved1=1, expect="oracle")
    T.add("H/reserved_bit_byte3", "H", None, hdr, 16, 16, reserved2=1, expect="oracle")
    T.add("H/padding_not_zero", "H", None, [dict(_verb(rng, 3, 15), wasted=1)], 3, 16, pad_bits=1, expect="oracle")
    T.add("H/header_byte2_ff", "H", None, hdr, 32768, 16, bs_code=15, sr_code=15, expect="oracle")
    T.add("H/header_byte3_ff", "H", None, [_const(1), _const(2)], 16, 16, assignment=15, bps_code=7, reserved2=1,
          expect="oracle")
    T.add("H/number_bad_continuation", "H", None, hdr, 16, 16, number_raw=b"\xc2\x41", expect="oracle")
    T.add("H/number_lead_byte_ff", "H", None, hdr, 16, 16, number_raw=b"\xff", expect="oracle")
    T.add("H/number_7_bytes_fixed_blocksize", "H", None, hdr, 16, 16, number_raw=utf8(1 << 31, 7), expect="oracle")


_ROWS = None


def rows():
    """The table, built once: the same rows in the same order on every call (random.Random(seed))."""
    global _ROWS
    if _ROWS is None:
        del DROPPED[:]
        T = _Table()
        for seed, build in enumerate((_group_a, _group_b, _group_c, _group_d, _group_e, _group_f, _group_g, _group_h)):
            build(T, random.Random(9639 + seed))
        _ROWS = T.rows
    return _ROWS


def groups(table=None):
    """{(channels, bps, with STREAMINFO): [rows]} in table order: one decode call each"""
    out = {}
    for r in table if table is not None else rows():
        out.setdefault((r.channels, r.bps, r.si), []).append(r)
    return out
