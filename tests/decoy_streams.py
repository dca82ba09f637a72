"""Streams with decoy frame starts: sync codes inside payloads, metadata and junk that look like
frame headers, some of them placed so that the CRC-16 from the carrying frame's start closes at
them (tests/test_decoy_streams_host.py certifies the table, tests/test_gpu_index_decoys.py runs it).

Built on tests/flac_frames.py alone: its frame writer, CRCs and exact reference.  Nothing here
comes from the product.  Carriers are VERBATIM subframes without wasted bits, so a payload byte
offset is a stream byte offset and a decoy is a byte string put into a channel's samples:

    S16   2 channels, 16 bits, blocksize 256     a frame is 1,034 bytes (the main carrier)
    M24   1 channel,  24 bits, blocksize 192     every decoy lies in the last subframe
    O16   8 channels, 16 bits, blocksize 256     the decoy lies in channel 3
    W16   2 channels, 16 bits, blocksize 32768   the `window` rows: a payload of FF F8 pairs

Payload bytes are random below 0xF0, so a carrier holds no sync pair but the frame starts and the
decoys.  A decoy is "tuned" by the 16 bits in front of it: CRC-16 is linear and its register is 16
bits wide, so writing the register's value there zeroes it, and the CRC-16 from the frame start
closes at the decoy (tune() asserts it rather than trusting the algebra).

A decoy's class says how far it gets as a frame start (DECOY_CLASSES below).  Every row gives the
stream bytes, the true frame offsets, the true PCM, each decoy's offset and its class.
"""
import random
from types import SimpleNamespace

import numpy as np

from tests.flac_frames import crc16, frame, frame_pcm, stream

CARRIERS = {"S16": (2, 16, 256), "M24": (1, 24, 192), "O16": (8, 16, 256), "W16": (2, 16, 32768)}
CHAIN_WIN = 1 << 16  # candidates the indexer looks at past a frame start for its successor

# class: does the candidate parse as a frame start (header, CRC-8, subframe walk inside the stream)
DECOY_CLASSES = {"pair": False, "crc8": False, "walk": False, "trunc": False, "valid": True, "close-early": True,
                 "close-last": True, "nested": True, "nested-n": True, "meta": True, "tail": True, "straddle": False,
                 "gapdecoy": False, "window": False}
# Rows whose frame list libFLAC and the CRC-16 algebra cannot agree on cheaply: the indexers may
# answer with a stated refusal or limit instead ("Decoys").
LIMIT_KINDS = ("window-over", "close-last", "nested", "tail-total0")


def sync_pairs(data):
    """byte offsets of every byte-aligned sync pair (FF, then 111110xx)"""
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    return np.flatnonzero((a[:-1] == 0xFF) & ((a[1:] >> 2) == 0x3E))


# ------------------------------------------------------------------ decoy byte strings
def _const(n):
    return [{"type": "constant", "value": 0}] * n


def header(channels, blocksize, bps, number, **kw):
    """The frame header alone (through its CRC-8) that frame() writes for these fields"""
    f = frame(_const(channels), blocksize, bps, number=number, **kw)
    body = channels * (1 + bps // 8)  # a CONSTANT subframe: one header byte and one sample
    assert (channels * (8 + bps)) % 8 == 0
    return f[: len(f) - body - 2]


SUB_VERBATIM, SUB_RESERVED = b"\x02", b"\x04"  # subframe header bytes: type 000001; type 000010 (reserved)
NESTED_BS = 64
NESTED_LEN = 7 + 1 + NESTED_BS * 2 + 2  # a mono 16-bit VERBATIM frame of 64 samples: 138 bytes


def decoy_bytes(cls, number, blocksize=NESTED_BS):
    """What is written at the decoy's offset, for the classes that live inside a payload.
    blocksize: what a valid decoy's header claims (the stream's own makes it a better resume point)"""
    if cls == "pair":  # the reserved bit of byte 3 set; the CRC-8 is right for these bytes
        return header(1, NESTED_BS, 16, number, reserved2=1)
    if cls == "crc8":
        h = header(1, NESTED_BS, 16, number)
        return h[:-1] + bytes([h[-1] ^ 0x5A])
    if cls == "walk":  # stereo: the walk has to pass subframe 0, whose type is reserved
        return header(2, NESTED_BS, 16, number) + SUB_RESERVED
    if cls == "trunc":  # stereo, blocksize 32768: subframe 0 alone is 64 KiB, past any row's end
        return header(2, 32768, 16, number) + SUB_VERBATIM
    # valid, close-early, close-last, nested, nested-n: a mono header and its subframe's header byte
    return header(1, blocksize, 16, number) + SUB_VERBATIM


def tune(buf, at):
    """Set buf[at - 2: at] so that crc16(buf[:at]) == 0"""
    buf[at - 2: at] = crc16(bytes(buf[: at - 2])).to_bytes(2, "big")
    assert crc16(bytes(buf[:at])) == 0


# ------------------------------------------------------------------ carrier frames
def _layout(carrier, number):
    channels, bps, bs = CARRIERS[carrier]
    hlen = len(header(channels, bs, bps, number))
    plen = bs * bps // 8
    starts = [hlen + c * (1 + plen) + 1 for c in range(channels)]  # first payload byte of each channel
    return channels, bps, bs, hlen, plen, starts, hlen + channels * (1 + plen) + 2


def _subs_of(buf, carrier, number):
    channels, bps, bs, hlen, plen, starts, flen = _layout(carrier, number)
    nb = bps // 8
    subs = []
    for c in range(channels):
        raw = bytes(buf[starts[c]: starts[c] + plen])
        subs.append({"type": "verbatim",
                     "samples": [int.from_bytes(raw[i: i + nb], "big", signed=True) for i in range(0, plen, nb)]})
    return subs


def carrier_frame(rng, carrier, number, decoys=(), fill=None):
    """One carrier frame.  decoys: [(channel, byte offset inside that channel's payload, or a negative
    offset from the frame's end, bytes, tuned)].  fill: the payload byte pattern (default: random
    bytes below 0xF0).  -> (frame bytes, subframes, [decoy offsets inside the frame])"""
    channels, bps, bs, hlen, plen, starts, flen = _layout(carrier, number)
    buf = bytearray(frame(_const(channels), bs, bps, number=number)[:hlen])
    for c in range(channels):
        buf += SUB_VERBATIM
        buf += (fill * (plen // len(fill) + 1))[:plen] if fill else bytes(rng.randrange(0xF0) for _ in range(plen))
    buf += b"\0\0"
    assert len(buf) == flen
    at = []
    for c, off, blob, tuned in sorted(decoys, key=lambda d: starts[d[0]] + d[1] if d[1] >= 0 else flen + d[1]):
        p = starts[c] + off if off >= 0 else flen + off
        assert starts[c] + (2 if tuned else 0) <= p and p + len(blob) <= starts[c] + plen, "decoy outside its channel"
        buf[p: p + len(blob)] = blob
        if tuned:  # in offset order: a later tuning never changes an earlier prefix
            tune(buf, p)
        at.append(p)
    subs = _subs_of(buf, carrier, number)
    data = frame(subs, bs, bps, number=number)
    assert data[:-2] == bytes(buf[:-2]), "the writer and the byte layout disagree"
    return data, subs, at


def _plain(rng, carrier, number):
    return carrier_frame(rng, carrier, number)[:2]


def with_block(data, block_type, body):
    """The stream with one more metadata block (PADDING 1, APPLICATION 2) behind STREAMINFO, as the
    last block: libFLAC skips both by their length"""
    assert data[:4] == b"fLaC" and data[4] == 0x80 and len(body) < 1 << 24
    return data[:4] + b"\x00" + data[5:42] + bytes([0x80 | block_type]) + len(body).to_bytes(3, "big") + body + data[42:]


def first_frame_offset(data):
    p = 4
    while True:
        last = data[p] & 0x80
        p += 4 + int.from_bytes(data[p + 1: p + 4], "big")
        if last:
            return p


# ------------------------------------------------------------------ the table
class _Rows:
    def __init__(self):
        self.rows = []

    def add(self, name, carrier, frames, decoys, *, total=None, block=None, tail=b"", kind=None):
        """frames: [(bytes, subs)]; decoys: [(frame index | 'meta' | 'tail', offset inside it, class, dict)]"""
        channels, bps, bs = CARRIERS[carrier]
        pcm = [frame_pcm(s, bs, bps) for _, s in frames]
        data = stream([f for f, _ in frames], pcm, channels=channels, bps=bps, total=total)
        if block is not None:
            data = with_block(data, *block)
        first = first_frame_offset(data)
        offs, p = [], first
        for f, _ in frames:
            offs.append(p)
            p += len(f)
        data += tail
        out = []
        for where, off, cls, info in decoys:
            base = first - len(block[1]) if where == "meta" else p if where == "tail" else offs[where]
            out.append(SimpleNamespace(offset=base + off, cls=cls, frame=where, valid=DECOY_CLASSES[cls], **info))
        assert name not in [r.name for r in self.rows]
        self.rows.append(SimpleNamespace(
            name=name, carrier=carrier, data=data, channels=channels, bps=bps, blocksize=bs, frame_offsets=offs,
            frame_ends=[o + len(f) for o, (f, _) in zip(offs, frames)], pcm=pcm, decoys=out, first=first,
            total=sum(len(c[0]) for c in pcm) if total is None else total, kind=kind or decoys[0][2],
            limit=(kind or decoys[0][2]) in LIMIT_KINDS))
        return self.rows[-1]


def _payload_rows(T, rng):
    """decoys inside a frame's payload"""
    def row(name, carrier, nframes, k, chan, off, cls, number, tuned, claims=NESTED_BS, **kw):
        fr = []
        for n in range(nframes):
            if n == k:
                f, s, at = carrier_frame(rng, carrier, n, [(chan, off, decoy_bytes(cls, number, claims), tuned)])
                fr.append((f, s))
            else:
                fr.append(_plain(rng, carrier, n))
        last_sub = _layout(carrier, k)[5][-1] - 1  # the last subframe's header byte
        assert (at[0] < last_sub) == (chan < CARRIERS[carrier][0] - 1)
        return T.add(name, carrier, fr, [(k, at[0], cls, dict(number=number, tuned=tuned, chan=chan))], **kw)

    # S16, 3..6 frames; the carrier is never the first frame where a damage variant needs one before it
    row("S16/pair", "S16", 4, 1, 0, 100, "pair", 2, False)
    row("S16/crc8", "S16", 4, 1, 1, 40, "crc8", 2, False)
    row("S16/walk", "S16", 5, 2, 0, 200, "walk", 3, False)
    row("S16/trunc", "S16", 3, 2, 1, 300, "trunc", 3, False)  # the last frame
    row("S16/valid_ch0", "S16", 4, 1, 0, 61, "valid", 2, False)
    row("S16/valid_ch1", "S16", 4, 1, 1, 300, "valid", 2, False)
    # the issue's "early" stream: frame 0, channel 0, one tuning sample, then the header (frame byte 9);
    # the number continues, so only the position tells it from a successor
    row("S16/close-early_frame0", "S16", 3, 0, 0, 2, "close-early", 1, True)
    row("S16/close-early_next", "S16", 5, 2, 0, 82, "close-early", 3, True)
    row("S16/close-early_other", "S16", 5, 2, 0, 301, "close-early", 77, True)
    row("S16/close-early_end_of_ch0", "S16", 4, 1, 0, 512 - 8, "close-early", 2, True)
    # in the last subframe the position is legitimate; the number decides where it can
    row("S16/close-last_other", "S16", 5, 2, 1, 100, "close-last", 90, True, kind="nested-n")
    row("S16/close-last_next", "S16", 5, 2, 1, 100, "close-last", 3, True)
    # headers that claim the stream's own blocksize and the next frame's number: all that the resync
    # rule asks of a place to resume at, but a successor
    row("S16/close-early_claims_B", "S16", 5, 2, 0, 150, "close-early", 3, True, claims=256)
    row("S16/close-last_claims_B_other", "S16", 5, 2, 1, 222, "close-last", 90, True, claims=256, kind="nested-n")
    row("S16/valid_claims_B", "S16", 5, 2, 1, 400, "valid", 3, False, claims=256)
    row("S16/nested_next", "S16", 5, 2, 1, -NESTED_LEN, "nested", 3, True)
    row("S16/nested_frame0", "S16", 3, 0, 1, -NESTED_LEN, "nested", 1, True)
    row("S16/nested-n", "S16", 5, 2, 1, -NESTED_LEN, "nested-n", 40, True)
    row("S16/nested-n_previous", "S16", 6, 3, 1, -NESTED_LEN, "nested-n", 2, True)
    # M24: one channel, so every decoy lies in the last subframe and the walk has nothing to pass
    row("M24/pair", "M24", 4, 1, 0, 50, "pair", 2, False)
    row("M24/crc8", "M24", 4, 1, 0, 51, "crc8", 2, False)
    row("M24/valid", "M24", 5, 2, 0, 200, "valid", 3, False)
    row("M24/nested-n", "M24", 4, 1, 0, -NESTED_LEN, "nested-n", 9, True)
    row("M24/nested_next", "M24", 4, 1, 0, -NESTED_LEN, "nested", 2, True)
    # O16: channel 3 of 8 is not the last subframe
    row("O16/crc8", "O16", 4, 1, 3, 33, "crc8", 2, False)
    row("O16/valid", "O16", 4, 1, 3, 34, "valid", 2, False)
    row("O16/close-early_next", "O16", 4, 1, 3, 100, "close-early", 2, True)
    row("O16/close-early_ch6", "O16", 3, 0, 6, 501, "close-early", 1, True)
    row("O16/nested-n", "O16", 4, 1, 7, -NESTED_LEN, "nested-n", 70, True)


def _nested_frame(rng, number):
    """a complete mono 16-bit VERBATIM frame of NESTED_BS samples"""
    sub = {"type": "verbatim", "samples": [rng.randrange(3000) for _ in range(NESTED_BS)]}
    f = frame([sub], NESTED_BS, 16, number=number)
    assert len(f) == NESTED_LEN and len(sync_pairs(f)) == 1
    return f


def _outside_rows(T, rng):
    """decoys in a metadata block and behind the last frame"""
    for block_type, label in ((1, "padding"), (2, "application")):
        d = _nested_frame(rng, 0)
        body = (b"bnfl" if block_type == 2 else b"") + bytes(37) + d  # ends exactly at the first frame
        fr = [_plain(rng, "S16", n) for n in range(3)]
        T.add(f"S16/meta_{label}", "S16", fr, [("meta", len(body) - len(d), "meta", dict(number=0, tuned=False))],
              block=(block_type, body))
    for total, label in ((None, "total_known"), (0, "total_0")):
        d = _nested_frame(rng, 4)
        junk = b"\x01\x02\x03\x04\x05"  # its CRC-16 is not zero: the chain does not close across it
        assert crc16(junk) != 0
        fr = [_plain(rng, "S16", n) for n in range(4)]
        T.add(f"S16/tail_{label}", "S16", fr, [("tail", len(junk), "tail", dict(number=4, tuned=False))], total=total,
              tail=junk + d, kind="tail" if total is None else "tail-total0")
    # for the batch: a stereo header in the trailing junk whose first subframe (513 bytes) runs past the end
    h = header(2, 256, 16, 3) + SUB_VERBATIM
    junk = b"\x09\x08\x07" + h + bytes(rng.randrange(0xF0) for _ in range(40))
    fr = [_plain(rng, "S16", n) for n in range(3)]
    T.add("S16/straddle", "S16", fr, [("tail", 3, "straddle", dict(number=3, tuned=False))], tail=junk)


def _window_rows(T, rng):
    """One frame of 32,768 stereo samples whose payload is all FF F8 pairs: 65,536 candidates between
    its start and its end.  Zeroed samples take pairs away: one fewer puts the next frame inside the
    successor window, none leaves it one candidate outside."""
    for label, zeroed in (("under", 1), ("over", 0)):
        f, subs, _ = carrier_frame(rng, "W16", 0, fill=b"\xff\xf8")
        for z in range(zeroed):
            subs[0]["samples"][100 + z] = 0
        f = frame(subs, 32768, 16, number=0)
        inside = len(sync_pairs(f)) - 1
        assert inside == CHAIN_WIN - zeroed, inside
        fr = [(f, subs)]
        for n in (1, 2):
            s = [{"type": "constant", "value": 17 * n}, {"type": "constant", "value": -n}]
            fr.append((frame(s, 32768, 16, number=n), s))
        T.add(f"W16/window_{label}", "W16", fr, [(0, 7, "window", dict(number=None, tuned=False, inside=inside))],
              kind=f"window-{label}")


def _seam_rows(T, rng):
    """A close-early decoy that is candidate 1,023 / 1,024 of a buffer that starts with this stream:
    the seam of the 1,024-wide scans.  Filler sync pairs in a PADDING block put it there."""
    for index in (1023, 1024):
        f, s, at = carrier_frame(rng, "S16", 0, [(0, 120, decoy_bytes("close-early", 1), True)])
        fr = [(f, s)] + [_plain(rng, "S16", n) for n in (1, 2)]
        body = b"\xff\xf8" * (index - 1) + b"\x00"  # the fillers, then frame 0's own pair, then the decoy
        r = T.add(f"S16/seam_{index}", "S16", fr, [(0, at[0], "close-early", dict(number=1, tuned=True, chan=0))],
                  block=(1, body), kind="seam")
        r.seam_index = index
        assert int(np.searchsorted(sync_pairs(r.data), r.decoys[0].offset)) == index


_ROWS = None


def rows():
    """The table, built once: the same rows in the same order on every call"""
    global _ROWS
    if _ROWS is None:
        T = _Rows()
        for seed, build in enumerate((_payload_rows, _outside_rows, _window_rows, _seam_rows)):
            build(T, random.Random(1663 + seed))
        _ROWS = T.rows
    return _ROWS


def row(name):
    return next(r for r in rows() if r.name == name)


def decoy_frame_bytes(r, d):
    """the carrier frame's bytes in front of a payload decoy: the CRC-16 of these decides `tuned`"""
    return r.data[r.frame_offsets[d.frame]: d.offset]


# ------------------------------------------------------------------ damage and batches
def damage_variants(r):
    """{'before' | 'behind': the frame that loses its CRC-16} for a row, and why a variant is absent.
    'before': one body byte flipped in the frame in front of the decoy's carrier; 'behind': in the
    carrier itself, behind the decoy.  A decoy in a metadata block has the first frame behind it and
    nothing before; one in trailing junk has the last frame before it and nothing behind.
    A variant needs the frames the resync rule resumes with: behind the damaged frame, a frame that
    has a successor of its own (bnf_resync.h, start_ok).  Where the row has no such frames the
    variant would test that rule's own limit, not a decoy, and is left out.  A row at a stated limit
    has only 'before': its decoy is then met after a resync step (the test pins what follows)."""
    n, d = len(r.frame_offsets), r.decoys[0]
    out, absent = {}, {}
    if r.kind in ("window-over", "tail-total0"):
        return out, {"before": "a stated limit without a carrier frame to damage", "behind": "the same"}
    before, behind = (None, 0) if d.frame == "meta" else (n - 1, None) if d.frame == "tail" else (d.frame - 1, d.frame)
    if before is None or before < 0:
        absent["before"] = "no frame in front of the decoy"
    elif d.frame != "tail" and before + 2 >= n:
        absent["before"] = "the carrier is the last frame: nothing to resume at"
    else:
        out["before"] = before
    if r.limit:
        absent["behind"] = "a stated limit: pinned for 'before' only"
    elif behind is None:
        absent["behind"] = "no frame behind the decoy"
    elif behind + 2 >= n:
        absent["behind"] = "fewer than two frames behind the carrier: nothing to resume at"
    else:
        out["behind"] = behind
    return out, absent


def damaged(r, where):
    """The row's stream with damage_variants' byte flipped -> (bytes, the frame that loses its CRC-16).
    The byte lies in the frame's last subframe: headers, walks and every length stay."""
    lost = damage_variants(r)[0][where]
    data = bytearray(r.data)
    at = r.frame_ends[lost] - 10
    assert where == "before" or r.decoys[0].frame == "meta" or at > r.decoys[0].offset + 8
    data[at] ^= 0x10
    return bytes(data), lost


BATCH_ROWS = ("S16/close-early_next", "S16/pair", "S16/nested-n", "S16/straddle", "S16/valid_ch0", None,
              "S16/close-early_other", "S16/tail_total_known", "S16/meta_padding", "S16/close-early_end_of_ch0")


def batch(rng=None):
    """Several S16 rows in one buffer with junk gaps (sync pairs across the stream ends), one empty
    stream, the straddling header at a stream's end and a complete valid frame in a gap.
    -> (buffer, [(begin, end)], [row | None], [(offset, class)] of the decoys that belong to no stream)"""
    rng = rng or random.Random(7)
    gap = bytes([0xF8, 0xFF]) * 8
    buf, ranges, members, loose = bytearray(), [], [], []
    for k, name in enumerate(BATCH_ROWS):
        r = row(name) if name else None
        data = r.data if r else b""
        ranges.append((len(buf), len(buf) + len(data)))
        members.append(r)
        buf += data
        if name == "S16/straddle":  # nothing between this stream's junk and the next stream
            continue
        buf += gap[: (5 * k + 3) % 16]
        if k == 1:
            loose.append((len(buf), "gapdecoy"))
            buf += _nested_frame(rng, 0) + b"\x55"
    return bytes(buf), ranges, members, loose
