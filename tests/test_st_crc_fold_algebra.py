"""k_decode_st's running CRC-16 of channel 1 (bnflac_kernels.hip StFold / st_fold_point /
st_crc16_run), restated in Python over the host algebra of test_crc_algebra.py and checked against
the oracle's bit-serial CRC-16.

The frame's remainder is built from three parts, as the kernel builds it:
- k_parse's prefix: the frame's first line (bytes before the frame cleared) and the whole
  64-byte lines after it, up to channel 1's line (crcp_fold / crcp_z);
- zero or more 64-byte ring groups folded one at a time into the T^4 form (st_fold_point:
  crcz_blk over the line's four 16-byte slots);
- the tail over the rest, bytes past the footer cleared (st_crc16_ok with `from`).
The verdict must be that of the plain frame wherever the three parts meet.
CPU only: these are the formulas, not the kernel (tests/test_gpu_st_crc_fold.py checks that)."""
import random

import pytest

from tests.test_crc_algebra import crcp_fold, crcp_z, crcz_w, frame_with_footer, tail_zero_test, words_le


def prefix(data, b0, wc):
    """k_parse's hand-off: the lines [b0 >> 6, wc) in the tail's form (r0, r1, parity bit)."""
    l0 = b0 >> 6
    s, px = [0] * 15, 0
    for L in range(l0, wc):
        line = bytearray(data[64 * L:64 * L + 64].ljust(64, b"\0"))
        if L == l0:
            for i in range(b0 & 63):
                line[i] = 0
        s, px = crcp_fold(s, px, bytes(line))
    z = crcp_z(s, px)
    return (z[0], z[1] & 0x0FFFFFFF, bin(z[2]).count("1") & 1)


def fold_group(z, data, L):
    """st_fold_point: the whole 64-byte group L (the ring's copy of the line) into z."""
    r0, r1, px = z
    for w in words_le(data[64 * L:64 * L + 64]):
        px ^= w
        r0, r1, _ = crcz_w((r0, r1, 0), w)
    return (r0, r1, px)


def run_verdict(data, b0, b1, wc, fl):
    """st_crc16_run: the running remainder (the lines before fl) when fl is inside (b0, b1],
    else k_parse's prefix (the lines before wc) when it ends inside the frame, continued by the
    tail, else the whole frame."""
    if fl is not None and 64 * fl <= b1 and 64 * fl > b0:
        z = prefix(data, b0, wc)
        for L in range(wc, fl):
            z = fold_group(z, data, L)
        return tail_zero_test(data, b0, b1, z, 64 * fl), True
    if 64 * wc <= b1:
        return tail_zero_test(data, b0, b1, prefix(data, b0, wc), 64 * wc), False
    return tail_zero_test(data, b0, b1), False  # a prefix past the frame's end is not the frame's


def stream(rng, lead, n, good=True, trail=150):
    fr = frame_with_footer(rng, n, good)
    junk = bytes(rng.getrandbits(8) | 1 for _ in range(trail))  # never zero: bytes past the footer must be cleared
    return bytes(rng.getrandbits(8) for _ in range(lead)) + fr + junk, lead, lead + len(fr)


@pytest.mark.parametrize("seed", range(3))
def test_every_split_point(seed):
    """Every prefix end and every number of groups folded after it, good and bad footers."""
    rng = random.Random(200 + seed)
    for _ in range(6):
        data, b0, b1 = stream(rng, rng.randrange(0, 130), rng.randrange(300, 900), good=rng.random() < 0.6)
        want = tail_zero_test(data, b0, b1)
        l0, le = b0 >> 6, b1 >> 6
        for wc in range(l0 + 1, le + 1):
            for fl in range(wc, le + 1):
                got, used = run_verdict(data, b0, b1, wc, fl)
                assert used and got == want, (b0, b1, wc, fl)


@pytest.mark.parametrize("slot", range(4))
@pytest.mark.parametrize("lookahead", [0, 1])
def test_channel1_in_each_slot_of_its_line(slot, lookahead):
    """Channel 1 starting in each 16-byte slot of a line: the prefix ends at its line, or (the
    reader's lookahead across the line's end) the ring's first group is the line after it and
    the line between is folded from memory -- the same fold."""
    rng = random.Random(300 + slot)
    for lead in range(0, 64, 7):
        data, b0, b1 = stream(rng, lead, 700)
        sub1 = ((b0 + 200) & ~63) + 16 * slot + rng.randrange(16)  # channel 1's first byte
        l1 = sub1 >> 6
        first_group = l1 + lookahead
        for fl in range(first_group, (b1 >> 6) + 1):
            got, used = run_verdict(data, b0, b1, l1, fl)
            assert used and got is True, (lead, slot, lookahead, fl)


@pytest.mark.parametrize("cut", [0, 1, 2])
def test_footer_straddles_a_line(cut):
    """The frame's last line boundary falls before, inside and after the two footer bytes."""
    rng = random.Random(400 + cut)
    for lead in (0, 5, 63):
        for good in (True, False):
            n = 64 * 9 - lead - cut  # b1 = 64 * 9 + 2 - cut: 0, 1 or 2 footer bytes in line 9
            data, b0, b1 = stream(rng, lead, n, good)
            assert b1 == 64 * 9 + 2 - cut
            for fl in range((b0 >> 6) + 1, (b1 >> 6) + 1):
                got, used = run_verdict(data, b0, b1, (b0 >> 6) + 1, fl)
                assert used and got == good, (lead, good, fl)


def test_folded_past_the_footer_falls_back():
    """A group folded whole although the frame ends inside it holds bytes past the footer: the
    tail must not continue it (st_crc16_run's bound) and takes the prefix instead."""
    rng = random.Random(500)
    for _ in range(20):
        data, b0, b1 = stream(rng, rng.randrange(64), rng.randrange(300, 600))
        if b1 & 63 == 0:
            continue
        wc = (b0 >> 6) + 1
        got, used = run_verdict(data, b0, b1, wc, (b1 >> 6) + 1)
        assert not used and got is True
        z = prefix(data, b0, wc)
        for L in range(wc, (b1 >> 6) + 1):
            z = fold_group(z, data, L)
        assert not tail_zero_test(data, b0, b1, z, 64 * ((b1 >> 6) + 1))  # what the bound prevents


def test_channel1_shorter_than_one_group():
    """Nothing is ever folded in the loop: the running remainder is the prefix itself; and a
    frame inside one line, whose prefix already covers that line, keeps the plain path."""
    rng = random.Random(600)
    for lead in range(0, 64, 9):
        for good in (True, False):
            data, b0, b1 = stream(rng, lead, 100, good)
            for wc in range((b0 >> 6) + 1, (b1 >> 6) + 1):
                got, used = run_verdict(data, b0, b1, wc, wc)
                assert used and got == good
            data, b0, b1 = stream(rng, lead % 32, 20, good)  # ends inside its first line
            got, used = run_verdict(data, b0, b1, (b0 >> 6) + 1, (b0 >> 6) + 1)
            assert not used and got == good
            got, used = run_verdict(data, b0, b1, (b0 >> 6) + 1, None)
            assert not used and got == good
