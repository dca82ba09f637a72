"""k_decode_st's running CRC-16 of channel 1 (the fold in its chunk loop) against the same
binary with the fold switched off (ablate bit 0x40: the tail reads channel 1 again from
k_parse's prefix): identical frame records and PCM on every case, the computed CRC-16 equal to
the oracle's CRC of the frame's bytes, and damaged frames rejected on both paths.

The shapes are the smallest at which the fold can go wrong: channel 1 shorter than one 64-byte
ring group (blocksize 32), a few groups (192), many (4096); channel 1 starting in every slot of
a line; escaped partitions, long Rice prefixes and wasted bits (the generic and rare paths,
whose blocking refills leave a lane's remainder behind); lanes of one wave with different
lengths and lanes that are not k_decode_st's (C4)."""
import ctypes

import numpy as np
import pytest

from tests.conftest import gpu_available

pytestmark = pytest.mark.gpu

NO_FOLD = 0x40   # include/bnflac.h: bnflac_debug_set_ablate, the exact A/B switch
STATS = 0x100    # event counters on (exact)
FL_ST, FL_REDO = 32, 64  # bnflac_device.h BNF_FL_ST, BNF_FL_REDO


@pytest.fixture(scope="module")
def gpu():
    if not gpu_available():
        pytest.skip("no GPU")
    import torch
    from birdnest.audio_amd import libflac
    dec = libflac.BatchDecoder(0)
    L = dec.L
    # the lane kernels (small batches otherwise take k_decode_sys), the lane-per-frame k_parse
    # (k_parse_wave hands nothing over) and its prefix as the hand-off
    L.bnflac_debug_set_decode_sys(0)
    L.bnflac_debug_set_parse_wave(0)
    L.bnflac_debug_set_crc_mode(1)
    yield torch, libflac, dec
    L.bnflac_debug_set_ablate(0)
    L.bnflac_debug_set_crc_mode(-1)
    L.bnflac_debug_set_parse_wave(-1)
    L.bnflac_debug_set_decode_sys(-1)


def _params(libflac, data):
    si = data[8:42]
    x = int.from_bytes(si[10:18], "big")
    return libflac.StreamParams(1, int.from_bytes(si[0:2], "big"), int.from_bytes(si[2:4], "big"), x >> 44,
                                ((x >> 41) & 7) + 1, ((x >> 36) & 31) + 1, x & ((1 << 36) - 1))


def _decode(gpu, data, offs, ablate, base=0):
    """One batch decode of `data` placed at byte `base` of the device buffer; the frame records,
    the PCM and the event counters of that decode."""
    torch, libflac, dec = gpu
    sp = _params(libflac, data)
    dev = torch.device("cuda:0")
    n = base + len(data)
    d_bytes = torch.zeros((n + 15) // 16 * 16 + 16, dtype=torch.uint8, device=dev)
    d_bytes[base:n] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
    d_offs = torch.tensor([base + int(o) for o in offs], dtype=torch.int64, device=dev)
    stride = libflac.out_stride(libflac.OUT_FLACDECODER, sp)
    d_out = torch.full((sp.total_samples * stride + 64,), 0xAB, dtype=torch.uint8, device=dev)
    d_info = torch.zeros(len(offs) * libflac.FRAME_INFO_BYTES, dtype=torch.uint8, device=dev)
    buf = (ctypes.c_uint64 * 16)()
    dec.L.bnflac_debug_stats(buf, 1)
    dec.L.bnflac_debug_set_ablate(ablate)
    try:
        dec.decode_frames(d_bytes, n, d_offs, len(offs), sp, libflac.OUT_FLACDECODER, d_out, d_info)
        torch.cuda.synchronize()
    finally:
        dec.L.bnflac_debug_set_ablate(0)
    dec.L.bnflac_debug_stats(buf, 1)
    info = libflac.info_array(d_info.cpu().numpy())
    return info, d_out[: sp.total_samples * stride].cpu().numpy(), list(buf)


def _both(gpu, data, offs, base=0):
    """Fold on and off: identical records and PCM, and every CRC-16 the decode reports is the
    oracle's CRC of the frame's bytes (as test_gpu_parity._crc_cases).  Returns the fold-on
    records, PCM and counters, and the fold-off counters."""
    import oracle
    info, out, st = _decode(gpu, data, offs, STATS, base)
    info_b, out_b, st_b = _decode(gpu, data, offs, STATS | NO_FOLD, base)
    for name in info.dtype.names:
        assert np.array_equal(info[name], info_b[name]), name
    assert np.array_equal(out, out_b)
    assert st_b[6] == 0, st_b
    for i, o in enumerate(offs):
        if info["status"][i] != 0:
            continue
        end = int(info["resume_bit"][i]) // 8 - base
        want = oracle.crc16(data[int(o):end - 2])
        assert info["crc16_calc"][i] == want, (i, o)
        assert info["crc_ok"][i] == (want == int.from_bytes(data[end - 2:end], "big")), (i, o)
    return info, out, st, st_b


def _c2(**kw):
    from birdnest.audio_amd import synth
    s = synth.encode(synth.config("C2", **({"nframes": 8, "last_blocksize": 0} | kw)))
    return s, s.data.tobytes(), [int(x) for x in s.frame_offsets]


def _lossless(info, out, s):
    assert (info["status"] == 0).all() and (info["crc_ok"] == 1).all(), info[["status", "crc_ok"]]
    assert out.tobytes() == (s.pcm.astype(np.int64) & 0xFFFF).astype("<u2").tobytes()


@pytest.mark.parametrize("blocksize", [32, 192, 4096])
def test_fold_on_off_identical(gpu, blocksize):
    """Every stereo mode, partition orders 0 and 4.  At 4096 the tail of every frame k_decode_st
    keeps continues the running remainder (a lane folds only while 16 or more samples of ~9 bits
    or more are still to come, so no frame ends inside a folded line); at 32 channel 1 is shorter
    than one group."""
    for stereo_mode in range(4):
        for po in (0, 4):
            s, data, offs = _c2(blocksize=blocksize, stereo_mode=stereo_mode, partition_order=po, seed=10 + po)
            info, out, st, _ = _both(gpu, data, offs)
            _lossless(info, out, s)
            if blocksize == 4096:
                kept = (info["flags"] & (FL_ST | FL_REDO)) == FL_ST
                assert kept.any() and st[6] == kept.sum(), (stereo_mode, po, st, info["flags"])


def test_channel1_in_every_slot(gpu):
    """The stream behind 0..63 junk bytes: the frames, and channel 1 in them, start at every
    offset within a 64-byte line."""
    s, data, offs = _c2(blocksize=192, seed=31)
    used = 0
    for base in range(64):
        info, out, st, _ = _both(gpu, data, offs, base)
        _lossless(info, out, s)
        used += st[6]
    assert used > 0


@pytest.mark.parametrize("kw", [{"escape_permille": 200}, {"impulse_permille": 4}, {"wasted_bits_max": 3},
                                {"escape_permille": 100, "impulse_permille": 2, "partition_order": 0}],
                         ids=["escape", "impulse", "wasted", "escape+impulse"])
def test_generic_and_rare_paths(gpu, kw):
    """Escaped partitions and long prefixes (generic chunks, st_rare_pair, blocking refills) and
    wasted bits: lanes whose ring moved on without the fold read on from where it stopped."""
    s, data, offs = _c2(seed=41, **kw)
    info, out, _, _ = _both(gpu, data, offs)
    _lossless(info, out, s)


def test_c4_mixed_wave(gpu):
    """64 frames of the mixed corpus in one wave: blocksizes 192..16384 side by side, and
    frames of other classes in lanes k_decode_st leaves alone."""
    from birdnest.audio_amd import synth
    s = synth.encode(synth.config("C4", nframes=64, last_blocksize=0))
    data, offs = s.data.tobytes(), [int(x) for x in s.frame_offsets]
    info, out, st, _ = _both(gpu, data, offs)
    _lossless(info, out, s)
    assert st[6] > 0, st


@pytest.fixture(scope="module")
def clean_c2(gpu):
    s, data, offs = _c2(seed=51)
    info, out, st, _ = _both(gpu, data, offs)
    _lossless(info, out, s)
    return s, data, offs, info, st


@pytest.mark.parametrize("where", ["ch1_first_group", "ch1_middle", "ch1_last_group", "footer", "ch0"])
def test_one_flipped_bit(gpu, clean_c2, where):
    """Input damage of the kind the suite already has: the frame is rejected and zero-filled on
    both paths, the others decode as before."""
    s, data, offs, info0, _ = clean_c2
    f = 3
    o, end = offs[f], int(info0["resume_bit"][f]) // 8
    ch1 = o + int(info0["sub_start"][f][1]) // 8
    assert end - ch1 > 64 * 8
    pos = {"ch1_first_group": ch1 + 40, "ch1_middle": (ch1 + end) // 2, "ch1_last_group": end - 30,
           "footer": end - 1, "ch0": o + 60}[where]
    d = bytearray(data)
    d[pos] ^= 0x04
    info, out, _, _ = _both(gpu, bytes(d), offs)
    assert info["crc_ok"][f] == 0 or info["status"][f] != 0, where
    bs = s.params.blocksize
    pcm = out.view("<i2").reshape(-1, 2)
    assert not pcm[f * bs:(f + 1) * bs].any(), where
    keep = np.ones(len(pcm), bool)
    keep[f * bs:(f + 1) * bs] = False
    assert np.array_equal(pcm[keep], s.pcm[keep].astype("<i2")), where
    others = [i for i in range(len(offs)) if i != f]
    assert (info["crc_ok"][others] == 1).all()


def test_check_build_counts_no_disagreement(gpu, clean_c2):
    """A -DBNFLAC_CRC_FOLD_CHECK build computes both remainders in the tail: none may differ."""
    torch, libflac, dec = gpu
    fn = getattr(dec.L, "bnflac_debug_crc_fold_check", None)
    if fn is None or fn() != 1:
        pytest.skip("the library was not built with -DBNFLAC_CRC_FOLD_CHECK")
    _, _, offs, _, st = clean_c2
    assert st[6] == len(offs) and st[7] == 0, st
