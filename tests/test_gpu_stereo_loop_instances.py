"""The chunk-loop instances of k_decode_st, and the fused variants of k_decode_sw.

k_decode_st compiles its whole chunk loop once per wave-uniform stereo assignment (0..3, and
-1 for a wave of mixed assignments or with wasted bits).  A wave picks one instance for all
its chunks, so every instance has to handle every kind of chunk by itself: fused chunks,
generic chunks (warm-up, partitions that do not end on a chunk, a frame's partial last chunk),
lanes whose frame has ended beside lanes that still decode, and the changes between them.
k_decode_sw picks its fused variant (restore path, assignment, whole-line flush) chunk by
chunk; its twins below pin the same behaviour for the day its loop is split the same way.

Each case here is two waves (128 frames; 64-128 for the 24-bit twins) that select one instance,
decoded over shapes that put each kind of chunk into that instance:
  (a) blocksize 4096, partition order 4: fused chunks, partitions aligned to chunks
  (b) blocksize 1000: not a multiple of 32, the last chunk is generic
  (c) variable blocksizes 192..4608 inside one wave: lanes end early, the others stay fused
  (d) partitions of 72 samples (4608 / 2^6: a partition ends inside every other chunk, so the
      loop goes fused -> generic -> fused) and of 16 samples (4096 / 2^8: shorter than a chunk)
  (e) blocksize 32: no fused chunk at all
The PCM must equal the generator's source PCM and every record must say OK, CRC ok, the
oracle's CRC-16 of the frame's bytes, and the kernel's class flag without a hand-back: a
hand-back would let k_decode<8> / k_decode<16> hide a broken instance.  Which shapes the fast
paths keep was read off the parent commit's build (every frame of every case below).
"""
import numpy as np
import pytest

from tests.conftest import gpu_available

pytestmark = pytest.mark.gpu

FL_ST, FL_REDO, FL_SW = 32, 64, 1024  # bnflac_device.h BNF_FL_ST, BNF_FL_REDO, BNF_FL_SW
SW_NO_LINE = 0x20000000               # include/bnflac.h: k_decode_sw without the whole-line flush (exact)


@pytest.fixture(scope="module")
def gpu():
    if not gpu_available():
        pytest.skip("no GPU")
    import torch
    from birdnest.audio_amd import libflac
    dec = libflac.BatchDecoder(0)
    L = dec.L
    # the lane kernels (small batches otherwise take k_decode_sys), the lane-per-frame k_parse
    # and its CRC prefix, so that k_decode_st runs with its channel-1 fold as at bench size
    L.bnflac_debug_set_decode_sys(0)
    L.bnflac_debug_set_parse_wave(0)
    L.bnflac_debug_set_crc_mode(1)
    yield torch, libflac, dec
    L.bnflac_debug_set_ablate(0)
    L.bnflac_debug_set_crc_mode(-1)
    L.bnflac_debug_set_parse_wave(-1)
    L.bnflac_debug_set_decode_sys(-1)


# 16-bit stereo: which loop instance of k_decode_st the waves take
ST_CASES = {
    "indep": dict(stereo_mode=0),        # instance 0
    "left_side": dict(stereo_mode=1),    # instance 1
    "right_side": dict(stereo_mode=2),   # instance 2
    "mid_side": dict(stereo_mode=3),     # instance 3
    "mixed": dict(stereo_mode=4),        # frame f has assignment f % 4: instance -1
    # mid/side over left and right with one wasted bit: the side channel keeps the bit, the mid
    # channel (l + r) >> 1 does not: wasted bits in one channel, instance -1 through anyw
    "wasted": dict(stereo_mode=3, wasted_bits_max=1),
}
SHAPES = {
    "a_4096_po4": dict(blocksize=4096, partition_order=4),
    "b_1000": dict(blocksize=1000, partition_order=3),
    "c_variable": dict(variable_blocksize=1, bs_min=192, bs_max=4608, partition_order=-1),
    "d_part72": dict(blocksize=4608, partition_order=6),
    "d_part16": dict(blocksize=4096, partition_order=8),
    "e_32": dict(blocksize=32, partition_order=1),
}
# 24-bit stereo (C3-shaped frames): which loop instance of k_decode_sw
SW_CASES = {
    "mid_side": dict(stereo_mode=3, wasted_bits_max=4),  # fix 3 (C3's own)
    "indep": dict(stereo_mode=0, wasted_bits_max=0),     # fix 0
    "left_side": dict(stereo_mode=1, wasted_bits_max=0), # no instance of its own: the per-lane variant
    "mixed": dict(stereo_mode=4, wasted_bits_max=2),     # mixed assignments: the per-lane variant
}
SW_SHAPES = {
    "1152": dict(blocksize=1152, nframes=128),
    "4608": dict(blocksize=4608, nframes=64),
    "4608_part72": dict(blocksize=4608, nframes=64, partition_order=6),
    "variable": dict(variable_blocksize=1, bs_min=192, bs_max=4608, nframes=128),
}

_STREAMS = {}


def _stream(cfg, case, shape):
    """The encoded stream of one (case, shape), made once and shared by the layouts."""
    from birdnest.audio_amd import synth
    key = (cfg, case, shape)
    if key not in _STREAMS:
        kw = dict(nframes=128, last_blocksize=0, seed=7 + len(_STREAMS))
        kw.update((ST_CASES if cfg == "C2" else SW_CASES)[case])
        kw.update((SHAPES if cfg == "C2" else SW_SHAPES)[shape])
        s = synth.encode(synth.config(cfg, **kw))
        _STREAMS[key] = (s, s.data.tobytes(), [int(o) for o in s.frame_offsets])
    return _STREAMS[key]


def _decode(gpu, data, offs, fmt, ablate=0):
    from tests.test_gpu_parity import _decode_batch
    _, _, dec = gpu
    dec.L.bnflac_debug_set_ablate(ablate)
    try:
        return _decode_batch(gpu, data, offs, fmt)
    finally:
        dec.L.bnflac_debug_set_ablate(0)


def _expect(libflac, fmt, pcm, bps):
    if fmt == libflac.OUT_INTERLEAVED32:
        return pcm.astype("<i4").tobytes()
    v = pcm.astype(np.int64).reshape(-1)
    if bps == 24:
        return np.stack([v & 0xFF, (v >> 8) & 0xFF, (v >> 16) & 0xFF], axis=1).astype(np.uint8).tobytes()
    return (v & 0xFFFF).astype("<u2").tobytes()


def _check(libflac, fmt, s, data, offs, out, info, cls, tag):
    """Source PCM, and the records against the oracle: status, crc_ok, crc16_calc, flags."""
    import oracle
    print(tag, "kept", int(((info["flags"] & (cls | FL_REDO)) == cls).sum()), "of", len(offs))
    assert (info["status"] == 0).all(), (tag, info["status"])
    assert (info["crc_ok"] == 1).all(), (tag, info["crc_ok"])
    for i, o in enumerate(offs):
        end = int(info["resume_bit"][i]) // 8
        assert end == (offs[i + 1] if i + 1 < len(offs) else len(data)), (tag, i)
        assert info["crc16_calc"][i] == oracle.crc16(data[o:end - 2]), (tag, i)
    assert (info["flags"] & cls).all(), (tag, info["flags"])
    assert not (info["flags"] & FL_REDO).any(), (tag, np.nonzero(info["flags"] & FL_REDO)[0])
    assert out.tobytes() == _expect(libflac, fmt, s.pcm, s.params.bps), tag


@pytest.mark.parametrize("fmt_name", ["OUT_FLACDECODER", "OUT_INTERLEAVED32"])
@pytest.mark.parametrize("case", list(ST_CASES))
def test_st_instance_sees_every_chunk_kind(gpu, case, fmt_name):
    _, libflac, _ = gpu
    fmt = getattr(libflac, fmt_name)
    for shape in SHAPES:
        s, data, offs = _stream("C2", case, shape)
        out, info, _ = _decode(gpu, data, offs, fmt)
        _check(libflac, fmt, s, data, offs, out, info, FL_ST, (case, shape, fmt_name))


def test_st_cases_select_their_instance():
    """The inputs are what the cases say: one assignment per wave, or all four in each wave,
    and, for `wasted`, frames whose two subframes differ in their wasted-bits flag."""
    for case, kw in ST_CASES.items():
        s, data, offs = _stream("C2", case, "a_4096_po4")
        asg = [data[o + 3] >> 4 for o in offs]  # the frame header's channel assignment code
        want = {0: {1}, 1: {8}, 2: {9}, 3: {10}, 4: {1, 8, 9, 10}}[kw["stereo_mode"]]
        assert set(asg[:64]) == want and set(asg[64:]) == want, case
    s, data, offs = _stream("C2", "wasted", "a_4096_po4")
    side_only = 0
    for i, o in enumerate(offs):
        a, b = s.pcm[i * 4096:(i + 1) * 4096, 0].astype(np.int64), s.pcm[i * 4096:(i + 1) * 4096, 1].astype(np.int64)
        side_only += bool(((a - b) & 1).any() == 0 and (((a + b) >> 1) & 1).any())
    assert side_only >= 16, side_only


@pytest.mark.parametrize("leg", ["OUT_FILEREADER", "OUT_FILEREADER-noline", "OUT_INTERLEAVED32"])
@pytest.mark.parametrize("case", list(SW_CASES))
def test_sw_instance_sees_every_chunk_kind(gpu, case, leg):
    """The 24-bit twins: FileReader with and without the whole-line flush (LN 1 / 0), and one
    32-bit layout."""
    _, libflac, _ = gpu
    fmt = getattr(libflac, leg.split("-")[0])
    for shape in SW_SHAPES:
        s, data, offs = _stream("C3", case, shape)
        out, info, _ = _decode(gpu, data, offs, fmt, SW_NO_LINE if leg.endswith("noline") else 0)
        _check(libflac, fmt, s, data, offs, out, info, FL_SW, (case, shape, leg))
