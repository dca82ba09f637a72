"""Decode-class split across streams (SURVEY.md 8a A10 dispatch; bnf_launch_decode).

k_decode_st -> k_decode<8> run on the caller's stream, and k_decode<16> / k_decode<32> each
on a side stream forked before k_decode_st (or after it, BNFLAC_DECODE_FORK=1).  k_decode<8>
takes k_decode_st's hand-backs (BNF_FL_REDO) also in blocks that belong to the other
instances, which never look at stereo fast-path frames.
These tests put hand-back-prone stereo frames, LPC-12 (W16) and LPC-32 (W32) frames into
one batch, so the decode order's 32-frame blocks mix the classes at their edges, and
compare with the generator's source PCM and with the serial order (BNFLAC_DECODE_SERIAL=1,
in a child process).  The batches here are small enough for k_decode_sys's auto range, so the
module pins the lane kernels.  When the previous decode order had no W16 / W32 frames, both
classes go through one small segment grid (k_decode_seg) instead of the side grids: the last
test decodes a batch without them first, so that its mixed batch takes that path.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import gpu_available

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FL_REDO = 64  # BNF_FL_REDO (bnflac_device.h)


@pytest.fixture(autouse=True)
def _lane_kernels():
    if not gpu_available():
        yield
        return
    from birdnest.audio_amd import libflac
    L = libflac.load()
    L.bnflac_debug_set_decode_sys(0)
    yield
    L.bnflac_debug_set_decode_sys(-1)


def _mixed_batch(n_each, class1=False):
    from birdnest.audio_amd import synth
    parts = [
        synth.encode(synth.config("C2", nframes=n_each, stereo_mode=3, level=0.9, noise=0.5, seed=41)),
        synth.encode(synth.config("C2", nframes=n_each, order=12, seed=42)),
        synth.encode(synth.config("C2", nframes=n_each, order=32, partition_order=-1, seed=43)),
        synth.encode(synth.config("C2", nframes=n_each, seed=44)),
    ]
    if class1:  # C4's subframe mix at a fixed blocksize: VERBATIM / CONSTANT frames (decode class 1)
        parts.append(synth.encode(synth.config("C2", nframes=n_each, subframe_mode=synth.SUB_MIXED,
                                               stereo_mode=synth.ST_CYCLE, partition_order=-1, seed=45)))
    data, offs, osmp, pcm = bytearray(), [], [], []
    base = 0
    for s in parts:
        fo = s.frame_offsets.astype(np.int64)
        offs.append(fo + len(data))
        nsamp = np.full(len(fo), 4096, dtype=np.int64)
        nsamp[-1] = s.nsamples - 4096 * (len(fo) - 1)
        osmp.append(base + np.concatenate([[0], np.cumsum(nsamp)[:-1]]))
        pcm.append(s.pcm)
        data += s.data.tobytes()
        base += s.nsamples
    # frame i of each part in turn, so the classes alternate before the decode order sorts them
    order = [(p, i) for i in range(n_each) for p in range(len(parts))]
    o = np.array([offs[p][i] for p, i in order], dtype=np.int64)
    os_ = np.array([osmp[p][i] for p, i in order], dtype=np.int64)
    return bytes(data), o, os_, np.concatenate(pcm), base


def _decode(data, offs, osmp, total, sp=None, fmt=None):
    """osmp None: frames positioned by their own sample numbers (a whole stream, sp its STREAMINFO).
    fmt None: OUT_INTERLEAVED32."""
    import torch
    from birdnest.audio_amd import libflac
    dev = torch.device("cuda:0")
    if fmt is None:
        fmt = libflac.OUT_INTERLEAVED32
    if sp is None:
        sp = libflac.StreamParams(1, 4096, 4096, 44100, 2, 16, total)
    n = len(data)
    d_bytes = torch.zeros((n + 3) // 4 * 4 + 16, dtype=torch.uint8, device=dev)
    d_bytes[:n] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
    d_offs = torch.from_numpy(offs).to(dev)
    d_os = torch.from_numpy(osmp).to(dev) if osmp is not None else None
    stride = libflac.out_stride(fmt, sp)
    d_out = torch.full((total * stride,), 0xAB, dtype=torch.uint8, device=dev)
    d_info = torch.zeros(len(offs) * libflac.FRAME_INFO_BYTES, dtype=torch.uint8, device=dev)
    libflac.BatchDecoder(0).decode_frames(d_bytes, n, d_offs, len(offs), sp, fmt, d_out, d_info, d_out_sample=d_os)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), libflac.info_array(d_info.cpu().numpy())


@pytest.mark.skipif(not gpu_available(), reason="no GPU")
@pytest.mark.parametrize("n_each", [7, 20, 45])
def test_mixed_classes_with_handbacks(n_each):
    data, offs, osmp, pcm, total = _mixed_batch(n_each)
    out, info = _decode(data, offs, osmp, total)
    assert (info["status"] == 0).all() and (info["crc_ok"] == 1).all()
    assert (info["flags"] & FL_REDO).any(), "the batch should hold handed-back stereo frames"
    assert np.array_equal(out.view("<i4").reshape(-1, 2), pcm)


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from tests.test_gpu_decode_classes import _mixed_batch, _decode
data, offs, osmp, pcm, total = _mixed_batch(20)
out, info = _decode(data, offs, osmp, total)
sys.stdout.buffer.write(out.tobytes())
# the batch with class-1 frames twice: the second decode has the W = 8 split armed by the first
from birdnest.audio_amd import libflac
data, offs, osmp, pcm, total = _mixed_batch(13, class1=True)
_decode(data, offs, osmp, total)
out, info = _decode(data, offs, osmp, total)
sys.stdout.buffer.write(out.tobytes())
sys.stdout.buffer.write(np.array([libflac.last_route()["decode"]], dtype="<u4").tobytes())
"""


@pytest.mark.skipif(not gpu_available(), reason="no GPU")
@pytest.mark.parametrize("env", [{"BNFLAC_DECODE_SERIAL": "1"}, {"BNFLAC_DECODE_FORK": "1"}])
def test_side_stream_matches_other_orders(env):
    """The serial order and the fork after k_decode_st (in a child process: the order is read
    once) give the bytes of the default order, also for a batch with class-1 frames decoded with
    the W = 8 split armed; the child reports the order it took (bnflac_debug_last_route)."""
    from birdnest.audio_amd import libflac
    data, offs, osmp, pcm, total = _mixed_batch(20)
    out, _ = _decode(data, offs, osmp, total)
    data, offs, osmp, pcm2, total = _mixed_batch(13, class1=True)
    _decode(data, offs, osmp, total)
    out2, _ = _decode(data, offs, osmp, total)
    default = libflac.last_route()
    assert default["fork_before"] and default["w8split"], default
    assert np.array_equal(out2.view("<i4").reshape(-1, 2), pcm2)
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=dict(os.environ, BNFLAC_DECODE_SYS="0", **env),
                       capture_output=True, timeout=100)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    n, n2 = len(out.tobytes()), len(out2.tobytes())
    assert len(r.stdout) == n + n2 + 4
    assert r.stdout[:n] == out.tobytes()
    assert r.stdout[n:n + n2] == out2.tobytes()
    route = int(np.frombuffer(r.stdout[n + n2:], dtype="<u4")[0])
    if "BNFLAC_DECODE_FORK" in env:
        assert route & libflac.RT_FORK_AFTER and route & libflac.RT_W8SPLIT, hex(route)
    else:  # no side streams: no history, no split
        assert route & libflac.RT_SERIAL and not route & (libflac.RT_W8SPLIT | libflac.RT_HIST), hex(route)


def _plain_c2(nframes):
    from birdnest.audio_amd import synth
    s = synth.encode(synth.config("C2", nframes=nframes, seed=44))
    fo = s.frame_offsets.astype(np.int64)
    osmp = np.arange(len(fo), dtype=np.int64) * 4096
    return s.data.tobytes(), fo, osmp, s.pcm, s.nsamples


@pytest.mark.skipif(not gpu_available(), reason="no GPU")
@pytest.mark.parametrize("n_each", [7, 45])
def test_segment_grid_after_batch_without_w16_w32(n_each):
    from birdnest.audio_amd import libflac
    L = libflac.load()
    data, offs, osmp, pcm, total = _plain_c2(40)
    out, info = _decode(data, offs, osmp, total)  # records W16 = W32 = 0 for the next decode
    assert np.array_equal(out.view("<i4").reshape(-1, 2), pcm)
    data, offs, osmp, pcm, total = _mixed_batch(n_each)
    n0 = L.bnflac_debug_decode_seg_launches()
    out, info = _decode(data, offs, osmp, total)  # W16 + W32 through k_decode_seg
    assert L.bnflac_debug_decode_seg_launches() == n0 + 1
    assert (info["status"] == 0).all() and (info["crc_ok"] == 1).all()
    assert np.array_equal(out.view("<i4").reshape(-1, 2), pcm)
    out2, info2 = _decode(data, offs, osmp, total)  # this batch had both: the side grids again
    assert L.bnflac_debug_decode_seg_launches() == n0 + 1
    assert out2.tobytes() == out.tobytes() and info2.tobytes() == info.tobytes()


@pytest.mark.skipif(not gpu_available(), reason="no GPU")
@pytest.mark.parametrize("n_each", [9, 40])
def test_w8_split_launches(n_each):
    """k_decode<8> as two launches (the class-1 frames on a third side stream beside
    k_decode_st, the stereo hand-backs after it) once the previous decode order had class-1
    frames: the same bytes and records as the single launch (host bit 0x100000)."""
    from birdnest.audio_amd import libflac
    L = libflac.load()
    data, offs, osmp, pcm, total = _mixed_batch(n_each, class1=True)
    _decode(data, offs, osmp, total)  # records the class-1 count for the next decode
    out, info = _decode(data, offs, osmp, total)
    assert (info["status"] == 0).all() and (info["crc_ok"] == 1).all()
    assert (info["flags"] & FL_REDO).any(), "the batch should hold handed-back stereo frames"
    assert np.array_equal(out.view("<i4").reshape(-1, 2), pcm)
    L.bnflac_debug_set_ablate(0x100000)
    try:
        out1, info1 = _decode(data, offs, osmp, total)
    finally:
        L.bnflac_debug_set_ablate(0)
    assert out1.tobytes() == out.tobytes() and info1.tobytes() == info.tobytes()


FL_W32, FL_ST, FL_W16 = 16, 32, 128
FL_WAVE_REDO = 512  # BNF_FL_WAVE_REDO: k_decode_sys handed the frame back to k_decode_list
SYS_ONLY_BITS = 0x40000 | 0x80000  # bnflac_launch.h: BNF_ABLATE_SYS_MIXED | BNF_ABLATE_SYS_LAND_ONLY


def _c4_64():
    """BASELINE C4's shape at 64 frames: variable blocksize, every decode class."""
    from birdnest.audio_amd import libflac, synth
    from tests.test_gpu_parity import _stream_params
    s = synth.encode(synth.config("C4", nframes=64, last_blocksize=0))
    data = s.data.tobytes()
    return data, s.frame_offsets.astype(np.int64), None, s.pcm, s.nsamples, _stream_params(libflac, data)


@pytest.mark.skipif(not gpu_available(), reason="no GPU")
@pytest.mark.parametrize("batch", ["c4_64", "mixed_class1"])
def test_sys_ablate_bits_never_reach_lane_kernels(batch):
    """k_decode_sys's ablation bits 0x40000 / 0x80000 have the numeric values of k_decode<8>'s
    mode bits BNF_MODE_NOST / BNF_MODE_STREDO.  The launchers pass each kernel family only the
    ablation bits it defines, so with the lane kernels forced a user who sets the two sys bits
    gets the same records and PCM as with none (before the fields were separated, the W = 8
    instance then took neither the class-1 frames nor k_decode_st's hand-backs).  The first
    decode, with no bit set, also arms the W = 8 split for the second."""
    from birdnest.audio_amd import libflac
    L = libflac.load()
    if batch == "c4_64":
        data, offs, osmp, pcm, total, sp = _c4_64()
    else:
        data, offs, osmp, pcm, total = _mixed_batch(13, class1=True)
        sp = None
    L.bnflac_debug_set_ablate(0)
    out, info = _decode(data, offs, osmp, total, sp)
    fl = info["flags"]
    assert (info["status"] == 0).all() and (info["crc_ok"] == 1).all()
    assert (fl & FL_ST).any(), "the batch should hold stereo fast-path frames (BNF_FL_ST)"
    assert ((fl & (FL_ST | FL_W16 | FL_W32)) == 0).any(), "the batch should hold class-1 frames"
    assert np.array_equal(out.view("<i4").reshape(-1, 2), pcm)
    L.bnflac_debug_set_ablate(SYS_ONLY_BITS)
    try:
        out1, info1 = _decode(data, offs, osmp, total, sp)
    finally:
        L.bnflac_debug_set_ablate(0)
    assert info1.tobytes() == info.tobytes()
    assert out1.tobytes() == out.tobytes()


def _three_frames(**kw):
    from birdnest.audio_amd import synth
    s = synth.encode(synth.config("C2", nframes=3, **kw))
    fo = s.frame_offsets.astype(np.int64)
    assert len(fo) == 3
    return s.data.tobytes(), fo, np.arange(3, dtype=np.int64) * 4096, s.pcm, s.nsamples


@pytest.mark.skipif(not gpu_available(), reason="no GPU")
def test_every_kernel_tu_reports_its_counters():
    """bnf_stats sums g_stats over the table of kernel TUs that the parse TU keeps (g_tus); a
    TU left out of it uploads no tables and reports no counters.  One 3-frame batch (a partial
    wave, a last frame) per counting object -- k_decode_st<FLACDECODER>, k_decode_st's other
    layouts, k_decode<16>, k_decode<32>, k_decode<8>, k_decode_sys -- with the counters on
    (BNF_ABLATE_STATS): each must count its waves (slot 5), next to the usual status, CRC and PCM
    checks.  The flags say which lane kernel a batch went to.  (k_decode_sw has no slot 5.)"""
    import ctypes
    from birdnest.audio_amd import libflac, synth
    L = libflac.load()
    plain = _three_frames(seed=44)
    classes = (FL_ST | FL_W16 | FL_W32)
    cases = [  # name, batch, layout, the class every frame must carry, k_decode_sys
        ("k_decode_st<FLACDECODER>", plain, libflac.OUT_FLACDECODER, FL_ST, 0),
        ("k_decode_st<INTERLEAVED32>", plain, libflac.OUT_INTERLEAVED32, FL_ST, 0),
        ("k_decode<16>", _three_frames(order=12, seed=42), libflac.OUT_INTERLEAVED32, FL_W16, 0),
        ("k_decode<32>", _three_frames(order=32, partition_order=-1, seed=43), libflac.OUT_INTERLEAVED32, FL_W32, 0),
        ("k_decode<8>", _three_frames(subframe_mode=synth.SUB_MIXED, seed=45), libflac.OUT_INTERLEAVED32, 0, 0),
        ("k_decode_sys", plain, libflac.OUT_INTERLEAVED32, FL_ST, 1),
    ]
    buf = (ctypes.c_uint64 * 16)()
    for name, (data, offs, osmp, pcm, total), fmt, cls, sys_on in cases:
        L.bnflac_debug_stats(buf, 1)
        L.bnflac_debug_set_ablate(0x100)  # BNF_ABLATE_STATS
        L.bnflac_debug_set_decode_sys(sys_on)
        try:
            out, info = _decode(data, offs, osmp, total, fmt=fmt)
        finally:
            L.bnflac_debug_set_decode_sys(0)
            L.bnflac_debug_set_ablate(0)
        L.bnflac_debug_stats(buf, 1)
        assert (info["status"] == 0).all() and (info["crc_ok"] == 1).all(), name
        if cls:
            assert ((info["flags"] & classes) == cls).all(), (name, info["flags"])
        else:  # class 1: at least one frame that no other lane kernel takes
            assert ((info["flags"] & classes) == 0).any(), (name, info["flags"])
        if cls == FL_ST and not sys_on:  # k_decode_st kept its frames: the count is its own
            assert not (info["flags"] & FL_REDO).any(), (name, info["flags"])
        if sys_on:  # k_decode_sys handed nothing back: no k_decode_list wave (the W = 32 object) counted
            assert not (info["flags"] & FL_WAVE_REDO).any(), (name, info["flags"])
        if fmt == libflac.OUT_FLACDECODER:
            assert out.tobytes() == (pcm.astype(np.int64) & 0xFFFF).astype("<u2").tobytes(), name
        else:
            assert np.array_equal(out.view("<i4").reshape(-1, 2), pcm), name
        assert buf[5] > 0, (name, list(buf))
