"""The host side of tests/test_gpu_decode_routes.py (tests/decode_routes.py), without a GPU: every
batch and primer builds, its table and its expected output have the shapes the GPU module relies
on, and the stride-loop batches pass the launchers' 512 workgroups by two blocks."""
import numpy as np
import pytest

from tests import decode_routes as R


def test_launcher_constants_are_the_sources():
    """DEC_LANES and the 512-workgroup cap, read from the sources the helpers restate them from"""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "birdnest", "audio_amd", "csrc")
    assert int(re.search(r"#define DEC_LANES (\d+)", open(os.path.join(csrc, "bnf_residual.h")).read()).group(1)) == R.DEC_LANES
    k = open(os.path.join(csrc, "bnflac_kernels.hip")).read()
    for fn in ("bnf_launch_decode_list", "bnf_launch_decode_seg"):
        body = k[k.index("hipError_t " + fn + "("):]
        assert int(re.search(r"std::min<uint32_t>\(\(nframes \+ fpb - 1\) / fpb, (\d+)u\)", body).group(1)) == R.STRIDE_WGS
    assert R.fpb(2) == 32 and R.fpb(8) == 8 and R.fpb(1) == 64


@pytest.mark.parametrize("name", list(R.BATCHES) + ["primer:" + p for p in R.PRIMERS])
def test_batches_build(name):
    b = R.batch(name)
    assert b is R.batch(name)  # encoded once
    assert b.channels == 2 and 0 < b.nbytes <= len(b.data)
    assert (b.offs >= 0).all() and (b.offs < len(b.data)).all() and len(set(b.offs.tolist())) == b.nframes
    for fmt, stride in (("OUT_INTERLEAVED32", 8), ("OUT_FLACDECODER", 4)):
        e = b.expected(fmt)
        assert e.dtype == np.uint8 and e.size == b.total * stride
    if b.osmp is not None:  # fixed blocksize: the frames tile the output, each sample covered at most once
        assert (b.osmp % R.BS == 0).all() and len(set(b.osmp.tolist())) == b.nframes and b.osmp.max() + R.BS <= b.total
        named = set(b.osmp.tolist())
        covered = b.nframes * R.BS + sum(n for s, n in b.keep if s not in named)
        assert covered == b.total
    pcm = b.expected("OUT_INTERLEAVED32").view("<i4").reshape(b.total, 2)
    plain = np.ones(b.total, dtype=bool)
    for s, n in b.zero + b.keep:
        plain[s:s + n] = False
    assert np.array_equal(pcm[plain], b.pcm[plain])
    for s, n in b.zero:
        assert not pcm[s:s + n].any()
    for s, n in b.keep:
        assert (pcm[s:s + n].view(np.uint8) == R.FILL).all()


def test_batch_shapes():
    f = R.fpb(2)
    assert [R.batch(n).nframes for n in ("one", "fpb", "fpb_plus_1", "mixed65", "c4_700", "plain16")] == [1, f, f + 1, 65, 700, 16]
    d = R.batch("damaged")
    hdr, st, w16, cut = d.damaged
    assert len({hdr, st, w16, cut}) == 4 and d.nbytes == len(d.data) - 3
    assert d.offs[cut] == d.offs.max() and d.nbytes > d.offs[cut] + 8  # the cut frame keeps its header
    assert sorted(d.zero) == sorted((int(d.osmp[k]), R.BS) for k in (st, w16, cut)) and d.keep == ((int(d.osmp[hdr]), R.BS),)
    clean = R._mixed_batch(6, class1=True)[0]
    diff = np.nonzero(np.frombuffer(clean, np.uint8) != np.frombuffer(d.data, np.uint8))[0]
    assert len(diff) == 3 and d.offs[hdr] + 2 in diff  # one byte each: a header, two residuals
    for k in (st, w16):  # the residual bytes lie deep inside their frames
        inside = diff[(diff > d.offs[k] + 256) & (diff < d.offs[k] + 1024 * 1024)]
        assert len(inside) >= 1 and inside[0] < np.sort(d.offs[d.offs > d.offs[k]])[0] - 256
    assert R.batch("c4_700").osmp is None and R.batch("c4_700").sp.min_blocksize < R.batch("c4_700").sp.max_blocksize


def test_history_of_classes():
    from birdnest.audio_amd import libflac
    info = np.zeros(7, dtype=libflac.FRAME_INFO_DTYPE)
    info["flags"] = [R.FL_ST, R.FL_ST | R.FL_REDO, R.FL_W16, R.FL_W32, 0, R.FL_ST, R.FL_W16]
    info["status"][5:] = 1  # failed frames are class 1 whatever their flags
    assert R.history_of(info) == (1, 1, 7, 3)
    for name, want in R.PRIMERS.items():
        if want["hist"] is not None:
            assert want["hist"][2] == R.batch("primer:" + name).nframes


@pytest.mark.parametrize("channels", [2, 8])
def test_seg_trip_shape(channels):
    """The generator encodes 16-bit streams of 8 channels, so the fpb = 8 case exists."""
    b, nwide, lead = R.seg_trip_batch(channels)
    f = R.fpb(channels)
    assert b.channels == channels and b.nframes == nwide + lead
    assert nwide >= R.STRIDE_WGS * f + 2 * f and nwide % f != 0  # two more whole blocks, then a partial one
    assert 0 < lead < f                                          # the segment starts inside the first block
    assert b.total * 4 * channels < 36 << 20                     # about 34 MB of output
    assert len(set(b.offs[:nwide].tolist())) == 8 and len(set(b.offs.tolist())) == 8 + lead
    assert np.array_equal(b.osmp, np.arange(b.nframes) * 256)
    assert np.array_equal(b.pcm[:256], b.pcm[8 * 256:9 * 256]) and not np.array_equal(b.pcm[:256], b.pcm[256:512])


def test_list_trip_shape():
    n = R.stride_trip_frames(2)
    t = R.list_trip_table(n)
    assert t.sum() == n and n > R.STRIDE_WGS * R.fpb(2) + 2 * R.fpb(2) and not t[1::2].any() and t[0::2].all()
