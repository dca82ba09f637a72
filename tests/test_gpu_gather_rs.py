"""bnflac_gather_ranges_f32_rs on the device: windows of a decoded selection as float32 channel planes
at another sample rate.

Every result is compared three ways: bit for bit (uint32 view) with the host twin
(bnflac_gather_ranges_f32_rs_host), within the derived bound of the float64 yardstick of
tests/test_resample_host.py (`ref_rs`: numpy, no tiles, no steps), and status word for status word.
Floats the contract leaves alone keep their canary.  The shapes are the smallest at which the kernel
takes another path: rows round the output tile (libflac.RS_TILE), ratios that need one or several
steps per tile, the smallest and the largest tables, every layout, every source phase modulo 16
bytes and every destination phase modulo 4 floats (an odd plane_pitch).
"""
import ctypes

import numpy as np
import pytest

from tests.conftest import gpu_available
from tests.test_gather_f32_host import CANARY, MONO, assert_bits, layout, params, random_pcm, window_table
from tests.test_gpu_index_streams import _pack, _stream_params, _upload
from tests.test_gpu_select_ranges import _dev, _vp
from tests.test_resample_host import (TILE, assert_within, call_rs_host, design, frames_for, random_taps, ref_rs,
                                       windows_for)
from tests.test_select_ranges_host import U64

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POISON = 0x5A5A5A5A


@pytest.fixture(scope="module")
def gpu():
    if not gpu_available():
        pytest.skip("no GPU")
    import torch
    from birdnest.audio_amd import libflac
    return torch, libflac, libflac.BatchDecoder(0)


def _upload_pcm(torch, pcm):
    """exactly round_up(pcm_bytes, 16) bytes, the tail not zero"""
    return torch.from_numpy(np.concatenate([pcm, np.full(-len(pcm) % 16, 0xEE, np.uint8)])).to(DEV)


def _raw_rs(gpu, d_pcm, pcm_bytes, fmt, sp, win, spec, d_taps, R, pitch, flags, d_out, out_offset=0, win_offset=0,
            taps_offset=0, n=None):
    """bnflac_gather_ranges_f32_rs itself -> (rc, status[4]); the status starts as POISON"""
    torch, libflac, dec = gpu
    d_win = _dev(torch, win)
    d_st = torch.full((4,), POISON, dtype=torch.int32, device=DEV)
    rc = dec.L.bnflac_gather_ranges_f32_rs(dec.ctx, _vp(d_pcm), pcm_bytes, fmt, ctypes.byref(sp),
                                           ctypes.c_void_p(d_win.data_ptr() + win_offset), len(win) if n is None else n,
                                           ctypes.byref(spec), ctypes.c_void_p(d_taps.data_ptr() + taps_offset), R, pitch, flags,
                                           ctypes.c_void_p(d_out.data_ptr() + out_offset), _vp(d_st),
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, d_st.cpu().numpy().tolist()


def check(gpu, pcm, fmt, sp, win, spec, taps, R, pitch, flags, what, d_pcm=None, d_taps=None):
    """host twin within the yardstick's bound; device = host twin bit for bit, the same status, canaries kept"""
    torch, libflac, dec = gpu
    rc, host, host_st = call_rs_host(pcm, fmt, sp, win, spec, taps, R, pitch, flags)
    assert rc == 0, libflac.load().bnflac_last_error()
    ref = ref_rs(pcm, fmt, sp, win, spec, taps, R, pitch, flags)
    assert host_st == ref[3], what
    assert_within(host, ref, what + ", host twin")
    d_pcm = _upload_pcm(torch, pcm) if d_pcm is None else d_pcm
    d_taps = torch.from_numpy(np.ascontiguousarray(taps, np.float32).reshape(-1)).to(DEV) if d_taps is None else d_taps
    d_out = torch.full((len(host) + 64,), CANARY, dtype=torch.int32, device=DEV)
    rc, st = _raw_rs(gpu, d_pcm, len(pcm), fmt, sp, win, spec, d_taps, R, pitch, flags, d_out)
    assert rc == 0, dec.L.bnflac_last_error()
    got = d_out.cpu().numpy().view(np.uint32)
    assert_bits(got[: len(host)], host, what + ", device against the host twin")
    assert (got[len(host):] == CANARY).all(), what + ": a float was written behind the last plane"
    assert st == host_st, what
    return st


# (rate_in, rate_out) whose design has the ratio: 160/147, 147/160, 1/2, 3/2, 1/8, 1/1
RATIOS = [(147, 160), (160, 147), (2, 1), (2, 3), (8, 1), (1, 1)]
RATIO_IDS = ["160-147", "147-160", "1-2", "3-2", "1-8", "1-1"]


# ------------------------------------------------------------------ 1. tile seams x ratios
@pytest.mark.parametrize("R", [TILE - 1, TILE, TILE + 1, 2 * TILE + 3])
@pytest.mark.parametrize("rate_in,rate_out", RATIOS, ids=RATIO_IDS)
def test_rs_tile_seams(gpu, rate_in, rate_out, R):
    """FLACDECODER 16-bit stereo, planes and mono, an odd pitch, out_first 3: windows empty, shorter than
    the filter, two short of the row, filling it and cut.  1/8 (K = 256) works a tile in several steps."""
    torch, libflac, dec = gpu
    spec, taps = design(rate_in, rate_out)
    spec = spec.with_out_first(3)
    fmt, sp, stride, unit = layout("OUT_FLACDECODER", 2, 16)
    rng = np.random.default_rng(R + rate_in)
    nsmp = frames_for(R, spec)
    pcm = random_pcm(rng, nsmp * stride, unit, 16)
    win = windows_for(nsmp, R, spec)
    pitch = R + 1 + R % 2  # odd
    d_pcm = _upload_pcm(torch, pcm)
    for flags in (0, MONO):
        st = check(gpu, pcm, fmt, sp, win, spec, taps, R, pitch, flags, "R %d flags %d" % (R, flags), d_pcm=d_pcm)
        assert st[:2] == [0, 0] and st[2] >= 1


# ------------------------------------------------------------------ 2. the smallest and the largest tables
TABLES = [(160, 147, 4), (160, 147, 100), (147, 160, 4), (147, 160, 108), (1, 2, 4), (1, 2, 512), (3, 2, 4), (3, 2, 512),
          (1, 8, 4), (1, 8, 512), (1, 1, 512), (32, 3, 512), (4096, 1, 4), (2048, 3, 8), (1, 65535, 4)]


@pytest.mark.parametrize("up,down,K", TABLES, ids=["%d-%d-K%d" % t for t in TABLES])
def test_rs_table_sizes(gpu, up, down, K):
    """K = 4 and the largest K the table limit allows for the ratio; up * taps exactly 16384 three ways
    (the widest rows, the most rows, and rows that are padded in LDS: 96 KiB of table); a ratio so
    steep that a step is one output.  The taps are random: the contract is about their values."""
    torch, libflac, dec = gpu
    assert K == 4 or up * (K + 4) > 16384 or K == 512
    spec = libflac.ResampleSpec(up, down, K, 2)
    rng = np.random.default_rng(up * 7 + down + K)
    taps = random_taps(rng, up, K)
    fmt, sp, stride, unit = layout("OUT_FILEREADER", 2, 24)
    R = 301 if down < 100 * up else 9
    nsmp = frames_for(R, spec)
    pcm = random_pcm(rng, nsmp * stride, unit, 24)
    win = windows_for(nsmp, R, spec)
    for flags in (0, MONO):
        check(gpu, pcm, fmt, sp, win, spec, taps, R, R + 2, flags, "%d/%d K %d flags %d" % (up, down, K, flags))


# ------------------------------------------------------------------ 3. layouts x source phases
RS_LAYOUTS = [("OUT_INTERLEAVED32", 1, 32), ("OUT_INTERLEAVED32", 2, 16), ("OUT_INTERLEAVED32", 3, 20), ("OUT_INTERLEAVED32", 8, 24),
              ("OUT_FLACDECODER", 2, 16), ("OUT_FILEREADER", 1, 24), ("OUT_FILEREADER", 2, 24)]


@pytest.mark.parametrize("name,channels,bps", RS_LAYOUTS, ids=["%s-%dch-%d" % (f[4:], c, b) for f, c, b in RS_LAYOUTS])
def test_rs_layouts_and_source_phases(gpu, name, channels, bps):
    """pcm_first at every phase modulo 16 bytes the stride allows, planes and mono, 44100 -> 48000."""
    torch, libflac, dec = gpu
    spec, taps = design(44100, 48000)
    fmt, sp, stride, unit = layout(name, channels, bps)
    rng = np.random.default_rng(channels * 10 + unit)
    R = 150
    lens = [0, 5, 100, 137, 138, 160]  # 138 sample frames give 151 outputs
    pcm = random_pcm(rng, (17 + 160 + 8) * stride, unit, bps)
    win = window_table([(1 + k % 16, lens[k % len(lens)]) for k in range(32)])
    assert {int(w["pcm_first"]) * stride % 16 for w in win} == {p * stride % 16 for p in range(16)}
    d_pcm = _upload_pcm(torch, pcm)
    for flags in (0, MONO):
        st = check(gpu, pcm, fmt, sp, win, spec, taps, R, R + 3, flags, "%s flags %d" % (name, flags), d_pcm=d_pcm)
        assert st == [0, 0, sum(1 for w in win if -(-int(w["nsamples"]) * 160 // 147) > R), 0]


# ------------------------------------------------------------------ 4. out_first, empty, bad and cut windows
def test_rs_out_first_and_window_kinds(gpu):
    """out_first inside and past a window's outputs (a row of zeros); empty and bad windows (counted,
    never read: the PCM is allocated exactly, and a bad window's pcm_first points far outside); cut."""
    torch, libflac, dec = gpu
    spec, taps = design(2, 3)  # 3/2: a window of n sample frames has ceil(1.5 n) outputs
    assert (spec.up, spec.down) == (3, 2)
    fmt, sp, stride, unit = layout("OUT_FILEREADER", 2, 24)
    nsmp, R = 50, 40
    pcm = np.random.default_rng(4).integers(1, 256, nsmp * stride + 2, dtype=np.uint8)
    assert len(pcm) % stride and len(pcm) % 16
    win = window_table([(nsmp - 10, 10), (nsmp - 10, 11), (U64, 1), (U64, 0), (0, 0), (0, 30), (3, 47), (1 << 40, 5), (5, U64)])
    d_pcm = _upload_pcm(torch, pcm)
    for out_first, want_st in ((0, [1, 4, 2, 0]), (7, [1, 4, 1, 0]), (15, [1, 4, 1, 0]), (70, [1, 4, 0, 0]), (2 ** 31 - 1, [1, 4, 0, 0])):
        for flags in (0, MONO):
            st = check(gpu, pcm, fmt, sp, win, spec.with_out_first(out_first), taps, R, R + 1, flags,
                       "out_first %d flags %d" % (out_first, flags), d_pcm=d_pcm)
            assert st == want_st, (out_first, st)
    # nstreams 0 writes a zero status; row_out 0 counts the windows and writes no float
    d_taps = torch.from_numpy(taps.reshape(-1)).to(DEV)
    d_out = torch.full((64,), CANARY, dtype=torch.int32, device=DEV)
    assert _raw_rs(gpu, d_pcm, len(pcm), fmt, sp, win[:0], spec, d_taps, R, R, 0, d_out) == (0, [0, 0, 0, 0])
    assert _raw_rs(gpu, d_pcm, len(pcm), fmt, sp, win, spec, d_taps, 0, 3, 0, d_out) == (0, [1, 4, 3, 0])
    assert (d_out.cpu().numpy().view(np.uint32) == CANARY).all()


def test_rs_refusals(gpu):
    """A negative return and a message, nothing launched, nothing written."""
    torch, libflac, dec = gpu
    good, taps = design(3, 2)
    fmt, sp, stride, unit = layout("OUT_FILEREADER", 2, 24)
    R = 20
    pcm = np.random.default_rng(4).integers(1, 256, 50 * stride + 2, dtype=np.uint8)
    win = window_table([(0, 10), (5, 40), (U64, 1)])
    d_pcm = _upload_pcm(torch, pcm)
    d_taps = torch.zeros(16384 + 64, dtype=torch.float32, device=DEV)
    d_out = torch.full((3 * 2 * (R + 8),), CANARY, dtype=torch.int32, device=DEV)
    S = libflac.ResampleSpec

    def refused(word, fmt=fmt, sp=sp, R=R, pitch=R, flags=0, spec=good, d_pcm=d_pcm, **kw):
        rc, st = _raw_rs(gpu, d_pcm, len(pcm), fmt, sp, win, spec, d_taps, R, pitch, flags, d_out, **kw)
        assert rc < 0 and word in dec.L.bnflac_last_error(), (word, rc, dec.L.bnflac_last_error())
        assert st == [POISON] * 4 and (d_out.cpu().numpy().view(np.uint32) == CANARY).all(), word

    refused(b"1..65535", spec=S(0, 1, 4, 0))
    refused(b"1..65535", spec=S(1, 65536, 4, 0))
    refused(b"coprime", spec=S(4, 6, 4, 0))
    refused(b"multiple of 4", spec=S(3, 2, 6, 0))
    refused(b"multiple of 4", spec=S(3, 2, 516, 0))
    refused(b"16384", spec=S(4097, 2, 4, 0))
    refused(b"16384", spec=S(33, 2, 512, 0))
    refused(b"out_first", spec=S(3, 2, 4, 1 << 31))
    refused(b"row_out", R=1 << 31, pitch=1 << 31)
    refused(b"PLANAR32", fmt=libflac.OUT_PLANAR32)
    refused(b"bnflac_md5_layout", fmt=libflac.OUT_FLACDECODER)
    refused(b"bnflac_md5_layout", fmt=libflac.OUT_FILEREADER, sp=params(2, 20))
    refused(b"channels", fmt=libflac.OUT_INTERLEAVED32, sp=params(9, 24))
    refused(b"channels", sp=params(0, 24))
    refused(b"flags", flags=2)
    refused(b"plane_pitch", pitch=R - 1)
    refused(b"16-byte aligned", out_offset=4)
    refused(b"16-byte aligned", taps_offset=8)
    refused(b"16-byte aligned", d_pcm=d_pcm[8:])
    refused(b"8-byte aligned", win_offset=4)
    refused(b"too many streams", n=1 << 30)


# ------------------------------------------------------------------ 5. the wrapper and the chain
def test_rs_wrapper_writes_into_a_given_tensor(gpu):
    torch, libflac, dec = gpu
    spec, taps = design(48000, 44100)
    fmt, sp, stride, unit = layout("OUT_FLACDECODER", 2, 16)
    rng = np.random.default_rng(5)
    R, pitch = 777, 781
    pcm = random_pcm(rng, 1000 * stride, unit, 16)
    win = window_table([(3, 845), (9, 900), (0, 10)])
    d_out = torch.full((3 * 2 * pitch,), 7.0, dtype=torch.float32, device=DEV)
    planes, d_st = dec.gather_ranges_f32_rs(_upload_pcm(torch, pcm), fmt, sp, _dev(torch, win), 3, spec,
                                            torch.from_numpy(taps.reshape(-1)).to(DEV), R, d_out=d_out, plane_pitch=pitch,
                                            pcm_bytes=len(pcm))
    torch.cuda.synchronize()
    assert planes.data_ptr() == d_out.data_ptr() and tuple(planes.shape) == (3, 2, R)
    want, want_st = libflac.gather_ranges_f32_rs_host(pcm, fmt, sp, win, spec, taps, R)
    assert d_st.cpu().numpy().tolist() == want_st.tolist() == [0, 0, 1, 0]
    assert_bits(planes.contiguous().cpu().numpy().view(np.uint32).reshape(-1), np.ascontiguousarray(want).view(np.uint32).reshape(-1))
    assert (d_out.view(6, pitch)[:, R:] == 7.0).all()


@pytest.mark.parametrize("mono", [False, True], ids=["planes", "mono"])
def test_rs_chain_against_the_host_chain(gpu, mono):
    """decode_crops_f32_rs over three synthesised streams (12 frames of 4096 each) against
    resample_request -> the selection's clipping -> the host twin over the generator's PCM: crops at
    the start, in the middle (two of them overlapping), straddling the end, past it, and of a stream
    that is not there."""
    from birdnest.audio_amd import synth
    torch, libflac, dec = gpu
    syn = [synth.encode(synth.config("C2", nframes=12, seed=31 + i)) for i in range(3)]
    datas = [s.data.tobytes() for s in syn]
    buf, ranges = _pack(datas, (7, 2))
    sp = _stream_params(libflac, datas[0], 0)
    rate_out = 48000 if sp.sample_rate != 48000 else 44100
    corpus = dec.index_corpus(_upload(torch, buf), len(buf), ranges, sp)
    spec, taps = libflac.resample_design(sp.sample_rate, rate_out)
    T = int(syn[0].nsamples)
    total = -(-T * spec.up // spec.down)
    N = 1500
    crops = [(0, 0), (1, 20000), (1, 20000 + spec.up * 3), (2, 20777), (0, total - 700), (2, total + 10), (1, spec.up * 100), (5, 0)]
    planes, status = dec.decode_crops_f32_rs(corpus, crops, N, rate_out, mono=mono)
    torch.cuda.synchronize()
    assert planes.dtype == torch.float32 and tuple(planes.shape) == (len(crops), 1 if mono else sp.channels, N)
    got = planes.contiguous().cpu().numpy().view(np.uint32)
    isp = params(sp.channels, sp.bps)
    for k, (t, j0) in enumerate(crops):
        want = np.zeros((1 if mono else sp.channels, N), np.uint32)
        if t < 3:
            first, n, out_first = libflac.resample_request(spec, j0, N)
            lo = min(first, T)
            hi = min(lo + n, T)
            x = np.ascontiguousarray(syn[t].pcm[lo:hi], dtype="<i4").reshape(-1).view(np.uint8)
            rows, st = libflac.gather_ranges_f32_rs_host(x, libflac.OUT_INTERLEAVED32, isp, window_table([(0, hi - lo)]),
                                                         spec.with_out_first(out_first), taps, N, mono=mono)
            want = np.ascontiguousarray(rows[0]).view(np.uint32)
        assert_bits(got[k].reshape(-1), want.reshape(-1), "crop %d" % k)
    assert got[0].any() and got[4][:, :700].any() and not got[4][:, 700:].any() and not got[5].any()
    assert status["gather"].cpu().numpy().tolist()[:2] == [0, 0] and status["select"].cpu().numpy().tolist()[0] & 1 == 0
