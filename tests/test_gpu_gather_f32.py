"""bnflac_gather_ranges_f32 on the device: windows of a decoded selection as float32 channel planes.

References, all independent of the code under test: `ref_f32` (the formulas in numpy) and the
host twin from tests/test_gather_f32_host.py; the generator's PCM for the whole chain; today's
route (gather_ranges on an INTERLEAVED32 decode, then torch) for the same tensor.  Every comparison
of floats is on the bit pattern.
"""
import ctypes

import numpy as np
import pytest

from tests.conftest import gpu_available
from tests.test_gather_f32_host import (CANARY, LAYOUT_IDS, LAYOUTS, MONO, _edge_case, assert_bits, call_host, layout, params,
                                        random_pcm, ref_f32, window_table)
from tests.test_gpu_index_streams import Batch, _first_frame_offset, _mixed, _pack, _stream_params
from tests.test_gpu_select_ranges import _dev, _vp, _windows_of_batch

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


def _canaries(torch, n):
    return torch.full((n,), CANARY, dtype=torch.int32, device=DEV)  # 0x7FC5A5A5 fits an int32


def _raw_f32(gpu, d_pcm, pcm_bytes, fmt, sp, win, R, pitch, flags, d_out, out_offset=0, win_offset=0, n=None):
    """bnflac_gather_ranges_f32 itself -> (rc, status[4]); the status starts as POISON"""
    torch, libflac, dec = gpu
    d_win = _dev(torch, win)
    d_st = torch.full((4,), POISON, dtype=torch.int32, device=DEV)
    rc = dec.L.bnflac_gather_ranges_f32(dec.ctx, _vp(d_pcm), pcm_bytes, fmt, ctypes.byref(sp),
                                        ctypes.c_void_p(d_win.data_ptr() + win_offset), len(win) if n is None else n, R, pitch,
                                        flags, ctypes.c_void_p(d_out.data_ptr() + out_offset), _vp(d_st),
                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, d_st.cpu().numpy().tolist()


# ------------------------------------------------------------------ 1. the kernel alone: device = host twin = numpy
@pytest.mark.parametrize("R", [1, 1000, 4099])
@pytest.mark.parametrize("name,channels,bps", LAYOUTS, ids=LAYOUT_IDS)
def test_f32_alignment_sweep(gpu, name, channels, bps, R):
    """Every source phase the stride allows x every destination phase x every length class, both
    flags, the floats between planes and behind the last one untouched.  The kernel's tile is at
    most 2,048 sample frames (bnf_f32_tile_frames), so R = 4099 takes three tiles of every layout
    and no longer row is needed."""
    torch, libflac, dec = gpu
    fmt, sp, stride, unit = layout(name, channels, bps)
    rng = np.random.default_rng(R * 100 + channels * 10 + unit)
    lengths = sorted({0, 1, 3, 4, 5, R - 1, R, R + 3})
    nsmp = 16 + max(lengths) + 8  # sample frames of the PCM: every window lies inside
    pcm = random_pcm(rng, nsmp * stride, unit, bps)
    d_pcm = torch.from_numpy(np.concatenate([pcm, np.full(-len(pcm) % 16, 0xEE, np.uint8)])).to(DEV)
    win = window_table([(1 + k % 16, lengths[k // 16]) for k in range(16 * len(lengths))])
    assert {int(w["pcm_first"]) * stride % 16 for w in win} == {p * stride % 16 for p in range(16)}
    for flags in (0, MONO):
        planes = 1 if flags else channels
        for pitch in (R, R + 5):
            if pitch % 2:  # an odd pitch: the planes start at every phase modulo 4 floats
                assert {q * pitch % 4 for q in range(len(win) * planes)} == {0, 1, 2, 3}
            want, want_st = ref_f32(pcm, fmt, sp, win, R, pitch, flags)
            rc, host, host_st = call_host(pcm, fmt, sp, win, R, pitch, flags)
            assert rc == 0 and host_st == want_st
            assert_bits(host, want, "host twin, flags %d pitch %d" % (flags, pitch))
            d_out = _canaries(torch, len(want) + 64)
            rc, st = _raw_f32(gpu, d_pcm, len(pcm), fmt, sp, win, R, pitch, flags, d_out)
            assert rc == 0, dec.L.bnflac_last_error()
            assert st == want_st == [0, 0, sum(1 for w in win if w["nsamples"] > R), 0]
            got = d_out.cpu().numpy().view(np.uint32)
            assert_bits(got[: len(want)], want, "device, flags %d pitch %d" % (flags, pitch))
            assert (got[len(want):] == CANARY).all(), "a float was written behind the last plane"


# ------------------------------------------------------------------ 2. status and refusals
def test_f32_windows_past_the_pcm_and_refusals(gpu):
    torch, libflac, dec = gpu
    fmt, sp, stride, pcm, win, R, nsmp = _edge_case()
    d_pcm = torch.from_numpy(np.concatenate([pcm, np.full(-len(pcm) % 16, 0xEE, np.uint8)])).to(DEV)
    for flags in (0, MONO):
        want, want_st = ref_f32(pcm, fmt, sp, win, R, R + 1, flags)
        d_out = _canaries(torch, len(want) + 16)
        rc, st = _raw_f32(gpu, d_pcm, len(pcm), fmt, sp, win, R, R + 1, flags, d_out)
        assert rc == 0 and st == want_st == [1, 2, 0, 0]
        got = d_out.cpu().numpy().view(np.uint32)
        assert_bits(got[: len(want)], want)
        assert (got[len(want):] == CANARY).all()
    # nstreams 0 writes a zero status; row_samples 0 counts the windows and writes no float
    d_out = _canaries(torch, 64)
    assert _raw_f32(gpu, d_pcm, len(pcm), fmt, sp, win[:0], R, R, 0, d_out) == (0, [0, 0, 0, 0])
    assert _raw_f32(gpu, d_pcm, len(pcm), fmt, sp, win, 0, 3, 0, d_out) == (0, [1, 2, 1, 0])
    assert (d_out.cpu().numpy().view(np.uint32) == CANARY).all()

    # refusals: a negative return and a message, nothing launched, nothing written
    d_out = _canaries(torch, 4 * 2 * (R + 8))

    def refused(word, fmt=fmt, sp=sp, pitch=R, flags=0, out_offset=0, d_pcm=d_pcm, **kw):
        rc, st = _raw_f32(gpu, d_pcm, len(pcm), fmt, sp, win, R, pitch, flags, d_out, out_offset, **kw)
        assert rc < 0 and word in dec.L.bnflac_last_error(), (word, rc, dec.L.bnflac_last_error())
        assert st == [POISON] * 4 and (d_out.cpu().numpy().view(np.uint32) == CANARY).all(), word

    refused(b"PLANAR32", fmt=libflac.OUT_PLANAR32)
    refused(b"bnflac_md5_layout", fmt=libflac.OUT_FLACDECODER)
    refused(b"bnflac_md5_layout", fmt=libflac.OUT_FILEREADER, sp=params(2, 20))
    refused(b"channels", fmt=libflac.OUT_INTERLEAVED32, sp=params(9, 24))
    refused(b"channels", sp=params(0, 24))
    refused(b"flags", flags=2)
    refused(b"plane_pitch", pitch=R - 1)
    refused(b"16-byte aligned", out_offset=4)
    refused(b"16-byte aligned", d_pcm=d_pcm[8:])
    refused(b"8-byte aligned", win_offset=4)
    refused(b"too many streams", n=1 << 30)


# ------------------------------------------------------------------ 3. the chain against the generator
_F32_BATCHES = {}


def _f32_batch(gpu, name):
    """name -> (d_bytes, nbytes, [(begin, end)] of the files, the index as a Batch, the streams' PCM or
    None, sp); computed once.  C2: the five streams of tests/test_gpu_index_streams.py (one of them
    empty); C4 / C3 / C5: three streams of 40 / 16 / 8 frames; M1: three one-channel streams."""
    if name not in _F32_BATCHES:
        from birdnest.audio_amd import synth
        torch, libflac, dec = gpu
        if name == "C2":
            m = _mixed(gpu)
            syn, buf, table, sp = m["syn"], m["buf"], m["table"], _stream_params(libflac, m["datas"][0], 0)
        else:
            cfg = {"C4": ("C4", dict(nframes=40)), "C3": ("C3", dict(nframes=16)), "C5": ("C5", dict(nframes=8)),
                   "M1": ("C2", dict(channels=1, nframes=12))}[name]
            syn = [synth.encode(synth.config(cfg[0], seed=5 + 100 * i, **cfg[1])) for i in range(3)]
            datas = [s.data.tobytes() for s in syn]
            buf, ranges = _pack(datas, (3, 0))
            table = [(b, e, b + _first_frame_offset(d), _stream_params(libflac, d).total_samples)
                     for (b, e), d in zip(ranges, datas)]
            sp = _stream_params(libflac, datas[0], 0)
        b = Batch(gpu, buf, table, sp)
        assert b.status[0] == 0
        _F32_BATCHES[name] = (b.d_bytes, len(buf), [(t[0], t[1]) for t in table], b,
                              [s.pcm if s is not None else None for s in syn], sp)
    return _F32_BATCHES[name]


def _pcm_ref(pcms, sp, ranges, R, mono):
    """ref_f32 over the generator's PCM: stream s's window of its own samples, as INTERLEAVED32 bytes."""
    rows = []
    for pcm, (first, want) in zip(pcms, ranges):
        T = len(pcm) if pcm is not None else 0
        lo = min(first, T)
        hi = min(lo + want, T)
        x = np.ascontiguousarray(pcm[lo:hi], dtype="<i4").reshape(-1).view(np.uint8) if hi > lo else np.zeros(0, np.uint8)
        isp = params(sp.channels, sp.bps)
        bits, st = ref_f32(x, 1, isp, window_table([(0, hi - lo)]), R, R, MONO if mono else 0)  # 1: OUT_INTERLEAVED32
        assert st == [0, 0, 0, 0]
        rows.append(bits.reshape(-1, R))
    return np.stack(rows)


@pytest.mark.parametrize("mono", [False, True], ids=["planes", "mono"])
@pytest.mark.parametrize("name,fmt_name", [("C2", "OUT_FLACDECODER"), ("C3", "OUT_FILEREADER"), ("C4", "OUT_FLACDECODER"),
                                           ("C5", "OUT_FILEREADER"), ("M1", "OUT_FLACDECODER"), ("C2", "OUT_INTERLEAVED32")])
def test_f32_chain_against_the_generator(gpu, name, fmt_name, mono):
    """decode_windows_f32 with fmt=None picks fmt_name (the narrowest layout); the last case passes
    OUT_INTERLEAVED32 itself, so the chain runs through all three layouts."""
    torch, libflac, dec = gpu
    d_bytes, nbytes, files, b, pcms, sp = _f32_batch(gpu, name)
    assert libflac.OUT_INTERLEAVED32 == 1
    explicit = fmt_name == "OUT_INTERLEAVED32"
    if not explicit:
        assert libflac.f32_layout(sp) == getattr(libflac, fmt_name)
    n = len(files)
    for shift in (0, 5):
        ranges = _windows_of_batch(b, shift)
        R = max(1, max(min(w, int(b.ss[s + 1] - b.ss[s])) for s, (_, w) in enumerate(ranges)))
        windows = [(f, min(w, R)) for f, w in ranges]
        planes, status = dec.decode_windows_f32(d_bytes, nbytes, files, windows, R, sp, mono=mono,
                                                fmt=libflac.OUT_INTERLEAVED32 if explicit else None)
        torch.cuda.synchronize()
        assert planes.dtype == torch.float32 and tuple(planes.shape) == (n, 1 if mono else sp.channels, R)
        st = {k: v.cpu().numpy().tolist() for k, v in status.items()}
        assert st["gather"] == [0, 0, 0, 0] and st["index"][0] == 0 and st["select"][0] == 0
        empty = sum(1 for p in pcms if p is None)
        assert st["scan"][0] == (1 if empty else 0) and st["scan"][1] == n - empty
        got = planes.contiguous().cpu().numpy().view(np.uint32)
        want = _pcm_ref(pcms, sp, windows, R, mono)
        for s in range(n):
            assert_bits(got[s].reshape(-1), want[s].reshape(-1), "%s shift %d stream %d" % (name, shift, s))


# ------------------------------------------------------------------ 4. today's route gives the same tensor
@pytest.mark.parametrize("name", ["C2", "C3"])
def test_f32_equals_gather_ranges_then_torch(gpu, name):
    torch, libflac, dec = gpu
    d_bytes, nbytes, files, b, pcms, sp = _f32_batch(gpu, name)
    n = len(files)
    ranges = _windows_of_batch(b, 4)
    R = 3000
    windows = [(f, min(w, R)) for f, w in ranges]
    rows, st_a = dec.decode_windows(d_bytes, nbytes, files, windows, R, sp, libflac.OUT_INTERLEAVED32)
    a = rows.view(torch.int32).view(n, R, sp.channels).permute(0, 2, 1).to(torch.float32) * (2.0 ** -(sp.bps - 1))
    bplanes, st_b = dec.decode_windows_f32(d_bytes, nbytes, files, windows, R, sp)
    torch.cuda.synchronize()
    assert st_a["gather"].cpu().numpy().tolist() == st_b["gather"].cpu().numpy().tolist() == [0, 0, 0, 0]
    assert a.dtype == torch.float32 and a.shape == bplanes.shape
    assert_bits(bplanes.contiguous().cpu().numpy().view(np.uint32).reshape(-1),
                a.contiguous().cpu().numpy().view(np.uint32).reshape(-1), name)
    assert bplanes.abs().max().item() > 0.01


def test_f32_wrapper_writes_into_a_given_tensor(gpu):
    """gather_ranges_f32 with d_out and an odd plane_pitch: the result is a view of d_out."""
    torch, libflac, dec = gpu
    fmt, sp, stride, unit = layout("OUT_FLACDECODER", 2, 16)
    rng = np.random.default_rng(5)
    R, pitch = 777, 781
    pcm = random_pcm(rng, (R + 40) * stride, unit, 16)
    win = window_table([(3, R), (9, R + 5), (0, 10)])
    d_pcm = torch.from_numpy(np.concatenate([pcm, np.zeros(-len(pcm) % 16, np.uint8)])).to(DEV)
    d_out = torch.full((3 * 2 * pitch,), 7.0, dtype=torch.float32, device=DEV)
    planes, d_st = dec.gather_ranges_f32(d_pcm, fmt, sp, _dev(torch, win), 3, R, d_out=d_out, plane_pitch=pitch,
                                         pcm_bytes=len(pcm))
    torch.cuda.synchronize()
    assert planes.data_ptr() == d_out.data_ptr() and tuple(planes.shape) == (3, 2, R)
    assert d_st.cpu().numpy().tolist() == [0, 0, 1, 0]
    want, _ = ref_f32(pcm, fmt, sp, win, R, R, 0)
    assert_bits(planes.contiguous().cpu().numpy().view(np.uint32).reshape(-1), want)
    assert (d_out.view(6, pitch)[:, R:] == 7.0).all()
