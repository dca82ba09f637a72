"""bnflac_gather_ranges_mel on the device: windows of a decoded selection as mel (or power)
spectrogram planes.

Every result is compared bit for bit (uint32 view) with the host twin (bnflac_gather_ranges_mel_host,
which tests/test_mel_host.py holds against the float64 yardstick and its derived bound), and status
word for status word.  The output starts as a sentinel, and every float the contract leaves alone
keeps it.  The shapes are the smallest at which the kernel takes another path: rows round the tile of
libflac.MEL_TILE frames, hops that give one step or several per tile and one frame per step, FFT
sizes with an even and an odd number of stages and with four, two and one frame in flight, every
layout, every source phase modulo 16 bytes and every destination phase modulo 4 floats.
"""
import ctypes

import numpy as np
import pytest

from tests.conftest import gpu_available
from tests.test_gather_f32_host import CANARY, MONO, assert_bits, layout, params, random_pcm, window_table
from tests.test_gpu_index_streams import _pack, _stream_params, _upload
from tests.test_gpu_select_ranges import _dev, _vp
from tests.test_mel_host import TF, call_mel_host, checked_bands, design, frames_needed, n_valid_of, random_tables, windows_for
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


def _raw_mel(gpu, d_pcm, pcm_bytes, fmt, sp, win, spec, d_tab, d_bands, R, pitch, flags, d_out, out_offset=0, win_offset=0,
             tab_offset=0, bands_offset=0, n=None):
    """bnflac_gather_ranges_mel itself -> (rc, status[4]); the status starts as POISON"""
    torch, libflac, dec = gpu
    d_win = _dev(torch, win)
    d_st = torch.full((4,), POISON, dtype=torch.int32, device=DEV)
    rc = dec.L.bnflac_gather_ranges_mel(dec.ctx, _vp(d_pcm), pcm_bytes, fmt, ctypes.byref(sp),
                                        ctypes.c_void_p(d_win.data_ptr() + win_offset), len(win) if n is None else n,
                                        ctypes.byref(spec), ctypes.c_void_p(d_tab.data_ptr() + tab_offset),
                                        ctypes.c_void_p(d_bands.data_ptr() + bands_offset) if d_bands is not None else None,
                                        R, pitch, flags, ctypes.c_void_p(d_out.data_ptr() + out_offset), _vp(d_st),
                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, d_st.cpu().numpy().tolist()


def _tables(torch, tab, bands, spec):
    d_tab = torch.from_numpy(np.ascontiguousarray(tab, np.float32).reshape(-1)).to(DEV)
    d_bands = _dev(torch, np.ascontiguousarray(bands, np.uint32).reshape(-1)) if spec.n_mels else None
    return d_tab, d_bands


def check(gpu, pcm, fmt, sp, win, spec, tab, bands, R, pitch, flags, what, d_pcm=None, lead=0):
    """device = host twin bit for bit, the same status, the sentinel kept in front of d_out, between the
    rows and behind the last one.  lead: floats in front of d_out (a multiple of 4)."""
    torch, libflac, dec = gpu
    rc, host, host_st = call_mel_host(pcm, fmt, sp, win, spec, tab, bands if spec.n_mels else None, R, pitch, flags)
    assert rc == 0, libflac.load().bnflac_last_error()
    d_pcm = _upload_pcm(torch, pcm) if d_pcm is None else d_pcm
    d_tab, d_bands = _tables(torch, tab, bands, spec)
    d_out = torch.full((lead + len(host) + 64,), CANARY, dtype=torch.int32, device=DEV)
    rc, st = _raw_mel(gpu, d_pcm, len(pcm), fmt, sp, win, spec, d_tab, d_bands, R, pitch, flags, d_out, out_offset=4 * lead)
    assert rc == 0, dec.L.bnflac_last_error()
    got = d_out.cpu().numpy().view(np.uint32)
    assert (got[:lead] == CANARY).all(), what + ": a float was written in front of d_out"
    assert_bits(got[lead: lead + len(host)], host, what + ", device against the host twin")
    assert (got[lead + len(host):] == CANARY).all(), what + ": a float was written behind the last row"
    assert st == host_st, what
    return st, host


LAYOUTS = [("OUT_FLACDECODER", 2, 16), ("OUT_FILEREADER", 2, 24), ("OUT_INTERLEAVED32", 8, 24), ("OUT_FILEREADER", 1, 24)]


# ------------------------------------------------------------------ 1. layouts x FFT sizes, planes and mono
@pytest.mark.parametrize("n_fft", [64, 256, 2048])
@pytest.mark.parametrize("name,channels,bps", LAYOUTS, ids=["%s-%dch-%d" % (f[4:], c, b) for f, c, b in LAYOUTS])
def test_mel_layouts_and_sizes(gpu, name, channels, bps, n_fft):
    """40 bands, hop n_fft / 4, rows a little longer than a tile (2048: a few frames), an odd pitch:
    windows empty, of one sample, of n_fft - 1, n_fft, two hops short of the row, filling it and cut."""
    torch, libflac, dec = gpu
    spec, tab, bands = design(48000, n_fft, n_fft // 4, 40)
    fmt, sp, stride, unit = layout(name, channels, bps)
    rng = np.random.default_rng(n_fft + channels)
    R = TF + 3 if n_fft < 2048 else 7
    nsmp = frames_needed(R, spec)
    pcm = random_pcm(rng, nsmp * stride + 1, unit, bps)
    win = windows_for(nsmp, R, spec)
    d_pcm = _upload_pcm(torch, pcm)
    for flags in (0, MONO):
        st, _ = check(gpu, pcm, fmt, sp, win, spec, tab, bands, R, R + 1 + R % 2, flags, "%s N %d flags %d" % (name, n_fft, flags),
                      d_pcm=d_pcm)
        assert st[:2] == [0, 0] and st[2] >= 1 and st[3] == 0


# ------------------------------------------------------------------ 2. hops x tile seams
@pytest.mark.parametrize("R", [TF - 1, TF, TF + 1, 3 * TF + 5])
@pytest.mark.parametrize("hop", [1, 37, 32, 200], ids=["hop1", "hop37", "hopN/4", "hop>N"])
def test_mel_hops_and_tile_seams(gpu, hop, R):
    """n_fft 128 (an odd number of stages), 24-bit stereo: hop 1 and 37 work a tile in one step, 200
    (above n_fft, gaps between the frames) in several; rows end one frame short of a tile, on its
    seam, one behind it and in the fourth tile."""
    torch, libflac, dec = gpu
    spec, tab, bands = design(44100, 128, hop, 20)
    fmt, sp, stride, unit = layout("OUT_FILEREADER", 2, 24)
    rng = np.random.default_rng(hop * 1000 + R)
    nsmp = frames_needed(R, spec)
    pcm = random_pcm(rng, nsmp * stride, unit, 24)
    win = windows_for(nsmp, R, spec)
    d_pcm = _upload_pcm(torch, pcm)
    for flags in (0, MONO):
        st, _ = check(gpu, pcm, fmt, sp, win, spec, tab, bands, R, R + 1, flags, "hop %d R %d flags %d" % (hop, R, flags), d_pcm=d_pcm)
        assert st[:2] == [0, 0] and st[2] >= 1


def test_mel_steps_of_a_large_fft(gpu):
    """n_fft 1024, hop 256, 16-bit stereo (the shape of tools/gather_mel_bench.py): two frames in flight,
    several steps per tile; and n_fft 2048 at 8 channels of int32, where a step is one frame."""
    torch, libflac, dec = gpu
    rng = np.random.default_rng(77)
    for (n_fft, hop, n_mels, name, channels, bps, R) in ((1024, 256, 128, "OUT_FLACDECODER", 2, 16, TF + 2),
                                                        (2048, 512, 256, "OUT_INTERLEAVED32", 8, 24, 3)):
        spec, tab, bands = design(48000, n_fft, hop, n_mels)
        fmt, sp, stride, unit = layout(name, channels, bps)
        nsmp = frames_needed(R, spec)
        pcm = random_pcm(rng, nsmp * stride, unit, bps)
        win = windows_for(nsmp, R, spec)[[0, 2, -2, -1]]  # empty, a short one, the longest that is not cut, cut
        check(gpu, pcm, fmt, sp, win, spec, tab, bands, R, R, 0, "N %d" % n_fft)


# ------------------------------------------------------------------ 3. the destination's alignment
@pytest.mark.parametrize("pitch_extra,lead", [(0, 0), (1, 4), (2, 8), (3, 12), (4, 0)])
def test_mel_row_start_alignments(gpu, pitch_extra, lead):
    """row_frames 36 and frame_pitch 36 .. 40, d_out at several 16-byte offsets of its allocation: the
    row starts are 16-byte aligned, or 4- and 8-byte aligned in turn, so every phase of the split into
    aligned groups and single floats is taken at both ends of a tile."""
    torch, libflac, dec = gpu
    spec, tab, bands = design(48000, 64, 16, 7)
    fmt, sp, stride, unit = layout("OUT_FLACDECODER", 2, 16)
    R = 36
    pitch = R + pitch_extra
    nsmp = frames_needed(R, spec)
    pcm = random_pcm(np.random.default_rng(pitch), nsmp * stride, unit, 16)
    win = windows_for(nsmp, R, spec)
    st, host = check(gpu, pcm, fmt, sp, win, spec, tab, bands, R, pitch, 0, "pitch %d lead %d" % (pitch, lead), lead=lead)
    assert {(r * pitch) % 4 for r in range(8)} == ({0} if pitch % 4 == 0 else {0, 2} if pitch % 2 == 0 else {0, 1, 2, 3})


# ------------------------------------------------------------------ 4. the source's alignment
@pytest.mark.parametrize("name,channels,bps", [("OUT_FLACDECODER", 1, 16), ("OUT_FLACDECODER", 2, 16), ("OUT_FILEREADER", 1, 24),
                                               ("OUT_FILEREADER", 2, 24), ("OUT_INTERLEAVED32", 3, 20)],
                         ids=["FD-1ch", "FD-2ch", "FR-1ch-24", "FR-2ch-24", "I32-3ch"])
def test_mel_source_phases(gpu, name, channels, bps):
    """pcm_first at every phase modulo 16 bytes the stride allows (2- and 3-byte samples: every byte
    alignment of the compact PCM), windows of 0, 1, n_fft - 1 and a few thousand samples in one launch."""
    torch, libflac, dec = gpu
    spec, tab, bands = design(48000, 64, 50, 12)
    fmt, sp, stride, unit = layout(name, channels, bps)
    rng = np.random.default_rng(channels * 10 + unit)
    R = 40
    lens = [0, 1, 63, 3000, 64, 1950]
    pcm = random_pcm(rng, (17 + 3000 + 8) * stride + 1, unit, bps)
    win = window_table([(1 + k % 16, lens[k % len(lens)]) for k in range(32)])
    assert {int(w["pcm_first"]) * stride % 16 for w in win} == {p * stride % 16 for p in range(16)}
    d_pcm = _upload_pcm(torch, pcm)
    for flags in (0, MONO):
        st, _ = check(gpu, pcm, fmt, sp, win, spec, tab, bands, R, R + 3, flags, "%s flags %d" % (name, flags), d_pcm=d_pcm)
        assert st == [0, 0, sum(1 for w in win if n_valid_of(int(w["nsamples"]), spec) > R), 0] and st[2] > 0


# ------------------------------------------------------------------ 5. window kinds, origins, bad windows
def test_mel_window_kinds_and_origins(gpu):
    """A bad window between good ones (counted, never read: the PCM is allocated exactly, and a bad
    window's pcm_first points far outside), empty windows, origins in front of, inside and past the
    windows; nstreams 0 and 1; row_frames 0."""
    torch, libflac, dec = gpu
    d, tab, bands = design(48000, 128, 48, 12)
    fmt, sp, stride, unit = layout("OUT_FILEREADER", 2, 24)
    nsmp, R = 700, 13
    pcm = np.random.default_rng(4).integers(1, 256, nsmp * stride + 2, dtype=np.uint8)
    assert len(pcm) % stride and len(pcm) % 16
    win = window_table([(nsmp - 100, 100), (nsmp - 100, 101), (3, 600), (U64, 1), (U64, 0), (0, 0), (0, 127), (1 << 40, 5), (5, U64),
                        (9, 128)])
    d_pcm = _upload_pcm(torch, pcm)
    for origin in (-64, 0, 31, 650, -129, -1000, 2 ** 31 - 1, -2 ** 31):
        for flags in (0, MONO):
            st, _ = check(gpu, pcm, fmt, sp, win, d.with_origin(origin), tab, bands, R, R + 1, flags,
                          "origin %d flags %d" % (origin, flags), d_pcm=d_pcm)
            assert st[:2] == [1, 4] and st[3] == 0
    d_tab, d_bands = _tables(torch, tab, bands, d)
    d_out = torch.full((4096,), CANARY, dtype=torch.int32, device=DEV)
    assert _raw_mel(gpu, d_pcm, len(pcm), fmt, sp, win[:0], d, d_tab, d_bands, R, R, 0, d_out) == (0, [0, 0, 0, 0])
    assert _raw_mel(gpu, d_pcm, len(pcm), fmt, sp, win, d, d_tab, d_bands, 0, 3, 0, d_out) == (0, [1, 4, 4, 0])
    assert (d_out.cpu().numpy().view(np.uint32) == CANARY).all()
    st, host = check(gpu, pcm, fmt, sp, win[2:3], d, tab, bands, R, R, 0, "one window", d_pcm=d_pcm)
    assert st == [0, 0, 0, 0] and host.view(np.float32).all()


# ------------------------------------------------------------------ 6. band counts, tables that are no design, bad bands
@pytest.mark.parametrize("n_mels", [0, 1, 40, 256])
@pytest.mark.parametrize("n_fft", [64, 1024])
def test_mel_band_counts(gpu, n_fft, n_mels):
    """n_mels 0 (the power spectrum: 33 and 513 rows), 1, 40 and 256, with a random window, random
    weights (some negative) and bands at random places: the contract is about the tables' values."""
    torch, libflac, dec = gpu
    rng = np.random.default_rng(n_fft + n_mels)
    d, dtab, _ = design(48000, n_fft, n_fft // 2, 0)
    if n_mels:
        spec, tab, bands = random_tables(rng, d, dtab, n_mels, min(8192, 20 * n_mels + 13))
    else:
        spec, tab, bands = d, np.concatenate([rng.standard_normal(n_fft).astype(np.float32), dtab[n_fft:]]), None
    fmt, sp, stride, unit = layout("OUT_FLACDECODER", 2, 16)
    R = TF + 1 if n_fft == 64 else 5
    nsmp = frames_needed(R, spec)
    pcm = random_pcm(rng, nsmp * stride, unit, 16)
    win = windows_for(nsmp, R, spec)
    for flags in (0, MONO):
        st, _ = check(gpu, pcm, fmt, sp, win, spec, tab, bands, R, R + 2, flags, "N %d mels %d flags %d" % (n_fft, n_mels, flags))
        assert st[3] == 0 and st[0] == 0


def test_mel_power_rows_in_two_passes(gpu):
    """n_fft 2048 without bands: 1,025 rows go out in two passes of 520."""
    torch, libflac, dec = gpu
    spec, tab, _ = design(48000, 2048, 1000, 0)
    fmt, sp, stride, unit = layout("OUT_FLACDECODER", 2, 16)
    R = 3
    nsmp = frames_needed(R, spec)
    pcm = random_pcm(np.random.default_rng(2), nsmp * stride, unit, 16)
    check(gpu, pcm, fmt, sp, windows_for(nsmp, R, spec)[[1, -2, -1]], spec, tab, None, R, R + 1, 0, "1025 rows")


def test_mel_bad_bands(gpu):
    """Bands that descend, run past n_weights or past the last bin, and a table of 0xffffffff: zero
    rows, counted once per launch (8 windows, 40 frames each), status bit 1."""
    torch, libflac, dec = gpu
    d, tab, bands = design(48000, 128, 32, 8)
    fmt, sp, stride, unit = layout("OUT_FLACDECODER", 2, 16)
    pcm = random_pcm(np.random.default_rng(8), 1400 * stride, unit, 16)
    win = window_table([(k, 1300) for k in range(8)])
    b = bands.copy()
    b[2, 1] = b[3, 1] + 1
    b[5, 0] = 65 - 1
    b[8, 1] = d.n_weights + 1
    nbad = checked_bands(d, b)[1]
    assert nbad >= 3
    st, host = check(gpu, pcm, fmt, sp, win, d, tab, b, 40, 40, 0, "bad bands")
    assert st == [2, 0, 8, nbad] and host.reshape(8, 2, 8, 40)[:, :, 0, :].all() and not host.reshape(8, 2, 8, 40)[:, :, [2, 5, 7], :].any()
    st, host = check(gpu, pcm, fmt, sp, win, d, tab, np.full_like(b, 0xFFFFFFFF), 40, 40, 0, "bands of 0xffffffff")
    assert st == [2, 0, 8, 8] and not host.any()
    win[3] = (U64, 7, 0, 0, 0, 0)
    st, host = check(gpu, pcm, fmt, sp, win, d, tab, b, 40, 40, MONO, "bad bands and a bad window")
    assert st == [3, 1, 7, nbad]


# ------------------------------------------------------------------ 7. refusals
def test_mel_refusals(gpu):
    """A negative return and a message, nothing launched, nothing written."""
    torch, libflac, dec = gpu
    good, tab, bands = design(48000, 64, 16, 8)
    fmt, sp, stride, unit = layout("OUT_FILEREADER", 2, 24)
    R = 20
    pcm = np.random.default_rng(4).integers(1, 256, 900 * stride + 2, dtype=np.uint8)
    win = window_table([(0, 10), (5, 800), (U64, 1)])
    d_pcm = _upload_pcm(torch, pcm)
    d_tab = torch.zeros(2 * 2048 + 8192 + 64, dtype=torch.float32, device=DEV)
    d_bands = torch.zeros(2 * 258, dtype=torch.int32, device=DEV)
    d_out = torch.full((3 * 2 * 8 * (R + 8),), CANARY, dtype=torch.int32, device=DEV)
    S = lambda n_fft=64, hop=16, n_mels=8, origin=-32, n_weights=good.n_weights, reserved=(0, 0, 0): libflac.MelSpec(
        n_fft, hop, n_mels, origin, n_weights, (ctypes.c_uint32 * 3)(*reserved))

    def refused(word, fmt=fmt, sp=sp, R=R, pitch=R, flags=0, spec=good, d_pcm=d_pcm, d_tab=d_tab, d_bands=d_bands, **kw):
        rc, st = _raw_mel(gpu, d_pcm, len(pcm), fmt, sp, win, spec, d_tab, d_bands, R, pitch, flags, d_out, **kw)
        assert rc < 0 and word in dec.L.bnflac_last_error(), (word, rc, dec.L.bnflac_last_error())
        assert st == [POISON] * 4 and (d_out.cpu().numpy().view(np.uint32) == CANARY).all(), word

    refused(b"power of two", spec=S(n_fft=32))
    refused(b"power of two", spec=S(n_fft=96))
    refused(b"power of two", spec=S(n_fft=4096))
    refused(b"hop", spec=S(hop=0))
    refused(b"hop", spec=S(hop=65536))
    refused(b"n_mels", spec=S(n_mels=257))
    refused(b"n_weights", spec=S(n_weights=8193))
    refused(b"n_weights", spec=S(n_mels=0, n_weights=1))
    refused(b"reserved", spec=S(reserved=(0, 0, 7)))
    refused(b"row_frames", R=1 << 31, pitch=1 << 31)
    refused(b"frame_pitch", pitch=R - 1)
    refused(b"null d_bands", d_bands=None)
    refused(b"PLANAR32", fmt=libflac.OUT_PLANAR32)
    refused(b"bnflac_md5_layout", fmt=libflac.OUT_FLACDECODER)
    refused(b"bnflac_md5_layout", fmt=libflac.OUT_FILEREADER, sp=params(2, 20))
    refused(b"channels", fmt=libflac.OUT_INTERLEAVED32, sp=params(9, 24))
    refused(b"channels", sp=params(0, 24))
    refused(b"flags", flags=2)
    refused(b"16-byte aligned", out_offset=4)
    refused(b"16-byte aligned", tab_offset=8)
    refused(b"16-byte aligned", d_pcm=d_pcm[8:])
    refused(b"8-byte aligned", win_offset=4)
    refused(b"4-byte aligned", bands_offset=2)
    refused(b"too many streams", n=1 << 30)
    assert _raw_mel(gpu, d_pcm, len(pcm), fmt, sp, win, S(n_mels=0, n_weights=0), d_tab, None, 2, 2, 0,
                    torch.zeros(3 * 2 * 33 * 2, dtype=torch.int32, device=DEV)) == (0, [1, 1, 1, 0])  # null bands with n_mels 0 are taken


# ------------------------------------------------------------------ 8. the wrapper and the chain
def test_mel_wrapper_writes_into_a_given_tensor(gpu):
    torch, libflac, dec = gpu
    spec, tab, bands = design(48000, 256, 64, 40)
    fmt, sp, stride, unit = layout("OUT_FLACDECODER", 2, 16)
    R, pitch = 45, 49
    pcm = random_pcm(np.random.default_rng(5), 3200 * stride, unit, 16)
    win = window_table([(3, 2816), (9, 3100), (0, 10)])
    d_out = torch.full((3 * 2 * 40 * pitch,), 7.0, dtype=torch.float32, device=DEV)
    d_tab, d_bands = _tables(torch, tab, bands, spec)
    rows, d_st = dec.gather_ranges_mel(_upload_pcm(torch, pcm), fmt, sp, _dev(torch, win), 3, spec, d_tab, d_bands.view(torch.int32), R,
                                       d_out=d_out, frame_pitch=pitch, pcm_bytes=len(pcm))
    torch.cuda.synchronize()
    assert rows.data_ptr() == d_out.data_ptr() and tuple(rows.shape) == (3, 2, 40, R)
    want, want_st = libflac.gather_ranges_mel_host(pcm, fmt, sp, win, spec, tab, bands, R)
    assert d_st.cpu().numpy().tolist() == want_st.tolist() == [0, 0, 1, 0]
    assert_bits(rows.contiguous().cpu().numpy().view(np.uint32).reshape(-1), np.ascontiguousarray(want).view(np.uint32).reshape(-1))
    assert (d_out.view(3 * 2 * 40, pitch)[:, R:] == 7.0).all()


@pytest.mark.parametrize("mono", [False, True], ids=["planes", "mono"])
def test_mel_chain_against_the_f32_chain(gpu, mono):
    """decode_crops_mel over three synthesised streams (12 frames of 4096 each) against decode_crops_f32
    of the same source windows (mel_request) fed through the host twin: crops at the start (an origin
    of their own), in the middle (two of them overlapping), straddling the end, past it, and of a
    stream that is not there.  With health=True the health records are those of the f32 chain."""
    from birdnest.audio_amd import synth
    torch, libflac, dec = gpu
    syn = [synth.encode(synth.config("C2", nframes=12, seed=31 + i)) for i in range(3)]
    datas = [s.data.tobytes() for s in syn]
    buf, ranges = _pack(datas, (7, 2))
    sp = _stream_params(libflac, datas[0], 0)
    corpus = dec.index_corpus(_upload(torch, buf), len(buf), ranges, sp)
    mel = libflac.mel_design(sp.sample_rate, 512, 100, 24)
    spec, tab, bands = mel
    assert sp.min_blocksize % spec.hop
    T = int(syn[0].nsamples)
    total = 1 + T // spec.hop
    NF = 40
    crops = [(1, 200), (0, 0), (1, 210), (2, 333), (0, total - 15), (2, total + 10), (1, 2), (5, 0)]
    given = libflac.mel_to_device(mel, DEV) if mono else mel  # the tables uploaded once, or host tables
    rows, status = dec.decode_crops_mel(corpus, crops, NF, given, mono=mono, health=True)
    reqs = [(t, ) + libflac.mel_request(spec, t0, NF) for t, t0 in crops]
    nsamples = max(r[2] for r in reqs)
    planes, fstatus = dec.decode_crops_f32(corpus, [r[:3] for r in reqs], nsamples, shared=True, health=True)
    torch.cuda.synchronize()
    assert rows.dtype == torch.float32 and tuple(rows.shape) == (len(crops), 1 if mono else sp.channels, 24, NF)
    got = rows.contiguous().cpu().numpy().view(np.uint32)
    x = planes.cpu().numpy()
    isp = params(sp.channels, sp.bps)
    for k, (t, first, n, origin) in enumerate(reqs):
        want = np.zeros((1 if mono else sp.channels, 24, NF), np.uint32)
        if t < 3:
            lo = min(first, T)
            hi = min(lo + n, T)  # the selection's clipping
            v = np.rint(x[k, :, : hi - lo].astype(np.float64) * 2.0 ** (sp.bps - 1)).astype("<i4")  # exact: x is v 2^-(bps - 1)
            assert np.array_equal(v, np.asarray(syn[t].pcm[lo:hi]).T)
            w, st = libflac.gather_ranges_mel_host(np.ascontiguousarray(v.T).reshape(-1).view(np.uint8), libflac.OUT_INTERLEAVED32, isp,
                                                   window_table([(0, hi - lo)]), spec.with_origin(origin), tab, bands, NF, mono=mono)
            want = np.ascontiguousarray(w[0]).view(np.uint32)
        assert_bits(got[k].reshape(-1), want.reshape(-1), "crop %d" % k)
    assert got[0].any() and got[4][:, :, :15].any() and not got[4][:, :, 16:].any() and not got[5].any()
    assert status["gather"].cpu().numpy().tolist()[:2] == [0, 0] and status["select"].cpu().numpy().tolist()[0] & 1 == 0
    assert np.array_equal(status["windows_health"].cpu().numpy(), fstatus["windows_health"].cpu().numpy())
    assert status["health"].cpu().numpy().tolist() == fstatus["health"].cpu().numpy().tolist()
