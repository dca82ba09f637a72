"""Every decode path on the hand-built frames of tests/flac_frames.py: Rice parameters 0..30,
escapes of every width, partition orders up to 15, LPC precisions and shifts at their ends
(negative shifts on each libFLAC path), wasted bits down to a 1-bit subframe, full-scale stereo,
every header code, and the fields a decoder must refuse -- none of which the project's own encoder
writes.

The rows of one (channels, bps) go through one decode_frames call, in table order and reversed
(other lanes, other neighbours), under the lane kernels and under k_decode_sys, parsed by k_parse
and by k_parse_wave.  PCM: bit-exact against restore() (exact integers, in-spec rows) or the CPU
oracle (libFLAC-defined rows).  Records: field by field against the oracle's decode of the frame.
Refused frames: status, error and the reader's position against the oracle, their output range
zero-filled or untouched.  And, so that a hand-back cannot hide a broken fast path, the flags must
say that the kernel a row was built for decoded it (or handed it back, where its rules say so).
Nothing is a tolerance."""
import numpy as np
import pytest

from tests import flac_frames as F
from tests.conftest import gpu_available
from tests.test_frame_fields_host import oracle_frame

pytestmark = pytest.mark.gpu

FL_W32, FL_ST, FL_REDO, FL_W16, FL_WAVE_REDO, FL_SW = 16, 32, 64, 128, 512, 1024  # bnflac_device.h
FILL = 0xAB
LAYOUTS = ["OUT_INTERLEAVED32", "OUT_FLACDECODER", "OUT_FILEREADER", "OUT_PLANAR32"]
COMPARED = ["status", "err", "frame_off", "resume_bit", "cached", "blocksize", "sample_rate", "channels", "assignment",
            "bps", "number_type", "unparseable", "number", "out_sample", "crc8", "crc16_calc", "crc16_read", "crc_ok",
            "sub_start"]  # every field but the flags, which record the path


def _groups_of(layout):
    """the (channels, bps, STREAMINFO) groups a layout is decoded in"""
    keys = list(F.groups())
    if layout == "OUT_FLACDECODER":
        return [k for k in keys if k[:2] == (2, 16)]
    if layout == "OUT_FILEREADER":
        return [k for k in keys if k[:2] == (2, 24)]
    if layout == "OUT_PLANAR32":
        return [k for k in keys if k[:2] == (3, 24)]
    return keys


def _pack(layout, pcm, bps):
    """the bytes of one frame's [channel][sample] PCM in a layout"""
    a = np.array(pcm, dtype=np.int64)
    if layout == "OUT_PLANAR32":
        return a.astype("<i4").tobytes()
    v = np.ascontiguousarray(a.T).reshape(-1)
    if layout == "OUT_INTERLEAVED32":
        return v.astype("<i4").tobytes()
    if layout == "OUT_FLACDECODER" or bps != 24:
        return (v & 0xFFFF).astype("<u2").tobytes()
    return np.stack([v & 0xFF, (v >> 8) & 0xFF, (v >> 16) & 0xFF], axis=1).astype(np.uint8).tobytes()


class _Group:
    """one group's buffer, offsets, output slots and expectations, built once"""

    def __init__(self, key, rows, oracle_of):
        self.key, self.rows = key, rows
        self.data = b"".join(r.data for r in rows)
        self.offs = np.cumsum([0] + [len(r.data) for r in rows[:-1]]).astype(np.int64)
        self.slots = np.cumsum([0] + [r.blocksize for r in rows[:-1]]).astype(np.int64)
        self.total = int(sum(r.blocksize for r in rows))
        self.oracle = [oracle_of[r.name] for r in rows]
        self.pcm = [r.pcm if r.expect == "restore" else o[2] for r, o in zip(rows, self.oracle)]
        self.crc = [F.crc16(r.data[:-2]) for r in rows]  # the writer's own, bit by bit
        self._expected = {}

    def expected(self, layout, stride):
        if layout not in self._expected:
            buf = np.full(self.total * stride, FILL, dtype=np.uint8)
            for r, s, p in zip(self.rows, self.slots, self.pcm):
                if p is not None:
                    b = np.frombuffer(_pack(layout, p, r.bps), dtype=np.uint8)
                    assert len(b) == r.blocksize * stride
                    buf[s * stride:s * stride + len(b)] = b
            self._expected[layout] = buf
        return self._expected[layout]


@pytest.fixture(scope="module")
def table():
    oracle_of = {r.name: oracle_frame(r) for r in F.rows()}
    return {k: _Group(k, rows, oracle_of) for k, rows in F.groups().items()}


@pytest.fixture(scope="module")
def gpu():
    if not gpu_available():
        pytest.skip("no GPU")
    import torch
    from birdnest.audio_amd import libflac
    dec = libflac.BatchDecoder(0)
    yield torch, libflac, dec
    dec.L.bnflac_debug_set_decode_sys(-1)
    dec.L.bnflac_debug_set_parse_wave(-1)


_RUNS = {}


def _decode(gpu, g, layout, sys_on, wave, reverse):
    """one decode_frames call over a group -> (records in call order, output bytes, stride)"""
    key = (g.key, layout, sys_on, wave, reverse)
    if key in _RUNS:
        return _RUNS[key]
    torch, libflac, dec = gpu
    dev = torch.device("cuda:0")
    channels, bps, si = g.key
    sp = (libflac.StreamParams(1, F.SI_BLOCKSIZE, F.SI_BLOCKSIZE, F.SI_RATE, channels, bps, 0) if si
          else libflac.StreamParams(0, 0, 0, 0, channels, bps, 0))
    fmt = getattr(libflac, layout)
    stride = libflac.out_stride(fmt, sp)
    n = len(g.data)
    d_bytes = torch.zeros((n + 15) // 16 * 16 + 32, dtype=torch.uint8, device=dev)
    d_bytes[:n] = torch.frombuffer(bytearray(g.data), dtype=torch.uint8).to(dev)
    order = slice(None, None, -1) if reverse else slice(None)
    d_offs = torch.from_numpy(g.offs[order].copy()).to(dev)
    d_os = torch.from_numpy(g.slots[order].copy()).to(dev)
    d_out = torch.full((g.total * stride,), FILL, dtype=torch.uint8, device=dev)
    d_info = torch.zeros(len(g.rows) * libflac.FRAME_INFO_BYTES, dtype=torch.uint8, device=dev)
    dec.L.bnflac_debug_set_decode_sys(sys_on)
    dec.L.bnflac_debug_set_parse_wave(wave)
    try:
        dec.decode_frames(d_bytes, n, d_offs, len(g.rows), sp, fmt, d_out, d_info, d_out_sample=d_os)
        torch.cuda.synchronize()
    except Exception as e:  # a failed launch or a device fault: nothing more can be decoded in this process
        pytest.exit(f"decode of group {g.key} ({layout}, sys {sys_on}, wave {wave}) failed: {e}", returncode=3)
    finally:
        dec.L.bnflac_debug_set_decode_sys(-1)
        dec.L.bnflac_debug_set_parse_wave(-1)
    info = libflac.info_array(d_info.cpu().numpy())
    _RUNS[key] = (info, d_out.cpu().numpy(), stride)
    return _RUNS[key]


def _rows_of(g, reverse):
    """(record index, row index) pairs of a call"""
    n = len(g.rows)
    return [(i, n - 1 - i if reverse else i) for i in range(n)]


def _check_records(g, info, reverse, bad):
    """each record against the oracle's decode of its frame, field by field"""
    for i, j in _rows_of(g, reverse):
        r, (rc, res, _) = g.rows[j], g.oracle[j]
        rec = info[i]
        off = int(g.offs[j])
        got = {k: int(rec[k]) for k in ("frame_off", "status", "err", "crc_ok", "blocksize", "sample_rate", "channels",
                                        "assignment", "bps", "number_type", "number", "out_sample", "resume_bit",
                                        "crc16_read", "crc16_calc")}
        if rc == 0:
            want = {k: int(getattr(res, k)) for k in ("blocksize", "sample_rate", "channels", "assignment", "bps",
                                                      "number_type", "number")}
            assert int(res.end_off) == len(r.data), r.name  # (the host module's finding, if ever)
            want.update(frame_off=off, status=0, crc_ok=1, out_sample=int(g.slots[j]), resume_bit=8 * (off + len(r.data)),
                        crc16_read=int.from_bytes(r.data[-2:], "big"), crc16_calc=g.crc[j])
        else:
            want = {"frame_off": off, "status": 1, "err": int(res.error)}
            got["end_byte"], want["end_byte"] = (got["resume_bit"] + 7) // 8, off + int(res.end_off)
        bad += [f"{r.name}: record {k} = {got[k]}, the oracle says {v}" for k, v in want.items() if got[k] != v]


def _check_paths(g, info, reverse, sys_on, bad):
    """the kernel a row was built for decoded it, or handed it back where its rules say so"""
    cls = {"k_decode_st": FL_ST, "k_decode<16>": FL_W16, "k_decode<32>": FL_W32, "k_decode<8>": 0}
    for i, j in _rows_of(g, reverse):
        r = g.rows[j]
        if not r.marks or int(info["status"][i]) != 0:
            continue
        fl = int(info["flags"][i])
        if r.kernel == "k_decode_sw":
            ok = bool(fl & FL_SW)
        else:
            ok = fl & (FL_ST | FL_W16 | FL_W32) == cls[r.kernel] and not fl & FL_SW
        if sys_on:
            ok = ok and bool(fl & FL_WAVE_REDO) == (not r.sys_kept) and not fl & FL_REDO
        else:
            ok = ok and not fl & FL_WAVE_REDO and bool(fl & FL_REDO) == (not r.lane_kept)
        if not ok:
            bad.append(f"{r.name}: flags {fl:#x}, built for {r.kernel}, "
                       f"{'k_decode_sys' if sys_on else 'the lane kernel'} should "
                       f"{'keep it' if (r.sys_kept if sys_on else r.lane_kept) else 'hand it back'}")


def _check_output(g, info, out, stride, layout, reverse, bad):
    """decoded frames bit-exact; a refused frame's range zero-filled (its header parsed) or untouched"""
    want = g.expected(layout, stride).copy()
    for i, j in _rows_of(g, reverse):
        r = g.rows[j]
        a, b = int(g.slots[j]) * stride, (int(g.slots[j]) + r.blocksize) * stride
        if g.pcm[j] is None:
            got = out[a:b]
            if int(info["sub_start"][i][0]) != 0:
                if got.any():
                    bad.append(f"{r.name}: refused after its header parsed, yet not zero-filled")
            elif not (got == FILL).all():
                bad.append(f"{r.name}: the header was refused, yet the output was written")
            want[a:b] = got
        elif not np.array_equal(out[a:b], want[a:b]):
            k = int(np.nonzero(out[a:b] != want[a:b])[0][0])
            bad.append(f"{r.name} ({r.kernel}): PCM differs from byte {k} of its {b - a}: "
                       f"{out[a + k:a + k + 8].tolist()} != {want[a + k:a + k + 8].tolist()}")
            want[a:b] = out[a:b]
    if out.tobytes() != want.tobytes():
        bad.append("bytes outside the frames' ranges were written")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("wave", [0, 1], ids=["k_parse", "k_parse_wave"])
@pytest.mark.parametrize("sys_on", [0, 1], ids=["lanes", "k_decode_sys"])
def test_frame_fields(gpu, table, sys_on, wave, layout):
    for key in _groups_of(layout):
        g = table[key]
        for reverse in (False, True):
            info, out, stride = _decode(gpu, g, layout, sys_on, wave, reverse)
            bad = []
            _check_records(g, info, reverse, bad)
            _check_output(g, info, out, stride, layout, reverse, bad)
            _check_paths(g, info, reverse, sys_on, bad)
            assert not bad, f"group {key}, {'reversed' if reverse else 'table'} order: {len(bad)} findings\n" + "\n".join(bad[:40])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_modes_agree(gpu, table, layout):
    """records (all but the path flags) and output bytes are the same under the four combinations
    of decode and parse mode, in both orders"""
    for key in _groups_of(layout):
        g = table[key]
        for reverse in (False, True):
            ref_info, ref_out, _ = _decode(gpu, g, layout, 0, 0, reverse)
            for sys_on, wave in ((0, 1), (1, 0), (1, 1)):
                info, out, _ = _decode(gpu, g, layout, sys_on, wave, reverse)
                for name in COMPARED:
                    bad = np.nonzero((info[name] != ref_info[name]).reshape(len(info), -1).any(axis=1))[0]
                    assert len(bad) == 0, (name, sys_on, wave, [g.rows[::-1 if reverse else 1][b].name for b in bad[:4]])
                assert out.tobytes() == ref_out.tobytes(), (key, sys_on, wave, reverse)
        fwd, rev = _decode(gpu, g, layout, 0, 0, False), _decode(gpu, g, layout, 0, 0, True)
        assert fwd[1].tobytes() == rev[1].tobytes(), key  # the same slots in either order
