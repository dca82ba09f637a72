"""Where every decode kernel writes (tests/out_placement.py holds the frames, the plans and the model).

Each test runs bnflac_decode_frames on a view into a larger allocation filled with a fill byte and
compares the whole allocation -- front guard, every gap, the bytes between out_bytes and the end
of the view, back guard -- byte for byte with the contract of include/bnflac.h restated in Python
integers, and the records field by field.  The frames' PCM is frame_pcm() (RFC 9639 in unbounded
integers); nothing is a tolerance.

  a  the three placement plans of every (carrier, layout) leg through d_out_sample: every start
     residue modulo the leg's line, gaps of a sample or more, whole / ragged / single chunks;
     the S24 and T24 FILEREADER legs also under their exact ablation switches
  b  placement by header number: 36-bit sample numbers minus a 36-bit base_sample, frame number
     x blocksize, frame number x STREAMINFO blocksize
  c  the cut at out_bytes: a frame that ends on it, one sample past it, behind it; out_bytes no
     multiple of the stride; a truncated frame zero-filled in range and untouched across the cut
  d  positions that wrap: out_sample = 2^64 - d (through the table and through a header number
     below base_sample) and out_sample = ceil(2^64 / stride).  Before every launch the test proves
     on the CPU that the range the contract assigns and the range a wrapping product would hit
     both lie inside the allocation, so a kernel that wraps fails here by comparison.

Every batch runs under the lane kernels and under k_decode_sys, in plan order and reversed, and
every frame that decodes must carry its carrier's class flag and no hand-back flag: the store path
under test is the one that wrote the bytes.

A truncated frame out of range is not zero-filled.  Its status says which check met it first: the
parse walks every subframe but the last, so a cut before the last subframe is status 2 from the
parse (the range check marks only frames that would decode), and a cut inside the last subframe
(every cut of a one-channel frame) is status 3 with flags bit 1 from the range check, which comes
before the decode that would find the cut.  Test c cuts the first subframe, test d the last."""
import numpy as np
import pytest

from tests import flac_frames as F
from tests import out_placement as P
from tests.conftest import gpu_available

pytestmark = pytest.mark.gpu

FL_OOB, FL_W32, FL_ST, FL_REDO, FL_W16, FL_WAVE_REDO, FL_SW = 2, 16, 32, 64, 128, 512, 1024  # bnflac_device.h
CLASS = {"k_decode_st": FL_ST, "k_decode<16>": FL_W16, "k_decode<32>": FL_W32, "k_decode<8>": 0}
NO_WIDE24, SW_NO_LINE = 0x2000, 0x20000000  # bnflac_launch.h: exact switches
MODES = [0, 1]


@pytest.fixture(scope="module")
def gpu():
    if not gpu_available():
        pytest.skip("no GPU")
    import torch
    from birdnest.audio_amd import libflac
    dec = libflac.BatchDecoder(0)
    yield torch, libflac, dec
    dec.L.bnflac_debug_set_decode_sys(-1)
    dec.L.bnflac_debug_set_ablate(0)


def _run(gpu, b, sys_on, reverse, ablate=0):
    """one decode_frames call over a batch -> (records in call order, the whole allocation, the call's item order)"""
    torch, libflac, dec = gpu
    dev = torch.device("cuda:0")
    assert b.unsafe() == [], "a range of this batch would leave the guarded allocation: not launched"
    data, offs, nbytes = b.buffer()
    n = len(b.items)
    order = list(range(n))[::-1] if reverse else list(range(n))
    sp = (libflac.StreamParams(0, 0, 0, 0, b.channels, b.bps, 0) if b.si is None else
          libflac.StreamParams(1, P.SI_FIXED, P.SI_FIXED, F.SI_RATE, b.channels, b.bps, 0) if b.si == "fixed" else
          libflac.StreamParams(1, F.SI_BLOCKSIZE, F.SI_BLOCKSIZE, F.SI_RATE, b.channels, b.bps, 0))
    fmt = getattr(libflac, b.layout)
    assert libflac.out_stride(fmt, sp) == b.stride
    d_bytes = torch.zeros((len(data) + 15) // 16 * 16 + 32, dtype=torch.uint8, device=dev)
    d_bytes[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
    d_offs = torch.tensor([offs[k] for k in order], dtype=torch.int64, device=dev)
    d_os = None
    if b.table:  # values of 2^63 and more travel as the two's-complement int64 of a uint64
        d_os = torch.from_numpy(np.array([b.items[k].p % P.U64 for k in order], dtype=np.uint64).view(np.int64)).to(dev)
    alloc = torch.full((b.total,), P.FILL, dtype=torch.uint8, device=dev)
    assert alloc.data_ptr() % 256 == 0 and b.front % 256 == 0
    d_out = alloc[b.front:]  # the view runs past out_bytes by the back guard
    d_info = torch.zeros(n * libflac.FRAME_INFO_BYTES, dtype=torch.uint8, device=dev)
    dec.L.bnflac_debug_set_decode_sys(sys_on)
    dec.L.bnflac_debug_set_ablate(ablate)
    try:
        dec.decode_frames(d_bytes, nbytes, d_offs, n, sp, fmt, d_out, d_info, d_out_sample=d_os,
                          base_sample=b.base_sample, out_bytes=b.out_bytes)
        torch.cuda.synchronize()
    except Exception as e:  # a failed launch or a device fault: nothing more can be decoded in this process
        pytest.exit(f"decode of {b.carrier} {b.layout} (sys {sys_on}) failed: {e}", returncode=3)
    finally:
        dec.L.bnflac_debug_set_decode_sys(-1)
        dec.L.bnflac_debug_set_ablate(0)
    return libflac.info_array(d_info.cpu().numpy()), alloc.cpu().numpy(), order, offs


def _check(b, run, sys_on, bad, tag):
    info, got, order, offs = run
    want, verdicts = b.expected()
    kernel = F.CARRIERS[b.carrier][3]
    for i, k in enumerate(order):
        it, v, rec = b.items[k], verdicts[k], info[i]
        fr = it.frame
        name = f"{tag} item {k} (bs {fr.blocksize}, copy {fr.copy}, p {it.p})"
        data = fr.data(it.number, it.variable)
        fields = {"frame_off": offs[k], "blocksize": fr.blocksize, "channels": fr.channels, "bps": fr.bps,
                  "assignment": fr.record_assignment, "number_type": int(it.variable), "number": it.number,
                  "out_sample": it.p % P.U64, "sample_rate": F.SI_RATE}
        fl = int(rec["flags"])
        if it.truncated and int(rec["sub_start"][0]) == 0:
            bad.append(f"{name}: the truncated frame's header did not parse")
        if it.truncated and (v != "out" or P.parse_sees_cut(it)):
            fields.update(status=2)  # found by the parse, or by the decode of a frame in range
        elif v == "out":
            fields.update(status=3)
            if not fl & FL_OOB:
                bad.append(f"{name}: out of range, yet flags {fl:#x} lack bit 1")
        else:
            fields.update(status=0, crc_ok=1, err=-1, resume_bit=8 * (offs[k] + len(data)),
                          crc16_read=int.from_bytes(data[-2:], "big"), crc16_calc=F.crc16(data[:-2]))
            if fl & FL_OOB:
                bad.append(f"{name}: in range, yet flags bit 1 is set")
            # the kernel the carrier is built for wrote it: its class flag, no hand-back
            cls = bool(fl & FL_SW) if kernel == "k_decode_sw" else (
                fl & (FL_ST | FL_W16 | FL_W32) == CLASS[kernel] and not fl & FL_SW)
            if not cls or fl & (FL_REDO | FL_WAVE_REDO):
                bad.append(f"{name}: flags {fl:#x}: not decoded by {'k_decode_sys' if sys_on else kernel} itself")
        bad += [f"{name}: record {f} = {int(rec[f])}, expected {w}" for f, w in fields.items() if int(rec[f]) != w]
    if got.tobytes() != want.tobytes():
        diff = np.nonzero(got != want)[0]
        first = int(diff[0])
        where = ("the front guard" if first < b.front else "the back guard" if first >= b.front + b.out_bytes else
                 f"byte {first - b.front} of the output")
        owner = [k for k, it in enumerate(b.items)
                 if it.p >= 0 and it.p * b.stride <= first - b.front < (it.p + it.frame.blocksize) * b.stride]
        bad.append(f"{tag}: {len(diff)} bytes differ, the first in {where} (items {owner[:3]}): "
                   f"{got[first:first + 8].tolist()} != {want[first:first + 8].tolist()}")


def _run_and_check(gpu, b, tag, ablates=(0,)):
    bad, outs = [], {}
    for sys_on in MODES:
        for reverse in (False, True):
            for ablate in ablates:
                run = _run(gpu, b, sys_on, reverse, ablate)
                _check(b, run, sys_on, bad, f"{tag} [{'sys' if sys_on else 'lanes'}{', reversed' if reverse else ''}"
                                            f"{', ablate %#x' % ablate if ablate else ''}]")
                outs[(sys_on, reverse, ablate)] = run[1]
    first = next(iter(outs.values()))
    assert not bad, f"{len(bad)} findings\n" + "\n".join(bad[:30])
    assert all(o.tobytes() == first.tobytes() for o in outs.values())  # modes, orders and exact switches agree


def _ablates(carrier, layout, kind):
    if layout == "OUT_FILEREADER" and kind in ("line", "mixed"):
        if carrier == "S24":
            return (0, SW_NO_LINE)
        if carrier == "T24":
            return (0, NO_WIDE24)
    return (0,)


@pytest.mark.parametrize("kind", P.PLANS)
@pytest.mark.parametrize("carrier,layout", P.LEGS)
def test_guarded_sparse_placement(gpu, carrier, layout, kind):
    """a: a plan through d_out_sample"""
    _run_and_check(gpu, P.batch_table(carrier, layout, kind), f"{carrier} {layout} {kind}", _ablates(carrier, layout, kind))


@pytest.mark.parametrize("carrier,layout", P.LEGS)
def test_placement_by_sample_number(gpu, carrier, layout):
    """b: d_out_sample NULL, variable-blocksize headers: number - base_sample in 64 bits"""
    _run_and_check(gpu, P.batch_header_variable(carrier, layout), f"{carrier} {layout} header")


@pytest.mark.parametrize("si", [None, "fixed"], ids=["no_streaminfo", "streaminfo"])
@pytest.mark.parametrize("carrier,layout", P.FIXED_LEGS)
def test_placement_by_frame_number(gpu, carrier, layout, si):
    """b: fixed-blocksize headers: number * blocksize, or number * STREAMINFO's blocksize, minus base_sample"""
    _run_and_check(gpu, P.batch_header_fixed(carrier, layout, si), f"{carrier} {layout} fixed {si}")


@pytest.mark.parametrize("carrier,layout", P.LEGS)
def test_cut_at_out_bytes(gpu, carrier, layout):
    """c: frames on, across and behind the cut; the view goes on behind it"""
    _run_and_check(gpu, P.batch_cut(carrier, layout), f"{carrier} {layout} cut")


@pytest.mark.parametrize("carrier,layout", P.WRAP_LEGS)
def test_positions_that_wrap_table(gpu, carrier, layout):
    """d: case A and case B through d_out_sample, and a truncated frame at the case B position"""
    _run_and_check(gpu, P.batch_wrap_table(carrier, layout), f"{carrier} {layout} wrap")


@pytest.mark.parametrize("carrier,layout", P.WRAP_LEGS)
def test_positions_that_wrap_header(gpu, carrier, layout):
    """d: case A through a header number below base_sample, by 1 and by the blocksize"""
    _run_and_check(gpu, P.batch_wrap_header(carrier, layout), f"{carrier} {layout} wrap header")
