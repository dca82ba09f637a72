"""Host side of bnflac_md5_streams: which layouts carry the MD5 message, the exported names and
the STREAMINFO field reader (no GPU)."""
import json
import os
import subprocess

import pytest

from birdnest.audio_amd import libflac
from birdnest.audio_amd._lib import lib_path

GOLD_DIR = os.path.join(os.path.dirname(__file__), "golden")

FD, FR, I32, PL = libflac.OUT_FLACDECODER, libflac.OUT_FILEREADER, libflac.OUT_INTERLEAVED32, libflac.OUT_PLANAR32

LAYOUTS = [(FD, 16, 1, 2), (FD, 16, 2, 2), (FD, 16, 3, 0), (FD, 24, 2, 0)]
LAYOUTS += [(FR, bps, ch, bps // 8) for bps in (16, 24) for ch in (1, 2, 8)]
LAYOUTS += [(FR, bps, 2, 0) for bps in (8, 12, 20)]
LAYOUTS += [(I32, bps, 2, b) for bps, b in ((4, 1), (8, 1), (12, 2), (16, 2), (20, 3), (24, 3), (32, 4), (3, 0), (33, 0))]
LAYOUTS += [(PL, 16, 2, 0), (PL, 24, 1, 0)]


@pytest.mark.parametrize("fmt,bps,channels,want", LAYOUTS)
def test_md5_layout(fmt, bps, channels, want):
    sp = libflac.StreamParams(1, 4096, 4096, 44100, channels, bps, 0)
    assert libflac.md5_layout(fmt, sp) == want


def test_symbols_exported():
    assert {"bnflac_md5_layout", "bnflac_md5_streams"} <= set(libflac.BATCH_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path("libbnflac.so")], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert {"bnflac_md5_layout", "bnflac_md5_streams"} <= exported
    L = libflac.load()
    assert L.bnflac_md5_streams.argtypes is not None and len(L.bnflac_md5_streams.argtypes) == 12


def test_streaminfo_md5_reads_the_field():
    gold = json.load(open(os.path.join(GOLD_DIR, "golden.json")))
    data = open(os.path.join(GOLD_DIR, "rfc9639_ex1.flac"), "rb").read()
    assert libflac.streaminfo_md5(data).hex() == gold["rfc9639_ex1"]["md5"]
    with pytest.raises(ValueError):
        libflac.streaminfo_md5(b"fLaC" + bytes(20))
    with pytest.raises(ValueError):
        libflac.streaminfo_md5(b"OggS" + bytes(60))
