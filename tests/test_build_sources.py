"""build.py's inputs: the staleness check and source_hash() must cover every file a kernel TU
can include.  Both take their file list from build.hip_inputs(), a listing of csrc/, and the
compile jobs from build.HIP_TUS; nothing else names a source."""
import os
import shutil

import pytest

from birdnest.audio_amd import build


def _csrc_files(csrc):
    """Every regular file under csrc/ outside synth/ (libbnflac_synth.so's own sources)."""
    out = []
    for d, dirs, files in os.walk(csrc):
        dirs[:] = [x for x in dirs if not (d == csrc and x == "synth")]
        out += [os.path.join(d, f) for f in files]
    return sorted(out)


def test_every_csrc_file_is_a_build_input():
    files = _csrc_files(build.CSRC)
    assert os.path.join(build.CSRC, "bnflac_launch.h") in files and os.path.join(build.CSRC, "bnflac_md5.h") in files
    inputs = set(build.hip_inputs())
    assert set(files) <= inputs, sorted(set(files) - inputs)
    assert all(os.path.isfile(f) for f in inputs)


def test_staleness_check_sees_every_input(tmp_path):
    """A library older than any one input is stale; newer than all of them, it is not."""
    lib = tmp_path / "libbnflac.so"
    lib.write_bytes(b"")
    inputs = build.hip_inputs()
    newest = max(os.path.getmtime(f) for f in inputs)
    os.utime(lib, (newest + 10, newest + 10))
    assert not build._stale(str(lib), inputs)
    for f in inputs:
        t = os.path.getmtime(f)
        os.utime(lib, (t - 10, t - 10))
        assert build._stale(str(lib), inputs), f


def test_tu_descriptions_name_existing_files():
    objs = [name for _, _, name in build.HIP_TUS]
    assert len(set(objs)) == len(objs), "two TUs would share an object file"
    for src, defs, _ in build.HIP_TUS:
        assert os.path.isfile(os.path.join(build.CSRC, src)), src
        assert all(d.startswith("-D") for d in defs), defs


@pytest.fixture
def tree_copy(tmp_path, monkeypatch):
    """build.py looking at a copy of csrc/ and include/."""
    csrc, inc = tmp_path / "csrc", tmp_path / "include"
    shutil.copytree(build.CSRC, csrc)
    shutil.copytree(build.INCLUDE, inc)
    monkeypatch.setattr(build, "CSRC", str(csrc))
    monkeypatch.setattr(build, "INCLUDE", str(inc))
    return str(csrc)


def test_one_more_byte_in_any_file_changes_the_hash(tree_copy):
    h0 = build.source_hash()
    assert build.source_hash() == h0
    for f in _csrc_files(tree_copy):
        with open(f, "rb") as fh:
            orig = fh.read()
        with open(f, "ab") as fh:
            fh.write(b"\n")
        assert build.source_hash() != h0, os.path.basename(f)
        with open(f, "wb") as fh:
            fh.write(orig)
    assert build.source_hash() == h0
