"""build.py's inputs: the staleness check and source_hash() must cover every file a kernel TU
can include.  Both take their file list from build.hip_inputs(), a listing of csrc/, and the
compile jobs from build.HIP_TUS; nothing else names a source."""
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

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


def _includes(path):
    """The files under csrc/ and include/ that `path` names in #include "..." lines."""
    out = []
    with open(path) as fh:
        for name in re.findall(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', fh.read(), re.M):
            for d in (os.path.dirname(path), build.CSRC, build.INCLUDE):
                f = os.path.normpath(os.path.join(d, name))
                if os.path.isfile(f):
                    out.append(f)
                    break
            else:
                raise AssertionError("%s includes %s, which is in neither csrc/ nor include/" % (path, name))
    return out


def test_every_csrc_file_is_reached_from_a_tu():
    """No orphans: following #include "..." from the HIP_TUS sources reaches every file under csrc/."""
    seen, todo = set(), [os.path.join(build.CSRC, src) for src, _, _ in build.HIP_TUS]
    while todo:
        f = todo.pop()
        if f not in seen:
            seen.add(f)
            todo += _includes(f)
    orphans = sorted(set(_csrc_files(build.CSRC)) - seen)
    assert not orphans, orphans


def test_no_two_tus_are_the_same_build():
    """Rows that share a source differ in their defines, not only in the object's name."""
    jobs = [(src, tuple(sorted(defs))) for src, defs, _ in build.HIP_TUS]
    assert len(set(jobs)) == len(jobs), sorted(j for j in jobs if jobs.count(j) > 1)


def test_every_header_compiles_on_its_own(tmp_path):
    """A header includes what it uses: a file holding nothing but `#include "<header>"` passes
    the device-side syntax check, for every header under csrc/."""
    try:
        cc = build.hipcc()
    except RuntimeError:
        pytest.skip("hipcc not found")
    headers = [f for f in _csrc_files(build.CSRC) if f.endswith(".h")]
    family = {"bnf_common.h", "bnf_bitreader.h", "bnf_frame.h", "bnf_crc16.h", "bnf_crc16_tab.h", "bnf_residual.h"}
    assert family <= {os.path.basename(h) for h in headers}, "the shared device code is in headers of its own"

    def check(h):
        src = tmp_path / (os.path.basename(h) + ".hip")
        src.write_text('#include "%s"\n' % os.path.relpath(h, build.CSRC))
        cmd = [cc] + build.HIPCC_FLAGS + ["-I" + build.INCLUDE, "-I" + build.CSRC, "--cuda-device-only",
                                          "-fsyntax-only", str(src)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        return h, r.returncode, r.stderr

    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        bad = [(os.path.basename(h), err[-1500:]) for h, rc, err in pool.map(check, headers) if rc != 0]
    assert not bad, bad


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
