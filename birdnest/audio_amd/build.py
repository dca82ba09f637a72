"""Build the in-tree native libraries (hipcc for gfx950, gcc for host-only C).

    libbnflac.so        -- HIP kernels + C ABI (the product)
    libbnflac_synth.so  -- synthetic FLAC workload generator

Outputs go to birdnest/audio_amd/lib/ so they travel with the repo snapshot to the GPU box.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(PKG))
CSRC = os.path.join(PKG, "csrc")
LIB = os.path.join(PKG, "lib")
INCLUDE = os.path.join(ROOT, "include")

# The translation units of libbnflac.so: (source under csrc/, extra -D flags, object name).
# bnflac_kernels.hip is built once per instance, and the define names what the object holds;
# bnflac_sys.hip includes the headers it uses.  This is the only description of the build: the
# compile jobs, the staleness check and source_hash() all derive from it and from the listing
# of csrc/ below.  (The rows keep the link order the library has always had.)
HIP_TUS = [
    ("bnflac_kernels.hip", ["-DBNF_K_PARSE"], "bnflac_parse"),  # sync scan, parse, both indexers, frame orders, the dispatcher
    ("bnflac_kernels.hip", ["-DBNF_DEC_W=8"], "bnflac_decode_w8"),  # k_decode<8>
    ("bnflac_kernels.hip", ["-DBNF_DEC_W=32"], "bnflac_decode_w32"),  # k_decode<32>, k_decode_list, k_decode_seg
    ("bnflac_kernels.hip", ["-DBNF_ST_FD=1"], "bnflac_decode_st_fd"),  # k_decode_st<FLACDECODER>
    ("bnflac_kernels.hip", ["-DBNF_ST_FD=0"], "bnflac_decode_st_any"),  # k_decode_st<other layouts>
    ("bnflac_kernels.hip", ["-DBNF_DEC_W=16"], "bnflac_decode_w16"),  # k_decode<16>
    ("bnflac_kernels.hip", ["-DBNF_K_SW"], "bnflac_decode_sw"),  # k_decode_sw
    ("bnflac_sys.hip", [], "bnflac_sys"),  # k_decode_sys
    ("bnflac_md5.hip", [], "bnflac_md5"),  # k_md5_streams (no CRC tables, no g_stats)
    ("bnflac_scan.hip", [], "bnflac_scan"),  # k_scan_streams (no CRC tables, no g_stats)
    ("bnflac_select.hip", [], "bnflac_select"),  # k_sel_*, k_win_*, k_shr_*, k_gather_ranges (no CRC tables, no g_stats)
    ("bnflac_f32.hip", [], "bnflac_f32"),  # k_gather_f32 (no CRC tables, no g_stats)
    ("bnflac_resample.hip", [], "bnflac_resample"),  # k_gather_f32_rs (no CRC tables, no g_stats)
    ("bnflac_mel.hip", [], "bnflac_mel"),  # k_gather_mel (no CRC tables, no g_stats)
    ("bnflac_health.hip", [], "bnflac_health"),  # k_hl_* (no CRC tables, no g_stats)
    ("bnflac_resync.hip", [], "bnflac_resync"),  # k_rs_* (no CRC tables, no g_stats)
    ("bnflac_runtime.cpp", [], "bnflac_runtime"),
    ("bnflac_reader.cpp", [], "bnflac_reader"),
]


def hip_inputs():
    """Every file libbnflac.so can be built from: all regular files under csrc/, subdirectories
    included (synth/ aside: that is libbnflac_synth.so), and the public headers.  A listing, so
    a new header cannot be forgotten."""
    files = []
    for d, dirs, names in os.walk(CSRC):
        if d == CSRC and "synth" in dirs:
            dirs.remove("synth")
        files += [os.path.join(d, f) for f in names]
    files.sort()
    return files + [os.path.join(INCLUDE, "bnflac.h"), os.path.join(INCLUDE, "FLAC_compat.h")]


SYNTH_SOURCES = [os.path.join(CSRC, "synth", "bnflac_synth.c")]
SYNTH_HEADERS = [os.path.join(CSRC, "synth", "bnflac_synth.h")]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found")


HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden"]


def source_hash() -> str:
    """Hash of everything libbnflac.so is built from: every HIP/C++ source and header, the
    kernel TU split and the hipcc flags.  bench.py stamps its line with it, and a committed PMC
    summary (profiles/traffic_*.json) is attached to a bench run only when the stamps match."""
    import hashlib
    h = hashlib.sha256()
    for f in hip_inputs():
        h.update(os.path.relpath(f, ROOT).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    h.update(repr((HIP_TUS, HIPCC_FLAGS)).encode())
    return h.hexdigest()[:16]


def build_hip(force=False, verbose=False):
    """Compile the kernel TUs and the runtime in parallel (hipcc -c), then link.

    Development variants (never the product): BNFLAC_VARIANT_DIR=<dir> builds into <dir>
    (objects in <dir>/build) with the extra hipcc flags in BNFLAC_EXTRA_CFLAGS, e.g.
    -DBNFLAC_PHASE_TIMERS; load it with BNFLAC_LIB_DIR=<dir> in the debug tools."""
    vdir = os.environ.get("BNFLAC_VARIANT_DIR")
    libdir = vdir or LIB
    out = os.path.join(libdir, "libbnflac.so")
    if force or _stale(out, hip_inputs()):
        os.makedirs(libdir, exist_ok=True)
        objdir = os.path.join(vdir, "build") if vdir else os.path.join(PKG, "build")
        os.makedirs(objdir, exist_ok=True)
        base = [hipcc()] + HIPCC_FLAGS + ["-I" + INCLUDE]
        if vdir:
            base += os.environ.get("BNFLAC_EXTRA_CFLAGS", "").split()
        jobs, objs = [], []
        # development shortcut: BNFLAC_DEV_TUS="bnflac_decode_w8,bnflac_sys" recompiles only
        # those kernel objects (and the host .cpp files) and reuses the others as they are
        # (never set for a real build)
        dev = os.environ.get("BNFLAC_DEV_TUS")
        only = set(dev.split(",")) if dev else None
        for src, defs, name in HIP_TUS:
            o = os.path.join(objdir, name + ".o")
            if only is None or name in only or src.endswith(".cpp") or not os.path.exists(o):
                jobs.append(base + defs + ["-c", os.path.join(CSRC, src), "-o", o])
            objs.append(o)
        procs = []
        for cmd in jobs:
            if verbose:
                print(" ".join(cmd))
            procs.append((cmd, subprocess.Popen(cmd)))
        for cmd, p in procs:
            if p.wait() != 0:
                raise subprocess.CalledProcessError(p.returncode, cmd)
        link = [hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", out + ".tmp"]
        if verbose:
            print(" ".join(link))
        subprocess.check_call(link)
        os.replace(out + ".tmp", out)
    return out


def build_synth(force=False, verbose=False):
    out = os.path.join(LIB, "libbnflac_synth.so")
    if force or _stale(out, SYNTH_SOURCES + SYNTH_HEADERS):
        os.makedirs(LIB, exist_ok=True)
        cmd = ["gcc", "-O2", "-fPIC", "-shared", "-Wall"] + SYNTH_SOURCES + ["-o", out + ".tmp", "-lm"]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
        os.replace(out + ".tmp", out)
    return out


def build_all(force=False, verbose=False):
    return [build_synth(force, verbose), build_hip(force, verbose)]


if __name__ == "__main__":
    for p in build_all(force="--force" in sys.argv, verbose=True):
        print(p)
