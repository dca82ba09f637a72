#!/usr/bin/env python3
"""bnflac_md5_streams against the host route it replaces, on one box in one run.

    python tools/md5_streams_time.py [--streams 64] [--reps 5] [--out profiles/md5_streams.txt]

64 C2 streams (seeds 2 + 1000 i) in one buffer, indexed with one index_streams call.
  device  one decode into FLACDECODER, then md5_streams over the batch with the STREAMINFO sums
          as d_expected: one warm call, then `reps` calls timed with device events.  Every
          verdict must be 0.
  host    the only route without md5_streams: a decode into INTERLEAVED32, the copy of that PCM
          to the host, bnflac_md5_interleaved32 per stream (wall clock; the decode with events).
          Every sum must equal STREAMINFO's.
  static  hipcc -S on bnflac_md5.hip (no GPU): VGPRs per kernel instance and the VALU
          instructions of the fast loop's body, per 64-byte block.
Each step runs as a child process under its own `timeout`; the first failure ends the run.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_LIMIT_S = {"static": 120, "device": 300, "host": 420}
SRC_NAMES = {0: "packed", 1: "int32 B=1", 2: "int32 B=2", 3: "int32 B=3", 4: "int32 B=4"}


def static_counts():
    """-> lines: VGPRs and the fast loop's VALU count per block for every k_md5_streams<SRC>"""
    from birdnest.audio_amd import build
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "bnflac_md5.s")
        subprocess.check_call([build.hipcc()] + build.HIPCC_FLAGS + ["-I" + build.INCLUDE, "--cuda-device-only", "-S",
                                                                      os.path.join(build.CSRC, "bnflac_md5.hip"), "-o", asm],
                              stderr=subprocess.DEVNULL)
        text = open(asm).read()
    lines = []
    for m in re.finditer(r"^_Z13k_md5_streamsILi(\d)E\w*:.*?^; NumVgprs: (\d+).*?^; ScratchSize: (\d+)", text, re.S | re.M):
        src, vgprs, scratch = int(m.group(1)), int(m.group(2)), int(m.group(3))
        # the fast loop: the largest loop header block that loads from global memory
        best = []
        for blk in re.split(r"^\.LBB\d+_\d+:", m.group(0), flags=re.M)[1:]:
            head, ins = blk.split("\n", 1)[0], [x.strip() for x in blk.splitlines()[1:]]
            ins = [x for x in ins if x and not x.startswith((";", "."))]
            if "Loop Header" in head and any(x.startswith("global_load") for x in ins) and len(ins) > len(best):
                best = ins
        valu = sum(x.startswith("v_") for x in best)
        lit = sum(x.startswith("v_") and re.search(r"0x[0-9a-f]{5,8}", x) is not None for x in best)
        blocks = 3 if src == 3 else 1
        lines.append(f"k_md5_streams<{src}> ({SRC_NAMES[src]}): {vgprs} VGPRs, scratch {scratch} B; fast loop body "
                     f"{valu} VALU for {blocks} block(s) = {valu / blocks:.0f} VALU per 64-byte block, "
                     f"{lit} of them with a literal operand")
    return lines


def _encode(i):
    from birdnest.audio_amd import synth
    return synth.encode(synth.config("C2", seed=2 + 1000 * i))


def corpus(nstreams):
    import multiprocessing
    from birdnest.audio_amd import libflac, synth
    with multiprocessing.get_context("fork").Pool(min(16, nstreams)) as workers:  # before the GPU is touched
        streams = workers.map(_encode, range(nstreams))
    lens = [(len(s.data) + 255) // 256 * 256 for s in streams]
    base = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    buf = np.zeros(int(base[-1]) + 64, np.uint8)
    table = []
    for i, s in enumerate(streams):
        b = int(base[i])
        buf[b:b + len(s.data)] = s.data
        table.append((b, b + len(s.data), b + int(s.frame_offsets[0]), s.nsamples))
    sp = libflac.StreamParams.from_synth(synth.config("C2"), 0)
    sums = [libflac.streaminfo_md5(s.data) for s in streams]
    return buf, table, streams, sp, sums


def step(name, args):
    if name == "static":
        print("\n".join(static_counts()), flush=True)
        return 0
    import torch
    from birdnest.audio_amd import libflac
    buf, table, streams, sp, sums = corpus(args.streams)
    n = args.streams
    nbytes = len(buf) - 64
    nframes = sum(len(s.frame_offsets) for s in streams)
    total = sum(t[3] for t in table)
    dev = torch.device("cuda:0")
    dec = libflac.BatchDecoder(0)
    d_bytes = torch.from_numpy(buf).to(dev)
    d_offs, d_os, d_info, d_sf, d_ss, d_st = dec.index_streams(d_bytes, nbytes, table, sp, nframes + 8)
    fmt = libflac.OUT_FLACDECODER if name == "device" else libflac.OUT_INTERLEAVED32
    stride = libflac.out_stride(fmt, sp)
    pcm_bytes = total * stride
    d_out = torch.empty(pcm_bytes + 64, dtype=torch.uint8, device=dev)
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def decode():
        e0, e1 = ev(), ev()
        e0.record()
        dec.decode_parsed(d_bytes, nbytes, nframes, sp, fmt, d_out, d_info)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    decode()  # warm
    t_dec = decode()
    if int(d_sf[-1]) != nframes or int(d_st[0]) != 0:
        print("index_streams did not find every frame")
        return 1
    msg_mb = total * 4 / 1e6  # 16-bit stereo: 4 message bytes per sample frame
    if name == "device":
        d_exp = torch.from_numpy(np.frombuffer(b"".join(sums), dtype=np.uint8).copy()).to(dev)
        times = []
        for rep in range(1 + args.reps):
            e0, e1 = ev(), ev()
            e0.record()
            d_md5, d_v, d_status = dec.md5_streams(d_out, fmt, sp, d_ss, n, d_expected=d_exp, pcm_bytes=pcm_bytes)
            e1.record()
            torch.cuda.synchronize()
            if rep:
                times.append(e0.elapsed_time(e1))
        ok = d_status.cpu().tolist() == [0, n, 0, 0] and not d_v.cpu().numpy().any()
        med = float(np.median(times))
        print(f"{n} C2 streams, {msg_mb:.1f} MB of MD5 message ({msg_mb / n:.2f} MB per stream), decoded into FLACDECODER "
              f"in {t_dec:.2f} ms")
        print(f"device route: md5_streams median {med:.2f} ms (min {min(times):.2f}, max {max(times):.2f}, {len(times)} calls "
              f"after one warm call); {msg_mb / n / med * 1e3:.1f} MB/s per stream, {msg_mb / med:.2f} GB/s over the batch")
        print("every verdict 0 (sums equal STREAMINFO's):", bool(ok), flush=True)
        return 0 if ok else 1
    # the host route
    host = torch.empty(pcm_bytes, dtype=torch.uint8).pin_memory()
    t0 = time.perf_counter()
    host.copy_(d_out[:pcm_bytes])
    torch.cuda.synchronize()
    t_copy = (time.perf_counter() - t0) * 1e3
    pcm = host.numpy().view("<i4").reshape(-1, sp.channels)
    bounds = np.concatenate([[0], np.cumsum([t[3] for t in table])])
    t0 = time.perf_counter()
    got = [libflac.md5_interleaved32(pcm[bounds[i]:bounds[i + 1]], sp.channels, sp.bps) for i in range(n)]
    t_hash = (time.perf_counter() - t0) * 1e3
    ok = got == sums
    t_all = t_dec + t_copy + t_hash
    print(f"host route: decode into INTERLEAVED32 {t_dec:.2f} ms + copy of {pcm_bytes / 1e6:.0f} MB to pinned host memory "
          f"{t_copy:.1f} ms ({pcm_bytes / t_copy / 1e6:.1f} GB/s) + bnflac_md5_interleaved32 per stream {t_hash:.1f} ms "
          f"({msg_mb / n / (t_hash / n) * 1e3:.1f} MB/s per stream, one thread) = {t_all:.1f} ms")
    print("every sum equals STREAMINFO's:", bool(ok), flush=True)
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "md5_streams.txt"))
    ap.add_argument("--step", choices=sorted(STEP_LIMIT_S))
    args = ap.parse_args()
    if args.step:
        return step(args.step, args)
    lines = []
    for name in ("static", "device", "host"):
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S[name]), sys.executable, os.path.abspath(__file__), "--step", name,
               "--streams", str(args.streams), "--reps", str(args.reps)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)  # stderr passes through, not into the file
        print(r.stdout, end="", flush=True)
        lines.append(r.stdout)
        if r.returncode != 0:  # nothing more on the GPU after a failure
            print(f"step {name} failed with exit status {r.returncode}")
            return 1
    with open(args.out, "w") as f:
        f.write("tools/md5_streams_time.py --streams %d --reps %d\n" % (args.streams, args.reps))
        f.write("".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
