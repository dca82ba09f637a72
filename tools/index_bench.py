#!/usr/bin/env python3
"""bnflac_index_streams against the loop of bnflac_index_stream calls it replaces.

    python tools/index_bench.py [--streams 64] [--reps 20] [--out profiles/index_streams.txt]

64 C2 streams (seeds 2 + 1000 i) in one buffer.  (a) the loop every multi-file caller writes:
one index_stream call per stream, each with its host synchronisation; (b) one index_streams
call.  Both are timed with device events around work that ends in a synchronise, alternating,
each warmed up.  Untimed, the two results are compared.  Each GPU step (check, time) runs as
a child process under its own `timeout`; the first failure ends the run.

    rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- \\
        python tools/index_bench.py --step profile --reps 5

runs the batched call alone in this process (2 + reps calls), for the per-kernel split.
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_LIMIT_S = {"check": 240, "time": 420}
STEPS = sorted(STEP_LIMIT_S) + ["profile"]


def _encode(i):
    from birdnest.audio_amd import synth
    return synth.encode(synth.config("C2", seed=2 + 1000 * i))


def corpus(nstreams, pool=True):
    """-> (host buffer, [(begin, end, first_offset, total_samples)], the streams, shared params)"""
    import multiprocessing
    from birdnest.audio_amd import libflac, synth
    if pool:
        with multiprocessing.get_context("fork").Pool(min(16, nstreams)) as workers:  # before the GPU is touched
            streams = workers.map(_encode, range(nstreams))
    else:
        streams = [_encode(i) for i in range(nstreams)]
    lens = [(len(s.data) + 255) // 256 * 256 for s in streams]
    base = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    buf = np.zeros(int(base[-1]) + 64, np.uint8)
    table = []
    for i, s in enumerate(streams):
        b = int(base[i])
        buf[b:b + len(s.data)] = s.data
        table.append((b, b + len(s.data), b + int(s.frame_offsets[0]), s.nsamples))
    sp = libflac.StreamParams.from_synth(synth.config("C2"), 0)
    return buf, table, streams, sp


def loop(dec, libflac, d_bytes, table, streams, sp1):
    """(a): what bench.py's c5_job does per file, up to the concatenation on the host"""
    offs, osmp, nsmp = [], [], 0
    for (b, e, first, total), s in zip(table, streams):
        sp1.total_samples = total
        o, os_, _, nf = dec.index_stream(d_bytes[b:], e - b, first - b, sp1, len(s.frame_offsets) + 8)
        offs.append(o[:nf].cpu().numpy() + b)
        osmp.append(os_[:nf].cpu().numpy() + nsmp)
        nsmp += total
    return np.concatenate(offs), np.concatenate(osmp)


def step(name, args):
    import torch
    from birdnest.audio_amd import libflac
    buf, table, streams, sp = corpus(args.streams, pool=name != "profile")
    nbytes = len(buf) - 64
    stream_bytes = sum(e - b for b, e, _, _ in table)
    nframes = sum(len(s.frame_offsets) for s in streams)
    dev = torch.device("cuda:0")
    d_bytes = torch.from_numpy(buf).to(dev)
    dec = libflac.BatchDecoder(0)
    sp1 = libflac.StreamParams.from_synth(streams[0].params, 0)
    cap = nframes + 8

    def batched():
        r = dec.index_streams(d_bytes, nbytes, table, sp, cap)
        torch.cuda.synchronize()
        return r

    if name == "check":
        o, os_ = loop(dec, libflac, d_bytes, table, streams, sp1)
        d_offs, d_os, _, d_sf, d_ss, d_st = batched()
        st = d_st.cpu().numpy()
        sf = d_sf.cpu().numpy()
        ok = (st[0] == 0 and int(sf[-1]) == len(o) == nframes and np.array_equal(d_offs[:len(o)].cpu().numpy(), o)
              and np.array_equal(d_os[:len(o)].cpu().numpy(), os_)
              and np.array_equal(np.diff(sf), [len(s.frame_offsets) for s in streams])
              and np.array_equal(d_ss.cpu().numpy(), np.concatenate([[0], np.cumsum([t[3] for t in table])])))
        print(f"{args.streams} C2 streams, {stream_bytes / 1e6:.1f} MB, {nframes} frames, {int(st[1])} sync candidates")
        print("loop and batched call agree:", bool(ok), flush=True)
        return 0 if ok else 1

    if name == "profile":  # the batched call alone, for a kernel trace (no worker processes)
        for _ in range(2 + args.reps):
            batched()
        return 0

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    fa = lambda: loop(dec, libflac, d_bytes, table, streams, sp1)
    for _ in range(2):  # warm-up of both (scratch allocations, code objects)
        fa()
        batched()
    ta, tb = [], []
    for _ in range(args.reps):
        ta.append(timed(fa))
        tb.append(timed(batched))
    for label, t in (("(a) loop of %d index_stream calls" % args.streams, ta), ("(b) one index_streams call", tb)):
        med = float(np.median(t))
        print(f"{label}: median {med:.3f} ms (min {min(t):.3f}, max {max(t):.3f}, {len(t)} reps), "
              f"{stream_bytes / med / 1e6:.1f} GB/s")
    print(f"(a) / (b): {np.median(ta) / np.median(tb):.2f}", flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_streams.txt"))
    ap.add_argument("--step", choices=STEPS)
    args = ap.parse_args()
    if args.step:
        return step(args.step, args)
    lines = []
    for name in ("check", "time"):
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S[name]), sys.executable, os.path.abspath(__file__), "--step", name,
               "--streams", str(args.streams), "--reps", str(args.reps)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        print(r.stdout, end="", flush=True)
        lines.append(r.stdout)
        if r.returncode != 0:  # nothing more on the GPU after a failure
            print(f"step {name} failed with exit status {r.returncode}")
            return 1
    with open(args.out, "w") as f:
        f.write("tools/index_bench.py --streams %d --reps %d\n" % (args.streams, args.reps))
        f.write("".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
