#!/usr/bin/env python3
"""What resynchronisation adds to the batched index: bnflac_index_streams_resync against
bnflac_index_streams on tools/index_bench.py's corpus.

    python tools/index_resync_bench.py [--streams 64] [--reps 20] [--out profiles/index_resync.txt]

64 C2 streams in one buffer.  (a) one index_streams call (the baseline, unchanged code); (b) one
index_streams_resync call over the same intact corpus; (c) the resync call over a copy in which one
stream in eight is damaged (three frames zeroed, and a bit flipped in the body of a later frame).
Each is timed with device events around a call that ends in a synchronise, alternating, after a
warm-up; medians.  Untimed, (b) is compared with (a) table by table and (c) with the damage's
geometry.  Each GPU step (check, time) runs as a child process under its own `timeout`; the first
failure ends the run.
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

STEP_LIMIT_S = {"check": 240, "time": 300}
ZEROED, FLIPPED = (4, 5, 6), 9  # frames of a damaged stream


def damaged(buf, table, streams):
    """One stream in eight: frames 4..6 zeroed, one bit flipped near the end of frame 9."""
    out = buf.copy()
    hit = []
    for i, ((b, e, _, _), s) in enumerate(zip(table, streams)):
        o = [int(x) for x in s.frame_offsets] + [len(s.data)]
        if i % 8 or len(o) < 13:
            continue
        out[b + o[ZEROED[0]]: b + o[ZEROED[-1] + 1]] = 0
        out[b + o[FLIPPED + 1] - 10] ^= 0x10
        hit.append(i)
    return out, hit


def step(name, args):
    import torch
    import index_bench
    from birdnest.audio_amd import libflac
    buf, table, streams, sp = index_bench.corpus(args.streams)
    nbytes = len(buf) - 64
    nframes = sum(len(s.frame_offsets) for s in streams)
    stream_bytes = sum(e - b for b, e, _, _ in table)
    bad, hit = damaged(buf, table, streams)
    dev = torch.device("cuda:0")
    d_ok, d_bad = torch.from_numpy(buf).to(dev), torch.from_numpy(bad).to(dev)
    dec = libflac.BatchDecoder(0)
    cap = nframes + 8

    def plain():
        r = dec.index_streams(d_ok, nbytes, table, sp, cap)
        torch.cuda.synchronize()
        return r

    def resync(d):
        r = dec.index_streams_resync(d, nbytes, table, sp, cap)
        torch.cuda.synchronize()
        return r

    if name == "check":
        a, b, c = plain(), resync(d_ok), resync(d_bad)
        same = all(torch.equal(x, y) for x, y in zip(a, b[:6]))
        sf = c[3].cpu().numpy()
        st = c[5].cpu().numpy()
        rs = libflac.resync_array(c[6].cpu().numpy())
        gaps = (libflac.info_array(c[2].cpu().numpy())["flags"][: int(sf[-1])] & libflac.FRAME_GAP) != 0
        ok = (same and int(sf[-1]) == nframes and int(st[3]) == len(ZEROED) * len(hit) == int(gaps.sum())
              and np.array_equal(np.flatnonzero(rs["gap_frames"]), hit) and (rs["segments"][hit] == 3).all())
        print(f"{args.streams} C2 streams, {stream_bytes / 1e6:.1f} MB, {nframes} frames, {int(st[1])} sync candidates, "
              f"{len(hit)} streams damaged")
        print("resync equals index_streams on the intact corpus, and fills the holes of the damaged one:", bool(ok),
              flush=True)
        return 0 if ok else 1

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    runs = [("(a) index_streams, intact corpus", plain), ("(b) index_streams_resync, intact corpus", lambda: resync(d_ok)),
            ("(c) index_streams_resync, one stream in eight damaged", lambda: resync(d_bad))]
    for _ in range(2):  # warm-up (scratch allocations, code objects)
        for _, fn in runs:
            fn()
    times = [[] for _ in runs]
    for _ in range(args.reps):
        for t, (_, fn) in zip(times, runs):
            t.append(timed(fn))
    for (label, _), t in zip(runs, times):
        print(f"{label}: median {float(np.median(t)):.3f} ms (min {min(t):.3f}, max {max(t):.3f}, {len(t)} reps)")
    print(f"(b) / (a): {np.median(times[1]) / np.median(times[0]):.2f}   (c) / (a): "
          f"{np.median(times[2]) / np.median(times[0]):.2f}", flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_resync.txt"))
    ap.add_argument("--step", choices=sorted(STEP_LIMIT_S))
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
        f.write("tools/index_resync_bench.py --streams %d --reps %d\n" % (args.streams, args.reps))
        f.write("".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
