#!/usr/bin/env python3
"""What decode_crops(health=True) costs over health=False (bnflac_window_health).

    python tools/health_bench.py [--streams 64] [--crops 16] [--many 256] [--reps 20]
                                 [--out profiles/window_health.txt]

The corpus, the crops and the timing method are tools/crops_bench.py's: 64 C2 streams in one
buffer that stays on the device, indexed once outside the timed region; batches of 16 crops of a
second on streams of their own and of 256 crops in random order, requests on the device, rows as
BNFLAC_OUT_INTERLEAVED32.  One process; each figure is the time between two device events around
CALLS calls in a row, the second event followed by a synchronise, divided by CALLS; health=False
and health=True alternate, after a warm-up of each.  Before anything is timed: the rows of the two
are bit-equal, and the health records say that nothing is damaged or missing (the corpus is
intact).  Nothing is gated on a time.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CALLS = 5
WARMUP = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--crops", type=int, default=16)
    ap.add_argument("--many", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_health.txt"))
    args = ap.parse_args()
    from index_bench import corpus as make_corpus
    buf, table, streams, _ = make_corpus(args.streams)  # encodes in worker processes, before the GPU is touched
    import torch
    from birdnest.audio_amd import libflac
    if not torch.cuda.is_available():
        print("no GPU: nothing is measured")
        return 1
    n, K, M = args.streams, args.crops, args.many
    nbytes = len(buf) - 64
    sp = libflac.StreamParams.from_buffer_copy(libflac.scan_stream_host(streams[0].data)[0].sp)
    sp.total_samples = 0
    T = int(sp.sample_rate)
    fmt = libflac.OUT_INTERLEAVED32
    rng = np.random.default_rng(7)
    chosen = [int(s) for s in rng.permutation(n)[:K]]
    crops = [(s, int(rng.integers(0, streams[s].nsamples - T)), T) for s in chosen]
    many = [(int(s), int(rng.integers(0, streams[int(s)].nsamples - T)), T) for s in rng.integers(0, n, M)]

    dev = torch.device("cuda:0")
    dec = libflac.BatchDecoder(0)
    d_bytes = torch.from_numpy(buf).to(dev)
    d_files = torch.tensor([[b, e, 0, 0] for b, e, _, _ in table], dtype=torch.int64, device=dev).reshape(-1)
    cap = sum(len(s.frame_offsets) for s in streams) + 8
    corp = dec.index_corpus(d_bytes, nbytes, d_files, sp, cap=cap)
    lines = [f"tools/health_bench.py --streams {n} --crops {K} --many {M} --reps {args.reps}",
             f"{n} C2 streams, {cap - 8} frames, {nbytes} bytes resident; a crop is {T} sample frames "
             f"({T * libflac.out_stride(fmt, sp)} bytes)"]
    paths, ok = [], True
    for reqs in (crops, many):
        d_req = torch.tensor(reqs, dtype=torch.int64, device=dev).reshape(-1)
        k = len(reqs)
        sel_cap = k * ((T - 1) // sp.min_blocksize + 2)
        off = lambda d_req=d_req: dec.decode_crops(corp, d_req, T, fmt)
        on = lambda d_req=d_req: dec.decode_crops(corp, d_req, T, fmt, health=True)
        rows0, _ = off()
        rows1, st = on()
        torch.cuda.synchronize()
        words = st["health"].cpu().numpy().tolist()
        same = bool(torch.equal(rows0, rows1))
        clean = not st["windows_health"].cpu().numpy().any()
        ok = ok and same and clean and words == [0, 0, 0, 0]
        lines.append(f"{k} crops, {sel_cap} records ({sel_cap * 128} bytes read by the health call): health status {words}, "
                     f"every record zero: {clean}; rows equal between health=False and health=True: {same}")
        paths += [(f"{k} crops, health=False", off), (f"{k} crops, health=True ", on)]
    print("\n".join(lines), flush=True)
    if not ok:
        print("the paths disagree: nothing is timed")
        return 1

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / CALLS

    for _ in range(WARMUP):
        for _, fn in paths:
            timed(fn)
    t = [[] for _ in paths]
    for _ in range(args.reps):
        for i, (_, fn) in enumerate(paths):
            t[i].append(timed(fn))
    out = [f"{label}: median {np.median(x):.3f} ms per call (min {min(x):.3f}, max {max(x):.3f}, {len(x)} reps of {CALLS} calls)"
           for (label, _), x in zip(paths, t)]
    for i in (0, 2):
        out.append(f"{paths[i][0].split(',')[0]}: health=True - health=False = "
                   f"{1000 * (np.median(t[i + 1]) - np.median(t[i])):.1f} us per call (difference of the medians)")
    print("\n".join(out), flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines + out) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
