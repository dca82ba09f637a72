#!/usr/bin/env python3
"""Crops of a resident corpus: decode_crops over an index made once (bnflac_select_windows)
against decode_windows, which scans and indexes the buffer again for every batch.

    python tools/crops_bench.py [--streams 64] [--crops 16] [--many 256] [--reps 20]
                                [--out profiles/select_windows.txt]

64 C2 streams (seeds 2 + 1000 i) in one buffer that stays on the device.  A batch is 16 crops of a
second (sample_rate sample frames), each on a stream of its own so that both paths can express
it, rows as BNFLAC_OUT_INTERLEAVED32.
(a) what the library offered before: decode_windows over the whole buffer, with a zero-length
    window for each of the other 48 streams; the 16 rows are picked out of its 64 afterwards
    (untimed).
(b) index_corpus once, outside the timed region, then decode_crops per batch.
(b256) the same with 256 crops, four per stream on average, in random order: (a) cannot express it.
All tables (files, windows, requests) are on the device before the timed region.  One process;
each figure is the time between two device events around CALLS calls in a row, the second event
followed by a synchronise, divided by CALLS; the three paths alternate, after a warm-up of each.
Before anything is timed: the rows of (a) and (b) are bit-equal to each other and to the
generator's PCM, (b256)'s rows are the generator's PCM, and word 1 of each select status equals
the frame count of bnflac_select_windows_host over the index copied to the host.  Nothing is gated
on a time.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_windows.txt"))
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
    windows = np.zeros((n, 2), np.int64)
    for s, first, _ in crops:
        windows[s] = (first, T)

    dev = torch.device("cuda:0")
    dec = libflac.BatchDecoder(0)
    d_bytes = torch.from_numpy(buf).to(dev)
    d_files = torch.tensor([[b, e, 0, 0] for b, e, _, _ in table], dtype=torch.int64, device=dev).reshape(-1)
    d_windows = torch.from_numpy(windows.reshape(-1)).to(dev)
    d_crops = torch.tensor(crops, dtype=torch.int64, device=dev).reshape(-1)
    d_many = torch.tensor(many, dtype=torch.int64, device=dev).reshape(-1)
    cap = sum(len(s.frame_offsets) for s in streams) + 8

    def path_a():  # scan, index, select_ranges, decode, gather: the table is completed in place, so a copy per call
        return dec.decode_windows(d_bytes, nbytes, d_files.clone(), d_windows, T, sp, fmt, cap=cap)

    corp = dec.index_corpus(d_bytes, nbytes, d_files.clone(), sp, cap=cap)
    path_b = lambda: dec.decode_crops(corp, d_crops, T, fmt)
    path_m = lambda: dec.decode_crops(corp, d_many, T, fmt)

    # ---- untimed: the results
    rows_a, st_a = path_a()
    rows_b, st_b = path_b()
    rows_m, st_m = path_m()
    torch.cuda.synchronize()
    info = libflac.info_array(corp.d_info.cpu().numpy())
    sf = corp.d_stream_frames.cpu().numpy().view(np.uint32)
    ss = corp.d_stream_samples.cpu().numpy().view(np.uint64)
    nframes = int(sf[-1])
    lines = [f"tools/crops_bench.py --streams {n} --crops {K} --many {M} --reps {args.reps}",
             f"{n} C2 streams, {nframes} frames, {nbytes} bytes resident; a crop is {T} sample frames "
             f"({T * libflac.out_stride(fmt, sp)} bytes)"]
    ok = corp.index_status.cpu().numpy()[0] == 0 and int(sf[-1]) == sum(len(s.frame_offsets) for s in streams)
    for label, reqs, rows, st in (("(b)", crops, rows_b, st_b), ("(b256)", many, rows_m, st_m)):
        sel_cap = len(reqs) * ((T - 1) // sp.min_blocksize + 2)
        host = libflac.select_windows_host(info, cap, sf, ss, reqs, sel_cap)[4]
        word = st["select"].cpu().numpy().view(np.uint32).tolist()
        want = np.stack([streams[s].pcm[f: f + T] for s, f, _ in reqs])
        same = np.array_equal(rows.cpu().numpy(), want)
        ok = ok and same and word == host.tolist() and word[0] == 0 and st["gather"].cpu().numpy().tolist() == [0, 0, 0, 0]
        lines.append(f"{label} {len(reqs)} crops: select status {word} (host twin {host.tolist()}) of {sel_cap} records; "
                     f"rows equal the generator's PCM: {same}")
    same_ab = bool(torch.equal(rows_a[chosen], rows_b))
    word_a = st_a["select"].cpu().numpy().view(np.uint32).tolist()
    ok = ok and same_ab and word_a[0] == 0 and word_a[1] == st_b["select"].cpu().numpy()[1]
    lines.append(f"(a) {n} windows, {n - K} of them empty: select status {word_a}; its {K} rows equal (b)'s: {same_ab}")
    print("\n".join(lines), flush=True)
    if not ok:
        print("the paths disagree: nothing is timed")
        return 1

    # ---- timed
    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / CALLS

    paths = ((f"(a) decode_windows: scan, index, select_ranges over {n} streams, decode, gather {n} rows", path_a),
             (f"(b) decode_crops: select_windows of {K} crops over the resident index, decode, gather", path_b),
             (f"(b256) decode_crops: {M} crops with repeats over the {n} streams", path_m))
    for _ in range(WARMUP):
        for _, fn in paths:
            timed(fn)
    t = [[] for _ in paths]
    for _ in range(args.reps):
        for k, (_, fn) in enumerate(paths):
            t[k].append(timed(fn))
    out = []
    for (label, _), x in zip(paths, t):
        out.append(f"{label}: median {np.median(x):.3f} ms per call (min {min(x):.3f}, max {max(x):.3f}, "
                   f"{len(x)} reps of {CALLS} calls)")
    out.append(f"(a) / (b): {np.median(t[0]) / np.median(t[1]):.2f}; (b256) per crop: {1000 * np.median(t[2]) / M:.2f} us, "
               f"(b) per crop: {1000 * np.median(t[1]) / K:.2f} us")
    print("\n".join(out), flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines + out) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
