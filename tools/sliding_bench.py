#!/usr/bin/env python3
"""Sliding windows over a resident corpus: decode_crops with shared=False (bnflac_select_windows:
a frame two windows need is copied and decoded twice) against shared=True
(bnflac_select_windows_shared: the union of the frames, each once).

    python tools/sliding_bench.py [--streams 64] [--window 3.0] [--hops 3.0,1.0,0.5] [--reps 20]
                                  [--out profiles/select_windows_shared.txt]

64 C2 streams (seeds 2 + 1000 i) in one buffer that stays on the device, scanned and indexed once,
untimed (index_corpus with cap = the frame count + 8, as tools/crops_bench.py).  For each hop, the
requests are windows of `window` seconds every `hop` seconds over every whole stream (the last ones
clipped by the stream's end), on the device before the timed region; rows as BNFLAC_OUT_INTERLEAVED32.
shared=True is sized by what a caller of sliding windows knows without looking at them: the corpus's
own frame and sample counts (max_frames, max_samples); shared=False has its fixed bounds.
One process; each figure is the time between two device events around CALLS calls in a row, the
second event followed by a synchronise, divided by CALLS; the two paths alternate, after a warm-up of
each.  Before anything is timed, per hop: the rows of the two paths are bit-equal to each other and
to the generator's PCM (compared on the device, stream by stream), and the frame counts equal those
of the host twins over the index copied to the host.  Nothing is gated on a time.
With --default-cap the shortest hop is also run over a second index made with index_corpus's default
cap (a bound from the buffer's size): what the shared path's passes over [0, cap) cost there.
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
    ap.add_argument("--window", type=float, default=3.0)
    ap.add_argument("--hops", default="3.0,1.0,0.5")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--default-cap", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_windows_shared.txt"))
    args = ap.parse_args()
    from index_bench import corpus as make_corpus
    buf, table, streams, _ = make_corpus(args.streams)  # encodes in worker processes, before the GPU is touched
    import torch
    from birdnest.audio_amd import libflac
    if not torch.cuda.is_available():
        print("no GPU: nothing is measured")
        return 1
    n = args.streams
    nbytes = len(buf) - 64
    sp = libflac.StreamParams.from_buffer_copy(libflac.scan_stream_host(streams[0].data)[0].sp)
    sp.total_samples = 0
    rate = int(sp.sample_rate)
    W = int(round(args.window * rate))
    fmt = libflac.OUT_INTERLEAVED32
    stride = libflac.out_stride(fmt, sp)

    dev = torch.device("cuda:0")
    dec = libflac.BatchDecoder(0)
    d_bytes = torch.from_numpy(buf).to(dev)
    d_files = torch.tensor([[b, e, 0, 0] for b, e, _, _ in table], dtype=torch.int64, device=dev).reshape(-1)
    nframes = sum(len(s.frame_offsets) for s in streams)
    nsamples = sum(int(s.nsamples) for s in streams)
    cap = nframes + 8
    corp = dec.index_corpus(d_bytes, nbytes, d_files.clone(), sp, cap=cap)
    torch.cuda.synchronize()
    info = libflac.info_array(corp.d_info.cpu().numpy())
    sf = corp.d_stream_frames.cpu().numpy().view(np.uint32)
    ss = corp.d_stream_samples.cpu().numpy().view(np.uint64)
    if corp.index_status.cpu().numpy()[0] != 0 or int(sf[-1]) != nframes or int(ss[-1]) != nsamples:
        print("the index is not the generator's: nothing is measured")
        return 1
    lines = [f"tools/sliding_bench.py --streams {n} --window {args.window} --hops {args.hops} --reps {args.reps}"
             + (" --default-cap" if args.default_cap else ""),
             f"{n} C2 streams, {nframes} frames, {nsamples} sample frames ({nsamples * stride} PCM bytes), {nbytes} bytes "
             f"resident, cap {cap}; a window is {W} sample frames ({W * stride} bytes a row)"]
    print("\n".join(lines), flush=True)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / CALLS

    def measure(label, corpus, reqs, check):
        """-> the report lines of one hop over one corpus, or None when the paths disagree"""
        k = len(reqs)
        d_reqs = torch.tensor(reqs, dtype=torch.int64, device=dev).reshape(-1)
        unshared = lambda: dec.decode_crops(corpus, d_reqs, W, fmt)
        shared = lambda: dec.decode_crops(corpus, d_reqs, W, fmt, shared=True, max_frames=nframes, max_samples=nsamples)
        out = [] if check else [f"{label}: {k} windows"]
        if check:  # ---- untimed: the results
            rows_u, st_u = unshared()
            rows_s, st_s = shared()
            torch.cuda.synchronize()
            word_u = st_u["select"].cpu().numpy().view(np.uint32).tolist()
            word_s = st_s["select"].cpu().numpy().view(np.uint32).tolist()
            F, S = (int(x) for x in st_s["totals"].cpu().numpy())
            sel_cap = k * ((W - 1) // sp.min_blocksize + 2)
            host_u = libflac.select_windows_host(info, cap, sf, ss, reqs, 0)
            host_s = libflac.select_windows_shared_host(info, cap, sf, ss, reqs, 0)
            hull_u = int(host_u[2][-1])
            same = bool(torch.equal(rows_u, rows_s))
            gen, at = True, 0
            for s in range(n):  # the requests are stream-major: stream s's rows are a strided view of its PCM
                mine = [r for r in reqs if r[0] == s]
                hop = mine[1][1] - mine[0][1] if len(mine) > 1 else W
                pcm = np.zeros((len(mine) * hop + W, sp.channels), np.int32)
                pcm[: len(streams[s].pcm)] = streams[s].pcm
                d_p = torch.from_numpy(pcm).to(dev)
                want = d_p.as_strided((len(mine), W, sp.channels), (hop * sp.channels, sp.channels, 1))
                gen = gen and bool(torch.equal(rows_s[at: at + len(mine)], want))
                at += len(mine)
            ok = (same and gen and word_u[0] == 0 and word_s[0] == 0 and word_u[1:] == host_u[4][1:].tolist()
                  and word_s[1:] == host_s[4][1:].tolist() and [F, S] == host_s[3].tolist()
                  and st_u["gather"].cpu().numpy().tolist() == [0, 0, 0, 0] and st_s["gather"].cpu().numpy().tolist() == [0, 0, 0, 0])
            out += [f"{label}: {k} windows, {k * W * stride} bytes of rows",
                    f"  shared=False: {word_u[1]} frames decoded (host twin {int(host_u[4][1])}), {hull_u * stride} PCM bytes decoded, "
                    f"{k * (W + 2 * (sp.max_blocksize - 1)) * stride} allocated, {sel_cap} records",
                    f"  shared=True:  {F} frames decoded (host twin {int(host_s[3][0])}), {S * stride} PCM bytes decoded, "
                    f"{nsamples * stride} allocated, {nframes} records; frames {word_u[1] / max(F, 1):.2f} times fewer",
                    f"  rows equal between the paths: {same}; rows equal the generator's PCM: {gen}"]
            del rows_u, rows_s
            if not ok:
                print("\n".join(out + ["the paths disagree: nothing is timed"]), flush=True)
                return None
        paths = (("shared=False", unshared), ("shared=True ", shared))
        for _ in range(WARMUP):
            for _, fn in paths:
                timed(fn)
        t = [[] for _ in paths]
        for _ in range(args.reps):
            for j, (_, fn) in enumerate(paths):
                t[j].append(timed(fn))
        for (name, _), x in zip(paths, t):
            out.append(f"  {name}: median {np.median(x):.3f} ms per call (min {min(x):.3f}, max {max(x):.3f}, "
                       f"{len(x)} reps of {CALLS} calls)")
        out.append(f"  shared=False / shared=True: {np.median(t[0]) / np.median(t[1]):.2f}")
        print("\n".join(out), flush=True)
        return out

    def sliding(hop):
        return [(s, first, W) for s in range(n) for first in range(0, int(streams[s].nsamples), hop)]

    hops = [float(x) for x in args.hops.split(",")]
    for h in hops:
        got = measure(f"hop {h:g} s", corp, sliding(int(round(h * rate))), True)
        if got is None:
            return 1
        lines += got
    if args.default_cap:
        big = dec.index_corpus(d_bytes, nbytes, d_files.clone(), sp)
        torch.cuda.synchronize()
        h = min(hops)
        got = measure(f"hop {h:g} s over an index with the default cap {big.cap} (rows not compared again)", big,
                      sliding(int(round(h * rate))), False)
        lines += got
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
