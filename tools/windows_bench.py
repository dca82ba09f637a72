#!/usr/bin/env python3
"""One window per stream of a batch: bnflac_select_ranges / bnflac_gather_ranges against the
whole-batch decode and per-stream slices they replace.

    python tools/windows_bench.py [--streams 64] [--reps 20] [--out profiles/select_ranges.txt]

64 C2 streams (seeds 2 + 1000 i) in one buffer, one window of a second (sample_rate sample frames)
at a random position in each, rows as BNFLAC_OUT_INTERLEAVED32 in a [streams, T, channels] tensor.
(a) the path without the two calls: index_streams -> decode_parsed of every frame -> the prefix
tables read back -> one torch slice per stream, stacked.  (b) index_streams -> select_ranges ->
decode_parsed over the selection -> gather_ranges, nothing read back.  Both are timed with device
events around work that ends in a synchronise, alternating, each warmed up; the gather call is
also timed alone (the C call on preallocated outputs, ten in a row between the events), in GB/s of
bytes read plus bytes written.  Untimed, the rows of (a) and (b) are
compared.  Each GPU step (check, time) runs as a child process under its own `timeout`; the first
failure ends the run.

    rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- \\
        python tools/windows_bench.py --step profile --reps 5

runs path (b) alone in this process (2 + reps times), for the per-kernel split.
"""
import argparse
import ctypes
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

STEP_LIMIT_S = {"check": 240, "time": 420}
GATHER_CALLS = 10
STEPS = sorted(STEP_LIMIT_S) + ["profile"]


def step(name, args):
    import torch
    from birdnest.audio_amd import libflac
    from index_bench import corpus
    buf, table, streams, sp = corpus(args.streams, pool=name != "profile")
    nbytes = len(buf) - 64
    n = args.streams
    nframes = sum(len(s.frame_offsets) for s in streams)
    T = int(sp.sample_rate)
    rng = np.random.default_rng(7)
    firsts = [int(rng.integers(0, s.nsamples - T)) for s in streams]
    dev = torch.device("cuda:0")
    d_bytes = torch.from_numpy(buf).to(dev)
    dec = libflac.BatchDecoder(0)
    fmt = libflac.OUT_INTERLEAVED32
    stride = libflac.out_stride(fmt, sp)
    cap = nframes + 8
    total_samples = sum(s.nsamples for s in streams)
    d_full = torch.zeros(total_samples * stride, dtype=torch.uint8, device=dev)  # (a)'s PCM, allocated once
    sel_cap = n * ((T - 1) // sp.min_blocksize + 2)
    d_compact = torch.zeros(n * (T + 2 * (sp.max_blocksize - 1)) * stride, dtype=torch.uint8, device=dev)
    d_ranges = torch.tensor([[f, T] for f in firsts], dtype=torch.int64, device=dev).reshape(-1)

    def path_a():
        _, _, d_info, d_sf, d_ss, _ = dec.index_streams(d_bytes, nbytes, table, sp, cap)
        nf = int(d_sf[-1].item())  # the tables come back: how many frames, where each stream landed
        dec.decode_parsed(d_bytes, nbytes, nf, sp, fmt, d_full, d_info)
        ss = d_ss.cpu().numpy()
        pcm = d_full.view(torch.int32).view(-1, sp.channels)
        rows = torch.stack([pcm[int(ss[i]) + f: int(ss[i]) + f + T] for i, f in enumerate(firsts)])
        torch.cuda.synchronize()
        return rows, nf

    def path_b():
        d_offs, _, d_info, d_sf, d_ss, _ = dec.index_streams(d_bytes, nbytes, table, sp, cap)
        _, d_sel_info, _, _, d_win, d_st = dec.select_ranges(d_offs, d_info, cap, d_sf, d_ss, n, d_ranges, sel_cap)
        dec.decode_parsed(d_bytes, nbytes, sel_cap, sp, fmt, d_compact, d_sel_info)
        d_rows, d_gst = dec.gather_ranges(d_compact, fmt, sp, d_win, n, T)
        torch.cuda.synchronize()
        return d_rows.view(torch.int32).view(n, T, sp.channels), d_st, d_gst, d_win

    if name == "check":
        rows_a, nf = path_a()
        rows_b, d_st, d_gst, _ = path_b()
        st, gst = d_st.cpu().numpy().tolist(), d_gst.cpu().numpy().tolist()
        want = np.stack([s.pcm[f: f + T] for s, f in zip(streams, firsts)])
        ok = (st[0] == 0 and gst == [0, 0, 0, 0] and nf == nframes and bool(torch.equal(rows_a, rows_b))
              and np.array_equal(rows_b.cpu().numpy(), want))
        print(f"{n} C2 streams, {nframes} frames, a window of {T} sample frames ({T * stride} bytes) in each")
        print(f"(a) decodes {nf} frames, (b) decodes {st[1]} (select status word 1) of {sel_cap} records")
        print("(a), (b) and the generator's PCM agree:", ok, flush=True)
        return 0 if ok else 1

    if name == "profile":  # path (b) alone, for a kernel trace (no worker processes)
        for _ in range(2 + args.reps):
            path_b()
        return 0

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(2):  # warm-up of both (scratch allocations, code objects)
        path_a()
        d_win = path_b()[3]
    ta, tb, tg = [], [], []
    for _ in range(args.reps):
        ta.append(timed(path_a))
        tb.append(timed(path_b))
    d_rows = torch.zeros(n * T * stride, dtype=torch.uint8, device=dev)
    d_gst = torch.zeros(4, dtype=torch.int32, device=dev)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    hs = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def gather():  # the C call itself on preallocated outputs, GATHER_CALLS times between the events
        for _ in range(GATHER_CALLS):
            if dec.L.bnflac_gather_ranges(dec.ctx, vp(d_compact), d_compact.numel(), fmt, ctypes.byref(sp), vp(d_win), n, T,
                                          T * stride, vp(d_rows), vp(d_gst), hs) != 0:
                raise RuntimeError(dec.L.bnflac_last_error().decode())

    gather()
    for _ in range(args.reps):
        tg.append(timed(gather) / GATHER_CALLS)
    for label, t in (("(a) index, decode every frame, slice per stream", ta), ("(b) index, select, decode, gather", tb)):
        print(f"{label}: median {np.median(t):.3f} ms (min {min(t):.3f}, max {max(t):.3f}, {len(t)} reps)")
    print(f"(a) / (b): {np.median(ta) / np.median(tb):.2f}")
    moved = 2 * n * T * stride
    print(f"gather_ranges alone ({n} rows of {T * stride} bytes, per call of {GATHER_CALLS} in a row): median {np.median(tg):.4f} ms "
          f"(min {min(tg):.4f}, max {max(tg):.4f}, {len(tg)} reps), {moved / np.median(tg) / 1e6:.1f} GB/s read + written",
          flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_ranges.txt"))
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
        f.write("tools/windows_bench.py --streams %d --reps %d\n" % (args.streams, args.reps))
        f.write("".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
