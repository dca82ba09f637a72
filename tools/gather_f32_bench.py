#!/usr/bin/env python3
"""Windows as float32 channel planes: bnflac_gather_ranges_f32 against the route it replaces.

    python tools/gather_f32_bench.py [--streams 64] [--reps 20] [--out profiles/gather_f32.txt]

Both routes start from a decoded selection (the decode is not timed) and end in the same
float32[rows, channels, T] tensor:
(a) what the library offered before: gather_ranges on a BNFLAC_OUT_INTERLEAVED32 PCM into preallocated
    rows, then rows.view(int32).view(rows, T, channels).permute(0, 2, 1).to(float32) * 2^-(bps - 1) in
    torch;
(b) gather_ranges_f32 into a preallocated tensor, on the PCM in the layout decode_windows_f32 picks
    (BNFLAC_OUT_FLACDECODER for 16-bit stereo: 4 bytes per sample frame).
Shape 1, the windows_bench shape: 64 C2 streams (seeds 2 + 1000 i), one window of a second at a
random position in each, decoded by the chain of decode_windows.  Shape 2, rows that leave the
256 MiB Infinity Cache: 512 rows of ten seconds, over the compact PCM of shape 1 tiled until it
holds them (the same samples in both layouts), window r starting r % 7 sample frames into its ten
seconds so that the source phases differ.
Timed with device events around one route, the two alternating, after a warm-up of both; untimed,
the two tensors are compared bit for bit.  The GPU work runs as a child process under its own
`timeout`; a failure ends the run.
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

STEP_LIMIT_S = 540
HBM_ACHIEVABLE = 6.3e12  # bytes per second: a float4 copy on this part
LARGE_ROWS, LARGE_SECONDS = 512, 10


def step(args):
    import torch
    from birdnest.audio_amd import libflac
    from index_bench import corpus
    buf, table, streams, sp = corpus(args.streams)
    nbytes = len(buf) - 64
    n = args.streams
    T = int(sp.sample_rate)
    rng = np.random.default_rng(7)
    firsts = [int(rng.integers(0, s.nsamples - T)) for s in streams]
    dev = torch.device("cuda:0")
    d_bytes = torch.from_numpy(buf).to(dev)
    dec = libflac.BatchDecoder(0)
    s = torch.cuda.current_stream()
    files = [(b, e) for b, e, _, _ in table]
    cap = sum(len(x.frame_offsets) for x in streams) + 8
    fmt_a, fmt_b = libflac.OUT_INTERLEAVED32, libflac.f32_layout(sp)
    ch, k = sp.channels, 2.0 ** -(sp.bps - 1)
    stride_a, stride_b = libflac.out_stride(fmt_a, sp), libflac.out_stride(fmt_b, sp)
    pcm_a, win_a, _, st_a = dec._decode_selection(d_bytes, nbytes, files, firsts, T, sp, fmt_a, cap, 0, s)
    pcm_b, win_b, _, st_b = dec._decode_selection(d_bytes, nbytes, files, firsts, T, sp, fmt_b, cap, 0, s)
    torch.cuda.synchronize()
    for st in (st_a, st_b):
        assert st["index"].cpu().numpy()[0] == 0 and st["select"].cpu().numpy()[0] == 0
    want = np.stack([x.pcm[f: f + T] for x, f in zip(streams, firsts)]).transpose(0, 2, 1).astype(np.float32) * np.float32(k)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def shape(label, rows, R, d_pa, d_wa, d_pb, d_wb, expect):
        d_rows = torch.empty(rows * R * stride_a, dtype=torch.uint8, device=dev)
        d_out = torch.empty(rows * ch * R, dtype=torch.float32, device=dev)

        def route_a():
            dec.gather_ranges(d_pa, fmt_a, sp, d_wa, rows, R, d_rows=d_rows)
            return d_rows.view(torch.int32).view(rows, R, ch).permute(0, 2, 1).to(torch.float32) * k

        def route_b():
            return dec.gather_ranges_f32(d_pb, fmt_b, sp, d_wb, rows, R, d_out=d_out)[0]

        for _ in range(3):  # warm-up of both: code objects, the allocator's blocks
            a = route_a()
            b = route_b()
        torch.cuda.synchronize()
        equal = bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))
        if expect is not None:
            equal = equal and np.array_equal(b.cpu().numpy().view(np.uint32), expect.view(np.uint32))
        del a, b
        ta, tb = [], []
        for _ in range(args.reps):
            ta.append(timed(route_a))
            tb.append(timed(route_b))
        moved = rows * R * (stride_b + 4 * ch)
        print(f"{label}: {rows} rows of {R} sample frames, {ch} channels, {sp.bps} bits")
        for name, t in (("(a) gather_ranges on INTERLEAVED32, then torch (4 launches)", ta),
                        ("(b) gather_ranges_f32 on the %d-byte layout (1 launch)" % stride_b, tb)):
            print(f"  {name}: median {np.median(t):.4f} ms (min {min(t):.4f}, max {max(t):.4f}, {len(t)} reps)")
        rate = moved / (np.median(tb) * 1e-3)
        print(f"  (b) must move {moved} bytes ({stride_b} read + {4 * ch} written per sample frame): {rate / 1e9:.1f} GB/s, "
              f"{100 * rate / HBM_ACHIEVABLE:.1f} % of {HBM_ACHIEVABLE / 1e12:.1f} TB/s")
        print(f"  (a) median / (b) median: {np.median(ta) / np.median(tb):.2f}; (b) median below (a) minimum: {np.median(tb) < min(ta)}")
        print(f"  (a) and (b) bit-equal: {equal}", flush=True)
        return equal

    ok = shape("shape 1", n, T, pcm_a, win_a, pcm_b, win_b, want)
    # shape 2: the compact PCM of shape 1, tiled
    R2 = LARGE_SECONDS * T
    frames1 = n * (T + 2 * (sp.max_blocksize - 1))
    need = LARGE_ROWS * R2 + 8
    reps = (need + frames1 - 1) // frames1
    big_a = pcm_a[: frames1 * stride_a].repeat(reps)
    big_b = pcm_b[: frames1 * stride_b].repeat(reps)
    win = np.zeros(LARGE_ROWS, dtype=libflac.WINDOW_DTYPE)
    for r in range(LARGE_ROWS):
        win[r] = (r * R2 + r % 7, R2, 0, 0, 0, 0)
    d_win = torch.from_numpy(win.view(np.uint8).reshape(-1).copy()).to(dev)
    ok = shape("shape 2", LARGE_ROWS, R2, big_a, d_win, big_b, d_win, None) and ok
    print("not measured: the 24-bit and 8-channel layouts, mono, LDS bank-conflict counters, a register-only "
          "path for the 4-byte stride, more than one process on the device")
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gather_f32.txt"))
    ap.add_argument("--step", action="store_true")
    args = ap.parse_args()
    if args.step:
        return step(args)
    cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--step",
           "--streams", str(args.streams), "--reps", str(args.reps)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)  # the child's stderr goes to ours, not into the file
    print(r.stdout, end="", flush=True)
    if r.returncode != 0:
        print(f"the run failed with exit status {r.returncode}")
        return 1
    with open(args.out, "w") as f:
        f.write("tools/gather_f32_bench.py --streams %d --reps %d\n" % (args.streams, args.reps))
        f.write(r.stdout)
    return 0


if __name__ == "__main__":
    sys.exit(main())
