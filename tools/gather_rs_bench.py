#!/usr/bin/env python3
"""Windows at another sample rate: bnflac_gather_ranges_f32_rs against what a caller does today.

    python tools/gather_rs_bench.py [--reps 20] [--out profiles/gather_f32_rs.txt]

Both routes start from a decoded PCM on the device (16-bit stereo at 44.1 kHz in the
BNFLAC_OUT_FLACDECODER layout, 4 bytes per sample frame; random samples, the decode is not timed) and
a window table, and end in a float32[rows, channels, n_out] tensor at 48 kHz through the same
default design (resample_design(44100, 48000): 160 phases of 32 taps):
(a) today: gather_ranges_f32 into a preallocated float32[rows, channels, T], then the usual torch
    polyphase resampler: one conv1d with a kernel per output phase (160 output channels, stride 147),
    the phases interleaved by a transpose and cut to n_out;
(b) gather_ranges_f32_rs into a preallocated tensor, one launch.
Shape 1: 64 rows of 3 s.  Shape 2: 512 rows of 10 s, which leave the 256 MiB Infinity Cache.  Window r
starts r % 7 sample frames into its stretch so that the source phases differ.
Timed with device events around one route, the two alternating, after a warm-up of both; the median
of the repetitions counts.  Untimed, on shape 1, the two tensors are compared: they differ in
summation order, so not bit for bit but within (gamma_b + gamma_a) * sum_k |h_k x_k|, gamma_b the
bound of the library's order (n = K / 4 + 2) and gamma_a that of any order over the conv kernel's
width.  The GPU work runs as a child process under its own `timeout`; a failure ends the run.
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_LIMIT_S = 540
HBM_ACHIEVABLE = 6.3e12  # bytes per second: a float4 copy on this part
RATE_IN, RATE_OUT = 44100, 48000
SHAPES = [("shape 1", 64, 3), ("shape 2", 512, 10)]
U = 2.0 ** -24


def step(args):
    import torch
    from birdnest.audio_amd import libflac
    dev = torch.device("cuda:0")
    dec = libflac.BatchDecoder(0)
    sp = libflac.StreamParams(1, 4096, 4096, RATE_IN, 2, 16, 0)
    fmt = libflac.f32_layout(sp)
    stride, ch = libflac.out_stride(fmt, sp), sp.channels
    spec, taps = libflac.resample_design(RATE_IN, RATE_OUT)
    L, M, K = spec.up, spec.down, spec.taps
    c0 = K // 2 - 1
    d_taps = torch.from_numpy(taps.reshape(-1)).to(dev)
    # route (a)'s kernels: output j = m L + p reads x from m M + floor(p M / L) - c0 with the taps of phase p M mod L
    shift = np.arange(L) * M // L
    Kw = K + int(shift.max())
    W = np.zeros((L, 1, Kw), np.float32)
    for p in range(L):
        W[p, 0, shift[p]: shift[p] + K] = taps[p * M % L]
    d_W = torch.from_numpy(W).to(dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    ok = True
    for label, rows, seconds in SHAPES:
        T = seconds * RATE_IN
        n_out = -(-T * L // M)
        g = torch.Generator(device=dev)
        g.manual_seed(rows)
        d_pcm = torch.randint(0, 256, (((rows * T + 8) * stride + 15) // 16 * 16,), dtype=torch.uint8, device=dev, generator=g)
        win = np.zeros(rows, dtype=libflac.WINDOW_DTYPE)
        for r in range(rows):
            win[r] = (r * T + r % 7, T, 0, 0, 0, 0)
        d_win = torch.from_numpy(win.view(np.uint8).reshape(-1).copy()).to(dev)
        d_planes = torch.empty(rows * ch * T, dtype=torch.float32, device=dev)
        d_out = torch.empty(rows * ch * n_out, dtype=torch.float32, device=dev)
        nm = -(-n_out // L)  # conv positions: m = 0 .. nm - 1
        right = max(0, (nm - 1) * M + Kw - (T + c0))

        def conv(x, w):
            y = torch.nn.functional.conv1d(torch.nn.functional.pad(x.reshape(rows * ch, 1, T), (c0, right)), w, stride=M)
            return y.transpose(1, 2).reshape(rows, ch, -1)[:, :, :n_out]

        def route_a():
            x = dec.gather_ranges_f32(d_pcm, fmt, sp, d_win, rows, T, d_out=d_planes)[0]
            return conv(x, d_W).contiguous()

        def route_b():
            return dec.gather_ranges_f32_rs(d_pcm, fmt, sp, d_win, rows, spec, d_taps, n_out, d_out=d_out)[0]

        for _ in range(3):  # warm-up of both: code objects, the convolution's solver, the allocator's blocks
            a = route_a()
            b = route_b()
        torch.cuda.synchronize()
        if rows <= 64:
            x = dec.gather_ranges_f32(d_pcm, fmt, sp, d_win, rows, T, d_out=d_planes)[0]
            mag = conv(x.abs(), d_W.abs())
            ga, gb = Kw * U / (1 - Kw * U), (K // 4 + 2) * U / (1 - (K // 4 + 2) * U)
            ratio = ((a - b).abs().double() / ((ga + gb) * mag.double()).clamp_min(1e-300)).max().item()
            agree = ratio <= 1.0 and bool(torch.isfinite(b).all())
            print(f"{label}: (a) and (b) agree within (gamma_a + gamma_b) sum |h x|: {agree} (the largest difference is "
                  f"{ratio:.3f} of the bound; largest |a - b| {(a - b).abs().max().item():.3e})")
            ok = ok and agree
            del x, mag
        del a, b
        ta, tb = [], []
        for _ in range(args.reps):
            ta.append(timed(route_a))
            tb.append(timed(route_b))
        moved = rows * (T * stride + 4 * ch * n_out)
        print(f"{label}: {rows} rows of {T} sample frames -> {n_out} outputs, {ch} channels, {sp.bps} bits, {L}/{M}, {K} taps")
        for name, t in (("(a) gather_ranges_f32, then conv1d (%d kernels of %d, stride %d), transpose, cut" % (L, Kw, M), ta),
                        ("(b) gather_ranges_f32_rs (1 launch)", tb)):
            print(f"  {name}: median {np.median(t):.4f} ms (min {min(t):.4f}, max {max(t):.4f}, {len(t)} reps)")
        rate = moved / (np.median(tb) * 1e-3)
        fma = rows * ch * n_out * K
        print(f"  (b) must move {moved} bytes ({stride} read per sample frame, {4 * ch} written per output): {rate / 1e9:.1f} GB/s, "
              f"{100 * rate / HBM_ACHIEVABLE:.1f} % of {HBM_ACHIEVABLE / 1e12:.1f} TB/s")
        print(f"  (b) {K} FMAs per output and plane, {fma} in all: {fma / (np.median(tb) * 1e-3) / 1e12:.2f} T FMA/s; "
              f"(a) multiplies {Kw} per output, {Kw - K} of them by zero")
        print(f"  (a) median / (b) median: {np.median(ta) / np.median(tb):.2f}; (b) median below (a) minimum: {np.median(tb) < min(ta)}",
              flush=True)
        del d_pcm, d_planes, d_out
        torch.cuda.empty_cache()
    print("not measured: other ratios and tap counts, the 24-bit and 8-channel layouts, mono, LDS bank-conflict counters, "
          "a resampler of another library, more than one process on the device")
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gather_f32_rs.txt"))
    ap.add_argument("--step", action="store_true")
    args = ap.parse_args()
    if args.step:
        return step(args)
    cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--step", "--reps", str(args.reps)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)  # the child's stderr goes to ours, not into the file
    print(r.stdout, end="", flush=True)
    if r.returncode != 0:
        print(f"the run failed with exit status {r.returncode}")
        return 1
    with open(args.out, "w") as f:
        f.write("tools/gather_rs_bench.py --reps %d\n" % args.reps)
        f.write(r.stdout)
    return 0


if __name__ == "__main__":
    sys.exit(main())
