#!/usr/bin/env python3
"""Windows as mel spectrograms: bnflac_gather_ranges_mel against what a caller does today.

    python tools/gather_mel_bench.py [--reps 20] [--out profiles/gather_mel.txt]

Both routes start from a decoded PCM on the device (16-bit stereo at 48 kHz in the
BNFLAC_OUT_FLACDECODER layout, 4 bytes per sample frame; random samples, the decode is not timed) and
a window table, and end in a float32[rows, channels, 128, frames] tensor through the same design
(mel_design(48000, 1024, 256, 128): a periodic Hann window, 128 HTK triangles):
(a) today: gather_ranges_f32 into a preallocated float32[rows, channels, T], then torch.stft(
    center=True, pad_mode="constant", window=hann), abs() ** 2 and a matmul with the dense
    [128, 513] filterbank into a preallocated tensor;
(b) gather_ranges_mel into a preallocated tensor, one launch.
Shape 1: 64 rows of 3 s.  Shape 2: 512 rows of 10 s.  Window r starts r % 7 sample frames into its
stretch so that the source phases differ.
Timed with device events around one route, the two alternating, after a warm-up of both; the median
of the repetitions counts.  Untimed, on shape 1, the two tensors are compared: they differ in the
FFT's algorithm and the summation order, so not bit for bit but within the sum of their bounds
(DESIGN.md "Windows as mel spectrograms"): for each the FFT's norm-wise bound E, dP = (2 |X| E + E^2)
(1 + gamma_2) + gamma_2 |X|^2, and sum |w| dP + gamma_n sum |w| (P + dP) with n the longest band for
(b) and all 513 bins for (a)'s dense product; |X| and the frames' norms come from a float64 STFT.
The GPU work runs as a child process under its own `timeout`; a failure ends the run.
"""
import argparse
import math
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_LIMIT_S = 540
HBM_ACHIEVABLE = 6.3e12  # bytes per second: a float4 copy on this part
RATE, N_FFT, HOP, N_MELS = 48000, 1024, 256, 128
SHAPES = [("shape 1", 64, 3), ("shape 2", 512, 10)]
U = 2.0 ** -24


def gam(n):
    return n * U / (1 - n * U)


def step(args):
    import torch
    from birdnest.audio_amd import libflac
    dev = torch.device("cuda:0")
    dec = libflac.BatchDecoder(0)
    sp = libflac.StreamParams(1, 4096, 4096, RATE, 2, 16, 0)
    fmt = libflac.f32_layout(sp)
    stride, ch = libflac.out_stride(fmt, sp), sp.channels
    spec, tab, bands = libflac.mel_design(RATE, N_FFT, HOP, N_MELS)
    N, half = N_FFT, N_FFT // 2 + 1
    d_tab = torch.from_numpy(tab).to(dev)
    d_bands = torch.from_numpy(bands.reshape(-1).view(np.int32).copy()).to(dev)
    fb = np.zeros((N_MELS, half), np.float32)  # route (a)'s dense filterbank: the same weights
    nb_max = 0
    for m in range(N_MELS):
        f, w0, w1 = int(bands[m, 0]), int(bands[m, 1]), int(bands[m + 1, 1])
        fb[m, f: f + w1 - w0] = tab[2 * N + w0: 2 * N + w1]
        nb_max = max(nb_max, w1 - w0)
    d_fb = torch.from_numpy(fb).to(dev)
    d_hann = d_tab[:N].clone()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    ok = True
    for label, rows, seconds in SHAPES:
        T = seconds * RATE
        frames = 1 + T // HOP
        g = torch.Generator(device=dev)
        g.manual_seed(rows)
        d_pcm = torch.randint(0, 256, (((rows * T + 8) * stride + 15) // 16 * 16,), dtype=torch.uint8, device=dev, generator=g)
        win = np.zeros(rows, dtype=libflac.WINDOW_DTYPE)
        for r in range(rows):
            win[r] = (r * T + r % 7, T, 0, 0, 0, 0)
        d_win = torch.from_numpy(win.view(np.uint8).reshape(-1).copy()).to(dev)
        d_planes = torch.empty(rows * ch * T, dtype=torch.float32, device=dev)
        d_mel_a = torch.empty((rows * ch, N_MELS, frames), dtype=torch.float32, device=dev)
        pitch = (frames + 3) // 4 * 4
        d_mel_b = torch.empty(rows * ch * N_MELS * pitch, dtype=torch.float32, device=dev)

        def route_a():
            x = dec.gather_ranges_f32(d_pcm, fmt, sp, d_win, rows, T, d_out=d_planes)[0]
            S = torch.stft(x.reshape(rows * ch, T), N, hop_length=HOP, window=d_hann, center=True, pad_mode="constant",
                           return_complex=True)
            torch.matmul(d_fb, S.abs() ** 2, out=d_mel_a)
            return d_mel_a.view(rows, ch, N_MELS, frames)

        def route_b():
            return dec.gather_ranges_mel(d_pcm, fmt, sp, d_win, rows, spec, d_tab, d_bands, frames, d_out=d_mel_b, frame_pitch=pitch)[0]

        for _ in range(3):  # warm-up of both: code objects, the FFT's plan, the allocator's blocks
            a = route_a()
            b = route_b()
        torch.cuda.synchronize()
        if rows <= 64:
            x = dec.gather_ranges_f32(d_pcm, fmt, sp, d_win, rows, T, d_out=d_planes)[0].reshape(rows * ch, T).double()
            w64 = d_hann.double()
            X = torch.stft(x, N, hop_length=HOP, window=w64, center=True, pad_mode="constant", return_complex=True).abs()
            norm = torch.nn.functional.pad(x, (N // 2, N // 2)).unfold(1, N, HOP).mul(w64).pow(2).sum(dim=2).sqrt()  # ||w x||_2 per frame
            t = int(math.log2(N))
            eta = U + gam(4) * (math.sqrt(2.0) + U)
            E = ((t * eta / (1 - t * eta) * (1 + U) + U) * math.sqrt(N) * norm).unsqueeze(1)
            P = X * X
            dP = (2 * X * E + E * E) * (1 + gam(2)) + gam(2) * P
            fa = d_fb.double().abs()
            bound = 2 * torch.matmul(fa, dP) + (gam(nb_max) + gam(half)) * torch.matmul(fa, P + dP)
            diff = (a.reshape(rows * ch, N_MELS, frames) - b.reshape(rows * ch, N_MELS, frames)).abs().double()
            ratio = (diff / bound.clamp_min(1e-300)).max().item()
            ref = torch.matmul(d_fb.double(), P)
            err_b = ((b.reshape(rows * ch, N_MELS, frames).double() - ref).abs() / ref.abs().clamp_min(1e-300)).max().item()
            err_a = ((a.reshape(rows * ch, N_MELS, frames).double() - ref).abs() / ref.abs().clamp_min(1e-300)).max().item()
            agree = ratio <= 1.0 and bool(torch.isfinite(b).all())
            print(f"{label}: (a) and (b) agree within the sum of their bounds: {agree} (the largest difference is {ratio:.4f} of the "
                  f"bound; largest relative error against float64: (a) {err_a:.3e}, (b) {err_b:.3e})")
            ok = ok and agree
            del x, X, norm, E, P, dP, bound, diff, ref
        del a, b
        ta, tb = [], []
        for _ in range(args.reps):
            ta.append(timed(route_a))
            tb.append(timed(route_b))
        moved = rows * (T * stride + 4 * ch * N_MELS * frames)
        print(f"{label}: {rows} rows of {T} sample frames -> {frames} frames of {N_MELS} bands, {ch} channels, {sp.bps} bits, "
              f"n_fft {N}, hop {HOP}")
        for name, tt in (("(a) gather_ranges_f32, torch.stft, abs() ** 2, matmul with [128, 513]", ta),
                         ("(b) gather_ranges_mel (1 launch)", tb)):
            print(f"  {name}: median {np.median(tt):.4f} ms (min {min(tt):.4f}, max {max(tt):.4f}, {len(tt)} reps)")
        rate = moved / (np.median(tb) * 1e-3)
        nfft = rows * ch * frames
        print(f"  (b) must move {moved} bytes ({stride} read per sample frame, {4 * N_MELS} written per frame and plane): "
              f"{rate / 1e9:.1f} GB/s, {100 * rate / HBM_ACHIEVABLE:.2f} % of {HBM_ACHIEVABLE / 1e12:.1f} TB/s")
        print(f"  (b) {nfft} FFTs of {N} complex points: {nfft / (np.median(tb) * 1e-3) / 1e6:.1f} M FFT/s, "
              f"{nfft * 5 * N * 8 * 2 / (np.median(tb) * 1e-3) / 1e12:.2f} TB/s of LDS traffic in the stages alone "
              f"(5 passes reading and writing {8 * N} bytes)")
        print(f"  (a) median / (b) median: {np.median(ta) / np.median(tb):.2f}; (b) median below (a) minimum: {np.median(tb) < min(ta)}",
              flush=True)
        del d_pcm, d_planes, d_mel_a, d_mel_b
        torch.cuda.empty_cache()
    print("not measured: other FFT sizes, hops and band counts, the 24-bit and 8-channel layouts, mono, LDS bank-conflict "
          "counters, a real-input FFT, a spectrogram of another library, more than one process on the device")
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gather_mel.txt"))
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
        f.write("tools/gather_mel_bench.py --reps %d\n" % args.reps)
        f.write(r.stdout)
    return 0


if __name__ == "__main__":
    sys.exit(main())
