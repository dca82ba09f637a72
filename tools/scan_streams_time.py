#!/usr/bin/env python3
"""bnflac_scan_streams next to the call it feeds and the host route it replaces.

    python tools/scan_streams_time.py [--reps 20] [--out profiles/scan_streams.txt]

Two batches, each in one buffer:
  c2     64 C2 streams (seeds 2 + 1000 i), the batch of tools/index_bench.py
  small  4,096 streams of a header and one C2 frame, back to back (every byte alignment)
For each batch, one warm call and then the median of `reps` calls of
  scan   bnflac_scan_streams on preallocated outputs, device events around the call
  index  the bnflac_index_streams call it feeds (the table the scan wrote), device events
  host   the route the library had until now: a copy of each stream's first 4 KiB to the host,
         bnflac_scan_stream_host per stream, the table copied to the device (wall clock around
         work that ends in a synchronise)
Untimed, the scan's table is compared with the host route's.  Each batch runs as a child process
under its own `timeout`; the first failure ends the run.
"""
import argparse
import ctypes
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_LIMIT_S = {"c2": 420, "small": 300}
HEAD = 4096  # bytes of each stream the host route copies back


def _encode(i):
    from birdnest.audio_amd import synth
    return synth.encode(synth.config("C2", seed=2 + 1000 * i))


def corpus(name):
    """-> (host buffer with 64 spare bytes, [(begin, end)], frames in total, shared params)"""
    from birdnest.audio_amd import libflac, synth
    sp = libflac.StreamParams.from_synth(synth.config("C2"), 0)
    if name == "c2":
        import multiprocessing
        with multiprocessing.get_context("fork").Pool(16) as workers:  # before the GPU is touched
            streams = workers.map(_encode, range(64))
        datas = [s.data for s in streams]
        nframes = sum(len(s.frame_offsets) for s in streams)
        pad = 256
    else:
        one = synth.encode(synth.config("C2", nframes=1, seed=5))
        datas = [one.data] * 4096
        nframes = 4096
        pad = 1
    lens = [(len(d) + pad - 1) // pad * pad for d in datas]
    base = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    buf = np.zeros(int(base[-1]) + 64, np.uint8)
    ranges = []
    for b, d in zip(base, datas):
        buf[int(b):int(b) + len(d)] = d
        ranges.append((int(b), int(b) + len(d)))
    return buf, ranges, nframes, sp


def step(name, args):
    import torch
    from birdnest.audio_amd import libflac
    buf, ranges, nframes, sp = corpus(name)
    n, nbytes = len(ranges), len(buf) - 64
    dev = torch.device("cuda:0")
    dec = libflac.BatchDecoder(0)
    L = dec.L
    d_bytes = torch.from_numpy(buf).to(dev)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    hs = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    table = np.zeros(n, dtype=libflac.STREAM_DESC_DTYPE)
    table["begin"], table["end"] = [b for b, _ in ranges], [e for _, e in ranges]
    d_tab = torch.from_numpy(table.view(np.int64).reshape(-1).copy()).to(dev)
    d_meta = torch.zeros(n * libflac.STREAM_META_BYTES, dtype=torch.uint8, device=dev)
    d_md5 = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    d_st = torch.zeros(4, dtype=torch.int32, device=dev)
    cap = nframes + 8
    d_offs = torch.zeros(cap, dtype=torch.int64, device=dev)
    d_os = torch.zeros(cap, dtype=torch.int64, device=dev)
    d_info = torch.zeros(cap * libflac.FRAME_INFO_BYTES, dtype=torch.uint8, device=dev)
    d_sf = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    d_ss = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_ist = torch.zeros(4, dtype=torch.int32, device=dev)

    def scan():
        if L.bnflac_scan_streams(dec.ctx, vp(d_bytes), nbytes, vp(d_tab), n, ctypes.byref(sp), vp(d_meta), vp(d_md5),
                                 vp(d_st), hs) != 0:
            raise RuntimeError(L.bnflac_last_error().decode())

    def index():
        if L.bnflac_index_streams(dec.ctx, vp(d_bytes), nbytes, vp(d_tab), n, ctypes.byref(sp), 0, vp(d_offs), vp(d_os),
                                  vp(d_info), cap, vp(d_sf), vp(d_ss), vp(d_ist), hs) != 0:
            raise RuntimeError(L.bnflac_last_error().decode())

    host_tab = {}

    def host():
        t = np.zeros(n, dtype=libflac.STREAM_DESC_DTYPE)
        for k, (b, e) in enumerate(ranges):
            head = d_bytes[b:min(e, b + HEAD)].cpu().numpy()
            meta, _ = libflac.scan_stream_host(head)
            ok = meta.status == libflac.SCAN_OK
            t[k] = (b, e, b + meta.first_offset if ok else e, meta.sp.total_samples if ok else 0)
        host_tab["d"] = torch.from_numpy(t.view(np.int64).reshape(-1)).to(dev)
        torch.cuda.synchronize()

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    out = {}
    for label, fn, clock in (("scan", scan, events), ("index", index, events), ("host", host, wall)):
        clock(fn)  # warm
        out[label] = [clock(fn) for _ in range(args.reps)]
    ok = (d_st.cpu().tolist() == [0, n, 0, 0] and int(d_ist[0]) == 0 and int(d_sf[-1]) == nframes
          and torch.equal(host_tab["d"], d_tab))
    what = "64 C2 streams" if name == "c2" else "4,096 streams of a header and one C2 frame"
    print(f"{name}: {what}, {nbytes / 1e6:.1f} MB, {nframes} frames")
    for label, text in (("scan", "bnflac_scan_streams"), ("index", "bnflac_index_streams on the scan's table"),
                        ("host", f"host route (first {HEAD} bytes of each stream to the host, bnflac_scan_stream_host, "
                                 "table to the device)")):
        t = out[label]
        print(f"  {text}: median {np.median(t):.4f} ms (min {min(t):.4f}, max {max(t):.4f}, {len(t)} calls after one warm call)")
    print(f"  scan / index: {np.median(out['scan']) / np.median(out['index']):.4f}; host route / scan: "
          f"{np.median(out['host']) / np.median(out['scan']):.1f}")
    print("  every stream kept, every frame indexed, the scan's table equals the host route's:", bool(ok), flush=True)
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_streams.txt"))
    ap.add_argument("--step", choices=sorted(STEP_LIMIT_S))
    args = ap.parse_args()
    if args.step:
        return step(args.step, args)
    lines = []
    for name in ("c2", "small"):
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S[name]), sys.executable, os.path.abspath(__file__), "--step", name,
               "--reps", str(args.reps)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)  # stderr passes through, not into the file
        print(r.stdout, end="", flush=True)
        lines.append(r.stdout)
        if r.returncode != 0:  # nothing more on the GPU after a failure
            print(f"step {name} failed with exit status {r.returncode}")
            return 1
    with open(args.out, "w") as f:
        f.write("tools/scan_streams_time.py --reps %d\n" % args.reps)
        f.write("".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
