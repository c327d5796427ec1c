"""Times vti_convert_raw on the device: microseconds per call by device events after warm-up, the bytes a call
moves (raw read plus 3*H0*W0 written) over that time as a share of the HBM peak, a torch device-to-device copy of the same total
traffic in the same run as the yardstick for "memory-bound", the pinned H2D time of the raw batch against the BGR batch, and a
FrameFeeder predict loop with BGR slots against fmt="yuyv" slots (alternating).  Prints one JSON line per measurement.

    python tools/rawframes_bench.py [--frames 64] [--iters 50] [--feeder-steps 30] [--dtype h2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vti_amd  # noqa: E402
from vti_amd import rawframes as R  # noqa: E402

HBM_PEAK_GBS = 8000.0       # MI355X: 8 TB/s


def device_us(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def line(**kw):
    print(json.dumps(kw), flush=True)


def d2d_us(total_bytes, iters):
    """A torch copy whose read plus write traffic is total_bytes."""
    src = torch.empty(total_bytes // 2, dtype=torch.uint8, device="cuda").random_(0, 256)
    dst = torch.empty_like(src)
    return device_us(lambda: dst.copy_(src), iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--feeder-steps", type=int, default=30)
    ap.add_argument("--dtype", default="h2")
    ap.add_argument("--feeder-only", action="store_true", help="skip the kernel and copy timings")
    ap.add_argument("--own-copy-streams", action="store_true",
                    help="leave each FrameFeeder its own copy stream (default: both rings share one, so the comparison does not depend "
                         "on which hardware queue a stream happens to be mapped to)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a ROCm GPU")
    n, H0, W0 = args.frames, 960, 1280
    eng = vti_amd.Engine("n", 2, H=64, W=64, max_batch=max(n, 64))
    g = torch.Generator(device="cuda").manual_seed(0)

    if not args.feeder_only:
        # ---- the uniform call, every format ----
        out = torch.empty((n, H0, W0, 3), dtype=torch.uint8, device="cuda")
        for fmt in sorted(R.FORMATS, key=R.FORMATS.get):
            fb = R.frame_bytes(fmt, H0, W0)
            raw = torch.randint(0, 256, (n * fb,), dtype=torch.uint8, device="cuda", generator=g)
            us = device_us(lambda: eng.convert_raw(raw, fmt, H0, W0, out=out), args.iters)
            total = n * fb + out.numel()
            copy = d2d_us(total, args.iters)
            line(what="vti_convert_raw", fmt=fmt, frames=n, H0=H0, W0=W0, us_per_call=round(us, 1), bytes_per_call=total,
                 gb_per_s=round(total / us / 1e3, 1), share_of_hbm_peak=round(total / us / 1e3 / HBM_PEAK_GBS, 3),
                 d2d_copy_same_bytes_us=round(copy, 1), ratio_to_d2d_copy=round(us / copy, 2))

        # ---- the ragged call: 16 frames of each of four sizes ----
        sizes = [(480, 332), (720, 960), (960, 1280), (1080, 1920)]
        for fmts in (["yuyv"], ["nv12"], ["yuyv", "nv12", "uyvy", "i420"]):
            shapes = [s for s in sizes for _ in range(16)]
            ff = [fmts[k % len(fmts)] for k in range(len(shapes))]
            big = vti_amd.Engine("n", 2, H=640, W=640, max_batch=len(shapes))
            rt = big.pack_raw_frames(shapes, ff, "cuda")
            table = big.pack_frames(shapes, "cuda")[0]
            raw = torch.randint(0, 256, (rt.raw_bytes,), dtype=torch.uint8, device="cuda", generator=g)
            dst = torch.empty(table.total_bytes, dtype=torch.uint8, device="cuda")
            us = device_us(lambda: big.convert_raw_frames(raw, rt, table, out=dst), args.iters)
            total = sum(rt.frame_bytes) + sum(3 * h * w for h, w in shapes)
            copy = d2d_us(total, args.iters)
            line(what="vti_convert_raw_frames", fmts=fmts, frames=len(shapes), sizes=sizes, us_per_call=round(us, 1), bytes_per_call=total,
                 gb_per_s=round(total / us / 1e3, 1), share_of_hbm_peak=round(total / us / 1e3 / HBM_PEAK_GBS, 3),
                 d2d_copy_same_bytes_us=round(copy, 1), ratio_to_d2d_copy=round(us / copy, 2))

        # ---- the bus: pinned H2D of the raw batch against the BGR batch ----
        for name, nbytes in (("bgr", n * 3 * H0 * W0), ("yuyv", n * R.frame_bytes("yuyv", H0, W0)), ("nv12", n * R.frame_bytes("nv12", H0, W0))):
            host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
            dev = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            us = device_us(lambda: dev.copy_(host, non_blocking=True), max(args.iters // 5, 5), warmup=2)
            line(what="pinned H2D", batch=name, frames=n, bytes=nbytes, us_per_copy=round(us, 1), gb_per_s=round(nbytes / us / 1e3, 2))

    # ---- FrameFeeder predict loop: BGR slots against yuyv slots, alternating ----
    Bf = 32
    H, W = vti_amd.letterbox_shape(H0, W0, 640)
    net = vti_amd.Engine("n", 2, H=H, W=W, max_batch=Bf, dtype=args.dtype)
    net.load_weights(vti_amd.random_weights(net, seed=1, cls_bias=-2.0), 0)
    outs = net.alloc_outputs(Bf, 100, Bf * 100, "bits", "cuda")
    feeders = {"bgr": vti_amd.FrameFeeder(Bf, H0, W0, depth=3, device=0), "yuyv": vti_amd.FrameFeeder(Bf, H0, W0, depth=3, device=0, fmt="yuyv")}
    if not args.own_copy_streams:
        feeders["yuyv"].copy_stream = feeders["bgr"].copy_stream
    rng = np.random.Generator(np.random.PCG64(0))
    for f in feeders.values():
        for s in range(f.depth):
            v = f.host_view(s)
            v[...] = rng.integers(0, 256, v.shape, dtype=np.uint8)

    def loop(f, steps):
        slots = [f.submit(f.next_slot())]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            nxt = f.next_slot()
            f.host_view(nxt)                  # waits only if that slot's previous copy is still in flight
            slots.append(f.submit(nxt))
            f.predict_into(net, slots.pop(0), outs, max_det=100)
        torch.cuda.synchronize()
        return steps * Bf / (time.perf_counter() - t0)
    for f in feeders.values():
        loop(f, 5)
    for rep in range(2):
        for name, f in feeders.items():
            line(what="FrameFeeder predict loop", slots=name, copy_stream="own" if args.own_copy_streams else "shared", rep=rep, batch=Bf, H0=H0, W0=W0, canvas=[H, W], dtype=args.dtype,
                 frames_per_s=round(loop(f, args.feeder_steps), 1))


if __name__ == "__main__":
    main()
