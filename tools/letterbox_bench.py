"""Letterbox cost on a resizing batch: vti_letterbox against vti_letterbox_frames, timed with device events after warm-up, the
cases interleaved call-group by call-group inside one run, two runs.
    python3 tools/letterbox_bench.py [--iters 50] [--B 64] [--runs 2] [--parent-lib PATH]
B frames of 1280x960 at imgsz=960:
  (a)  vti_letterbox, canvas 736x960 (the rect letterbox of the reference's frame); with --parent-lib PATH (a libvti.so built from
       the parent commit) also the parent's vti_letterbox on the same buffers, as (a-parent)
  (b)  vti_letterbox_frames on the same B equal frames packed for the SAME 736x960 canvas: the same bytes in and out as (a)
  (c)  vti_letterbox_frames on B frames cycling through eight sizes (every resize branch) at the 960x960 canvas
Prints us per call and bytes moved (source bytes of the frames + canvas bytes written) over the kernel time against the 8 TB/s
HBM peak (6.3 TB/s achievable)."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

import vti_amd
from vti_amd import _lib

SIZES = [(960, 1280), (640, 640), (480, 640), (1080, 1920), (1920, 1920), (960, 960), (481, 333), (1200, 1600)]


def events(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters * 1e3        # us per call


def parent_letterbox(path, H, W, B):
    """vti_letterbox of another build of the library (no weights needed: the stage only reads the ctx's canvas)."""
    L = C.CDLL(path)
    L.vti_create.restype, L.vti_create.argtypes = C.c_int32, [C.POINTER(_lib.VtiDesc), C.POINTER(C.c_void_p)]
    L.vti_letterbox.restype, L.vti_letterbox.argtypes = C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    ctx = C.c_void_p(0)
    desc = _lib.VtiDesc(b"n", 2, 32, 16, H, W, B, _lib.VTI_H2)
    assert L.vti_create(C.byref(desc), C.byref(ctx)) == 0

    def call(frames, out):
        B_, H0, W0, _ = frames.shape
        rc = L.vti_letterbox(ctx, C.c_void_p(frames.data_ptr()), B_, H0, W0, C.c_void_p(out.data_ptr()),
                             C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("letterbox_bench needs the GPU")
    B, H0, W0 = a.B, 960, 1280
    H, W = vti_amd.letterbox_shape(H0, W0, 960)
    rect = vti_amd.Engine("n", 2, H=H, W=W, max_batch=B, dtype="h2")
    square = vti_amd.Engine("n", 2, H=960, W=960, max_batch=B, dtype="h2")
    rng = np.random.Generator(np.random.PCG64(0))
    frames = torch.from_numpy(rng.integers(0, 256, (B, H0, W0, 3), dtype=np.uint8)).cuda()
    out_a = torch.empty((B, H, W, 3), dtype=torch.uint8, device="cuda")
    out_b = torch.empty_like(out_a)
    out_c = torch.empty((B, 960, 960, 3), dtype=torch.uint8, device="cuda")
    table_b, _, _ = rect.pack_frames([(H0, W0)] * B, "cuda")
    assert table_b.total_bytes == frames.numel()                 # the same buffer serves (a) and (b)
    flat = frames.view(-1)
    shapes = [SIZES[b % 8] for b in range(B)]
    table_c, _, total_c = square.pack_frames(shapes, "cuda")
    buf_c = torch.from_numpy(rng.integers(0, 256, total_c, dtype=np.uint8)).cuda()
    cases = {"(a) vti_letterbox 736x960": (lambda: rect.letterbox(frames, out=out_a), frames.numel() + out_a.numel()),
             "(b) vti_letterbox_frames, equal frames, 736x960": (lambda: rect.letterbox_frames(flat, table_b, out=out_b),
                                                               frames.numel() + out_b.numel()),
             "(c) vti_letterbox_frames, eight sizes, 960x960": (lambda: square.letterbox_frames(buf_c, table_c, out=out_c),
                                                              sum(3 * h * w for h, w in shapes) + out_c.numel())}
    if a.parent_lib:
        par = parent_letterbox(a.parent_lib, H, W, B)
        out_p = torch.empty_like(out_a)
        cases = dict({"(a-parent) vti_letterbox 736x960": (lambda: par(frames, out_p), frames.numel() + out_p.numel())}, **cases)
    for fn, _ in cases.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    assert torch.equal(out_a, out_b)
    if a.parent_lib:
        assert torch.equal(out_a, out_p)
    print(f"B={B} frames {W0}x{H0}; {a.iters} calls per case and run, cases interleaved in groups of 10 calls")
    for run in range(a.runs):
        acc = {k: [] for k in cases}
        for _ in range(max(a.iters // 10, 1)):
            for k, (fn, _) in cases.items():
                acc[k].append(events(fn, 10))
        for k, (_, nbytes) in cases.items():
            us = float(np.mean(acc[k]))
            print(f"  run {run}  {k:50s} {us:8.1f} us/call  (min group {min(acc[k]):.1f}, max {max(acc[k]):.1f})  "
                  f"{nbytes / 1e6:7.1f} MB  {nbytes / us / 1e6:5.2f} TB/s = {100 * nbytes / us / 1e6 / 8.0:4.1f} % of the 8 TB/s peak")


if __name__ == "__main__":
    main()
