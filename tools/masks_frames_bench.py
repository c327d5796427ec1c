"""Cost of the ragged frame-resolution masks (vti_masks_native_frames, vti_measure_frames_native), device events after warm-up, the
cases of a comparison interleaved in groups of 10 calls, two runs each:
    python3 tools/masks_frames_bench.py [--dtype h2] [--iters 50] [--B 64] [--n-inst 50] [--parent-lib PATH [--parent-last]]
  (a) the uniform vti_masks_native, B frames of 1280x960: this build (and with --parent-lib, a libvti.so built from the parent commit,
      on the same buffers) -- the uniform instantiation of the tile kernel is meant to be the same code;
  (b) vti_masks_native_frames on B frames cycling four sizes, against the work-around it replaces: four uniform calls, one per size,
      on the frames regrouped by size beforehand (the regrouping itself is not timed);
  (c) vti_measure_frames_native on B equal frames, against vti_measure_cameras(native = 1) of this build and of the parent's.
--parent-last: the parent's case runs last in every group instead of first (is a difference the build's or the order's?)."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

import vti_amd
from vti_amd import _lib
from gpu_util import synth_pred

SIZES = [(960, 1280), (720, 960), (1080, 1920), (481, 333)]


def timed(fn, iters, warmup=0):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def interleaved(title, cases, iters):
    for fn in cases.values():
        timed(fn, 5, warmup=2)
    for run in range(2):
        acc = {k: [] for k in cases}
        for _ in range(max(iters // 10, 1)):
            for k, fn in cases.items():
                acc[k].append(timed(fn, 10) * 1e3)
        for k in cases:
            print(f"  {title} run {run}  {k:44s} {np.mean(acc[k]):9.1f} us/call  (min group {min(acc[k]):.1f}, max {max(acc[k]):.1f})")


def parent_ctx(path, eng, blob):
    """A context of the parent build with the same plan, weights and a workspace of its own."""
    L = C.CDLL(path)
    P, I = C.c_void_p, C.c_int32
    for name in ("vti_create", "vti_load_weights", "vti_set_workspace", "vti_workspace_bytes", "vti_masks_native", "vti_measure_cameras",
                 "vti_measure_pack_cameras"):
        getattr(L, name).restype, getattr(L, name).argtypes = _lib.SIGNATURES[name]
    ctx = P(0)
    desc = _lib.VtiDesc(b"n", eng.nc, eng.nm, eng.reg_max, eng.H, eng.W, eng.max_batch, vti_amd.engine.DTYPES[eng.dtype])
    assert L.vti_create(C.byref(desc), C.byref(ctx)) == 0
    buf = (C.c_char * len(blob)).from_buffer_copy(blob)
    assert L.vti_load_weights(ctx, buf, len(blob), 0) == 0
    n = int(L.vti_workspace_bytes(ctx))
    ws = torch.empty(n + 256, dtype=torch.uint8, device="cuda")
    assert L.vti_set_workspace(ctx, P((ws.data_ptr() + 255) & ~255), n) == 0
    return L, ctx, ws


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="h2")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--n-inst", type=int, default=50)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-last", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("masks_frames_bench needs the GPU")
    B, H0, W0, max_det = a.B, 960, 1280, 200
    H, W = vti_amd.letterbox_shape(H0, W0, 960)
    eng = vti_amd.Engine("n", 2, H=H, W=W, max_batch=B, dtype=a.dtype)
    blob = vti_amd.random_weights(eng, seed=1)
    eng.load_weights(blob, 0)
    P = C.c_void_p
    ptr = lambda t: P(t.data_ptr())
    stream = lambda: P(torch.cuda.current_stream().cuda_stream)
    par = parent_ctx(a.parent_lib, eng, blob) if a.parent_lib else None
    rng = np.random.default_rng(0)
    pred = torch.from_numpy(synth_pred(rng, B, 2, 32, eng.num_anchors, H=H, W=W, n_inst=a.n_inst)).cuda()
    proto = torch.from_numpy(rng.standard_normal((B, H // 4, W // 4, 32)).astype(np.float32)).to(eng.torch_dtype).cuda()
    dets, counts = eng.nms(pred, 0.25, 0.7, max_det)
    live = int(counts.sum())
    print(f"B={B}, canvas {W}x{H}, {a.dtype}, {live} instances ({live / B:.1f} per frame)")

    # (a) the uniform call, parent against this build
    xyxy = eng.scale_boxes(dets, counts, H0, W0)
    masks, off = eng.masks_native(dets, counts, xyxy, proto, H0, W0, "logit", "bits", capacity=live)
    cases = {"vti_masks_native (this build)": lambda: eng.masks_native(dets, counts, xyxy, proto, H0, W0, "logit", "bits", capacity=live,
                                                                       masks=masks, offsets=off)}
    if par:
        L, ctx, _ = par
        pm, po = torch.empty_like(masks), torch.empty_like(off)

        def parent_masks():
            rc = L.vti_masks_native(ctx, ptr(dets), ptr(xyxy), ptr(counts), ptr(proto), B, max_det, H0, W0, 0, 1, ptr(pm), live, ptr(po), stream())
            assert rc == 0, rc
        parent_masks()
        torch.cuda.synchronize()
        assert torch.equal(pm, masks) and torch.equal(po, off)
        first = {"vti_masks_native (parent build)": parent_masks}
        cases = dict(cases, **first) if a.parent_last else dict(first, **cases)
    interleaved(f"(a) uniform {W0}x{H0}", cases, a.iters)

    # (b) the ragged call against one uniform call per size on the regrouped frames
    shapes = [SIZES[b % 4] for b in range(B)]
    table, _, _ = eng.pack_frames(shapes, "cuda")
    rxy = eng.scale_boxes(dets, counts, frames=table)
    rmasks, roff, rbases = eng.masks_native_frames(dets, counts, rxy, proto, table, "logit")
    groups = []
    for g, (h, w) in enumerate(SIZES):
        sel = torch.arange(g, B, 4, device="cuda")
        gd, gc, gx, gp = dets[sel].contiguous(), counts[sel].contiguous(), rxy[sel].contiguous(), proto[sel].contiguous()
        n = int(gc.sum())
        gm, go = eng.masks_native(gd, gc, gx, gp, h, w, "logit", "bits", capacity=n)
        groups.append((gd, gc, gx, gp, h, w, n, gm, go))
    torch.cuda.synchronize()
    bases, cnt = rbases.cpu().tolist(), counts.cpu().tolist()
    for g, (gd, gc, gx, gp, h, w, n, gm, go) in enumerate(groups):       # the two routes write the same slots
        goh = go.cpu().tolist()
        for j, b in enumerate(range(g, B, 4)):
            assert torch.equal(eng.frame_masks(rmasks, table, b, bases[b], cnt[b]), gm[goh[j]:goh[j + 1]]), b

    def workaround():
        for gd, gc, gx, gp, h, w, n, gm, go in groups:
            eng.masks_native(gd, gc, gx, gp, h, w, "logit", "bits", capacity=n, masks=gm, offsets=go)
    interleaved("(b) four sizes", {
        "vti_masks_native_frames": lambda: eng.masks_native_frames(dets, counts, rxy, proto, table, "logit", masks=rmasks, offsets=roff,
                                                                   mask_bases=rbases),
        "work-around: 4 vti_masks_native calls": workaround}, a.iters)
    print(f"      ({rmasks.numel() / 1e6:.0f} MB of masks; sizes {SIZES})")

    # (c) the measurement on B equal frames
    golden = os.path.join(ROOT, "tests", "golden")
    params = vti_amd.MeasureParams.from_files(os.path.join(golden, "camera_calibration.json"), os.path.join(golden, "extrinsics.json"))
    cams = eng.pack_cameras([params], "cuda")
    idx = torch.zeros(B, dtype=torch.int32, device="cuda")
    eq, _, _ = eng.pack_frames([(H0, W0)] * B, "cuda")
    rows = B * max_det
    res = dict(frame_f64=torch.empty((B, 2), dtype=torch.float64, device="cuda"), frame_i32=torch.empty((B, 6), dtype=torch.int32, device="cuda"),
               stitch_f64=torch.empty((rows, 7), dtype=torch.float64, device="cuda"), stitch_i32=torch.empty((rows, 2), dtype=torch.int32, device="cuda"))
    big = torch.empty((rows,) + tuple(masks.shape[1:]), dtype=torch.uint8, device="cuda")          # capacity = B * max_det rows in both forms
    big[:live] = masks
    o_uni = dict(dets=dets, xyxy=xyxy, counts=counts, offsets=off, masks=big)
    em, eo, eb = eng.masks_native_frames(dets, counts, xyxy, proto, eq, "logit")
    assert torch.equal(em, masks.reshape(-1))
    o_rag = dict(dets=dets, xyxy=xyxy, counts=counts, offsets=eo, masks=em, mask_bases=eb, native_shapes=tuple(eq.shapes))
    eng.measure(o_uni, cams, H0, W0, native=True, result=res, cameras=idx)
    want = {k: v.clone() for k, v in res.items()}
    eng.measure(o_rag, cams, native=True, result=res, cameras=idx, frames=eq)
    torch.cuda.synchronize()
    for k, v in want.items():
        n = live if k.startswith("stitch") else B
        assert torch.equal(v[:n].view(torch.uint8), res[k][:n].view(torch.uint8)), k
    cases = {"vti_measure_cameras(native=1) (this build)": lambda: eng.measure(o_uni, cams, H0, W0, native=True, result=res, cameras=idx),
             "vti_measure_frames_native": lambda: eng.measure(o_rag, cams, native=True, result=res, cameras=idx, frames=eq)}
    if par:
        L, ctx, _ = par
        host = torch.zeros(cams.numel(), dtype=torch.uint8)
        assert L.vti_measure_pack_cameras(ctx, C.byref(params.to_c()), 1, P(host.data_ptr()), host.numel()) == 0
        pcams = host.cuda()
        ws = torch.empty(eng.measure_scratch_bytes(B, rows, W0), dtype=torch.uint8, device="cuda")
        pres = {k: torch.empty_like(v) for k, v in want.items()}

        def parent_measure():
            rc = L.vti_measure_cameras(ctx, ptr(pcams), 1, ptr(idx), ptr(big), 1, ptr(dets), ptr(xyxy), ptr(counts), ptr(off), B, max_det,
                                       rows, H0, W0, ptr(ws), ws.numel(), ptr(pres["frame_f64"]), ptr(pres["frame_i32"]),
                                       ptr(pres["stitch_f64"]), ptr(pres["stitch_i32"]), stream())
            assert rc == 0, rc
        parent_measure()
        torch.cuda.synchronize()
        for k, v in want.items():
            n = live if k.startswith("stitch") else B
            assert torch.equal(v[:n].view(torch.uint8), pres[k][:n].view(torch.uint8)), k
        first = {"vti_measure_cameras(native=1) (parent build)": parent_measure}
        cases = dict(cases, **first) if a.parent_last else dict(first, **cases)
    interleaved(f"(c) measure, {B} equal frames", cases, a.iters)


if __name__ == "__main__":
    main()
