"""vti_measure cost: process_frame's measurement record for a batch, from letterbox-size bit masks (vti_masks) and from
frame-size ones (vti_masks_native), on the SAME detections (synth_pred -> NMS -> scale_boxes), timed with device events after
warm-up, next to the predict step it follows.
    python3 tools/measure_bench.py [--dtype h2] [--iters 50] [--B 64] [--n-inst 50] [--cameras N [N ...]] [--groups G]
                                   [--frames-table [--parent-lib PATH]]
Prints per mask form: us per call (the three launches), us per frame, and its share of one predict_into step (letterbox ->
net -> NMS -> masks -> scale_boxes) at the same batch.
--cameras N: also vti_measure_cameras with a table of N cameras assigned round-robin (frame b -> camera b % N; the two calibration
files of tests/golden alternate, every row at a camera position of its own, ROI and thresholds shared so that the work is the
one-camera call's), table and index uploaded before the timing.
--groups G: also the work-around the table form replaces, G vti_measure calls on views of the same output set, one per contiguous
group of B / G frames (offsets rebased per group beforehand; a real caller would also have to sort its frames by camera).
--frames-table: also vti_measure_frames with a frame table of B equal frames (the same work as vti_measure_cameras with one camera,
letterbox masks) next to vti_measure_cameras, the two interleaved in groups of 10 calls, two runs; --parent-lib PATH (a libvti.so
built from the parent commit) adds that build's vti_measure_cameras on the same buffers to the interleave."""
import ctypes as C
import argparse
import dataclasses
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

import vti_amd
from gpu_util import frames_u8, synth_pred


def timed(fn, iters, warmup=5):
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


def frames_table_case(a, eng, o, res, params, B, H0, W0, cap, max_det):
    from vti_amd import _lib
    cams = eng.pack_cameras([params], "cuda")
    idx = torch.zeros(B, dtype=torch.int32, device="cuda")
    ft, _, _ = eng.pack_frames([(H0, W0)] * B, "cuda")
    cases = {"vti_measure_cameras": lambda: eng.measure(o, cams, H0, W0, result=res, cameras=idx),
             "vti_measure_frames ": lambda: eng.measure(o, cams, result=res, cameras=idx, frames=ft)}
    eng.measure(o, cams, H0, W0, result=res, cameras=idx)
    want = {k: res[k].clone() for k in ("frame_f64", "frame_i32", "stitch_f64", "stitch_i32")}
    eng.measure(o, cams, result=res, cameras=idx, frames=ft)
    torch.cuda.synchronize()
    for k, v in want.items():                 # NaN-safe: compare the bytes
        assert torch.equal(v.view(torch.uint8), res[k].view(torch.uint8)), k
    if a.parent_lib:
        L = C.CDLL(a.parent_lib)
        P, I = C.c_void_p, C.c_int32
        L.vti_create.restype, L.vti_create.argtypes = I, [C.POINTER(_lib.VtiDesc), C.POINTER(P)]
        L.vti_measure_pack_cameras.restype, L.vti_measure_pack_cameras.argtypes = I, [P, C.POINTER(_lib.VtiMeasureParams), I, P, C.c_size_t]
        L.vti_measure_cameras.restype, L.vti_measure_cameras.argtypes = _lib.SIGNATURES["vti_measure_cameras"]
        ctx = P(0)
        desc = _lib.VtiDesc(b"n", 2, 32, 16, eng.H, eng.W, B, _lib.VTI_H2)
        assert L.vti_create(C.byref(desc), C.byref(ctx)) == 0
        host = torch.zeros(cams.numel(), dtype=torch.uint8)
        assert L.vti_measure_pack_cameras(ctx, C.byref(params.to_c()), 1, P(host.data_ptr()), host.numel()) == 0
        pcams = host.cuda()
        ws = torch.empty(eng.measure_scratch_bytes(B, cap, W0), dtype=torch.uint8, device="cuda")
        pres = {k: torch.empty_like(v) for k, v in want.items()}
        ptr = lambda t: P(t.data_ptr())

        def parent():
            rc = L.vti_measure_cameras(ctx, ptr(pcams), 1, ptr(idx), ptr(o["masks"]), 0, ptr(o["dets"]), ptr(o["xyxy"]), ptr(o["counts"]),
                                       ptr(o["offsets"]), B, max_det, cap, H0, W0, ptr(ws), ws.numel(), ptr(pres["frame_f64"]),
                                       ptr(pres["frame_i32"]), ptr(pres["stitch_f64"]), ptr(pres["stitch_i32"]),
                                       P(torch.cuda.current_stream().cuda_stream))
            assert rc == 0, rc
        parent()
        torch.cuda.synchronize()
        for k, v in want.items():
            assert torch.equal(v.view(torch.uint8), pres[k].view(torch.uint8)), k
        cases = dict({"vti_measure_cameras (parent build)": parent}, **cases)
    for fn in cases.values():
        timed(fn, 5, warmup=2)
    for run in range(2):
        acc = {k: [] for k in cases}
        for _ in range(max(a.iters // 10, 1)):
            for k, fn in cases.items():
                acc[k].append(timed(fn, 10, warmup=0) * 1e3)
        for k in cases:
            print(f"    frames-table run {run}  {k:36s} {np.mean(acc[k]):8.1f} us/call  (min group {min(acc[k]):.1f}, max {max(acc[k]):.1f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="h2")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--n-inst", type=int, default=50)
    ap.add_argument("--cameras", type=int, nargs="+", default=[])
    ap.add_argument("--groups", type=int, default=0)
    ap.add_argument("--frames-table", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("measure_bench needs the GPU")
    B, H0, W0, max_det = a.B, 960, 1280, 200
    H, W = vti_amd.letterbox_shape(H0, W0, 960)
    eng = vti_amd.Engine("n", 2, H=H, W=W, max_batch=B, dtype=a.dtype)
    eng.load_weights(vti_amd.random_weights(eng, seed=1), 0)
    cap = B * max_det
    # the predict step this stage follows (reference call: conf 0.20, iou 0.25, max_det 200, imgsz 960)
    frames = torch.from_numpy(frames_u8(B, H0, W0, 0)).cuda()
    out = eng.alloc_outputs(B, max_det, cap, "bits", frames.device)
    ms_pred = timed(lambda: eng.predict_into(frames, out, 0.20, 0.25, max_det), a.iters)
    # realistic instance counts: planted detections of both classes with random-blob masks
    rng = np.random.default_rng(0)
    pred = torch.from_numpy(synth_pred(rng, B, 2, 32, eng.num_anchors, H=H, W=W, n_inst=a.n_inst)).cuda()
    proto = torch.from_numpy(rng.standard_normal((B, H // 4, W // 4, 32)).astype(np.float32)).to(eng.torch_dtype).cuda()
    dets, counts = eng.nms(pred, 0.25, 0.7, max_det)
    xyxy = eng.scale_boxes(dets, counts, H0, W0)
    golden = os.path.join(ROOT, "tests", "golden")
    params = vti_amd.MeasureParams.from_files(os.path.join(golden, "camera_calibration.json"), os.path.join(golden, "extrinsics.json"))
    other = vti_amd.MeasureParams.from_files(os.path.join(golden, "camera_calibration.json"), os.path.join(golden, "camera_extrinsics.json"))
    tables = {}
    for n in a.cameras:     # camera 0 = `params`; every row differs (calibration file, camera position) but keeps the ROI and the
        # thresholds, so the same instances are measured as in the one-camera call and the times compare
        cams = [dataclasses.replace(p, t=p.t + 1e-4 * c) for c, p in ((c, other if c & 1 else params) for c in range(n))]
        tables[n] = (eng.pack_cameras(cams, "cuda"), (torch.arange(B, dtype=torch.int32) % n).to(torch.int32).cuda())
    live = int(counts.sum())
    print(f"B={B} frames {W0}x{H0}, letterbox {W}x{H}, {a.dtype}; predict_into step {ms_pred * 1e3:.0f} us; "
          f"measure on {live} instances ({live / B:.1f} per frame), capacity {cap}")
    for native in (False, True):
        rb = eng.mask_native_layout(H0, W0)["row_bytes"] if native else W // 8
        masks = torch.empty((cap, H0 if native else H, rb), dtype=torch.uint8, device="cuda")
        off = torch.empty((B + 1,), dtype=torch.int32, device="cuda")
        if native:
            eng.masks_native(dets, counts, xyxy, proto, H0, W0, "logit", "bits", capacity=cap, masks=masks, offsets=off)
        else:
            eng.masks(dets, counts, proto, "logit", "bits", capacity=cap, masks=masks, offsets=off)
        o = dict(dets=dets, xyxy=xyxy, counts=counts, offsets=off, masks=masks)
        res = eng.measure(o, params, H0, W0, native=native)
        st = res["frame_i32"][:, 0].cpu().numpy()
        ms = timed(lambda: eng.measure(o, params, H0, W0, native=native, result=res), a.iters)
        ms_lean = timed(lambda: eng.measure(o, params, H0, W0, native=native, stitch_rows=False, result=res), a.iters)
        name = "native (vti_masks_native rows)" if native else "letterbox (vti_masks bits)"
        print(f"  {name:31s} {ms * 1e3:8.1f} us/call  {ms * 1e3 / B:6.2f} us/frame  {100 * ms / ms_pred:5.2f} % of the step"
              f"  (records only: {ms_lean * 1e3:.1f} us)  status 0 in {int((st == 0).sum())}/{B} frames")
        for n, (table, idx) in tables.items():
            ms = timed(lambda: eng.measure(o, table, H0, W0, native=native, result=res, cameras=idx), a.iters)
            st = res["frame_i32"][:, 0].cpu().numpy()
            print(f"    vti_measure_cameras, {n:3d} cameras    {ms * 1e3:8.1f} us/call  {ms * 1e3 / B:6.2f} us/frame"
                  f"  status 0 in {int((st == 0).sum())}/{B} frames")
        if a.frames_table and not native:
            frames_table_case(a, eng, o, res, params, B, H0, W0, cap, max_det)
        if a.groups:
            G, per = a.groups, B // a.groups
            oh = off.cpu()
            views = []
            for g in range(G):
                b0, b1 = g * per, (g + 1) * per
                s0, s1 = int(oh[b0]), int(oh[b1])
                og = dict(dets=dets[b0:b1], xyxy=xyxy[b0:b1], counts=counts[b0:b1], offsets=(off[b0:b1 + 1] - s0).contiguous(),
                          masks=masks[s0:s1])
                rg = dict(frame_f64=res["frame_f64"][b0:b1], frame_i32=res["frame_i32"][b0:b1], stitch_f64=res["stitch_f64"][s0:s1],
                          stitch_i32=res["stitch_i32"][s0:s1])
                views.append((og, rg))
            ms = timed(lambda: [eng.measure(og, params, H0, W0, native=native, result=rg) for og, rg in views], a.iters)
            print(f"    work-around: {G} vti_measure calls    {ms * 1e3:8.1f} us/all   {ms * 1e3 / B:6.2f} us/frame")


if __name__ == "__main__":
    main()
