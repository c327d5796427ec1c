"""vti_mask_polygons cost (Results.masks.xy on the device) on a B-frame output set at the reference call (1280x960 frames, imgsz
960, max_det 200): letterbox-size bit masks (vti_masks) and frame-size rows (vti_masks_native, retina_masks=True) of the SAME
detections (synth_pred -> NMS -> scale_boxes), timed with device events after warm-up; then the host restatement (polygons.py) on
one frame's masks for the speed-up.
    python3 tools/polygons_bench.py [--iters 20] [--B 64] [--n-inst 50] [--host-frames 1]
Prints per mask form and strategy: us per call (count + scan + write launches), us per instance, the vertex total, and the same
call through Engine.mask_polygons (with its one host read)."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

import vti_amd
from gpu_util import synth_pred
from vti_amd._lib import check
from vti_amd.engine import POLY_STRATEGIES
from vti_amd.polygons import masks2segments, scale_coords


def timed(fn, iters, warmup=3):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--n-inst", type=int, default=50)
    ap.add_argument("--host-frames", type=int, default=1)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("polygons_bench needs the GPU")
    B, H0, W0, max_det = a.B, 960, 1280, 200
    H, W = vti_amd.letterbox_shape(H0, W0, 960)
    eng = vti_amd.Engine("n", 2, H=H, W=W, max_batch=B, dtype="h2")
    eng.load_weights(vti_amd.random_weights(eng, seed=1), 0)
    cap = B * max_det
    rng = np.random.default_rng(0)
    pred = torch.from_numpy(synth_pred(rng, B, 2, 32, eng.num_anchors, H=H, W=W, n_inst=a.n_inst)).cuda()
    proto = torch.from_numpy(rng.standard_normal((B, H // 4, W // 4, 32)).astype(np.float32)).to(eng.torch_dtype).cuda()
    dets, counts = eng.nms(pred, 0.25, 0.7, max_det)
    xyxy = eng.scale_boxes(dets, counts, H0, W0)
    live = int(counts.sum())
    print(f"B={B} frames {W0}x{H0}, letterbox {W}x{H}; {live} instances ({live / B:.1f} per frame), capacity {cap}")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for native in (False, True):
        rb = eng.mask_native_layout(H0, W0)["row_bytes"] if native else W // 8
        mh, mw = (H0, W0) if native else (H, W)
        masks = torch.empty((cap, mh, rb), dtype=torch.uint8, device="cuda")
        off = torch.empty((B + 1,), dtype=torch.int32, device="cuda")
        if native:
            eng.masks_native(dets, counts, xyxy, proto, H0, W0, "logit", "bits", capacity=cap, masks=masks, offsets=off)
        else:
            eng.masks(dets, counts, proto, "logit", "bits", capacity=cap, masks=masks, offsets=off)
        masks = masks[:live]
        name = "retina (vti_masks_native rows)" if native else "letterbox (vti_masks bits)"
        print(f"  {name}: {mh}x{mw}, row_bytes {rb}, scratch {eng.mask_polygons_scratch_bytes(mh, mw, rb) / 2 ** 20:.0f} MiB")
        for strategy in ("largest", "concat"):
            pts, po = eng.mask_polygons(masks, mw, H0, W0, strategy)         # sizes the kept points buffer
            total = int(po[-1])
            ws, buf, po2 = eng._poly_ws, eng._poly_points, torch.empty_like(po)

            def call():
                check(eng._ctx, vti_amd.lib().vti_mask_polygons(
                    eng._ctx, C.c_void_p(masks.data_ptr()), live, None, mh, mw, rb, H0, W0, POLY_STRATEGIES[strategy],
                    C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(po2.data_ptr()), C.c_void_p(buf.data_ptr()), buf.shape[0], st))
            ms = timed(call, a.iters)
            ms_eng = timed(lambda: eng.mask_polygons(masks, mw, H0, W0, strategy), a.iters)
            print(f"    {strategy:8s} {ms * 1e3:9.1f} us/call  {ms * 1e3 / max(live, 1):7.2f} us/instance  {total:8d} vertices"
                  f"   Engine.mask_polygons {ms_eng * 1e3:9.1f} us")
        if a.host_frames > 0:                                                  # the host restatement on the first frames' masks
            n_host = int(counts[:a.host_frames].sum())
            m = vti_amd.unpack_bits(masks[:n_host], mw).cpu().numpy()
            t0 = time.perf_counter()
            [scale_coords((mh, mw), s, (H0, W0)) for s in masks2segments(m)]
            dt = time.perf_counter() - t0
            dev = timed(lambda: eng.mask_polygons(masks[:n_host], mw, H0, W0), 3, warmup=1)
            print(f"    host polygons.py on {a.host_frames} frame(s), {n_host} instances: {dt * 1e3:.0f} ms "
                  f"({dt * 1e3 / max(n_host, 1):.1f} ms/instance) vs {dev * 1e3:.0f} us on the device for the same masks: "
                  f"{dt / max(dev * 1e-3, 1e-9):.0f}x")


if __name__ == "__main__":
    main()
