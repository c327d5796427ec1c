"""retina_masks cost: vti_masks_native (frame-resolution masks) against vti_masks (letterbox-size masks) on the SAME detections
(synth_pred -> NMS -> scale_boxes), bit-packed, timed with device events after warm-up.
    python3 tools/retina_masks_bench.py [--dtype h2] [--iters 50] [--only native|letterbox]
Cases: the reference call (B=1, 1280x960 frame, imgsz 960, ~20 instances) and a batch (B=64 such frames, 50 instances each).
Prints per case and kernel: ms per call, output Mpx/s (instances x mask pixels), and the per-pixel cost of native over letterbox."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

import vti_amd
from gpu_util import synth_pred

CASES = [("reference call", 1, 960, 1280, 960, 20), ("batch", 64, 960, 1280, 960, 50)]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="h2")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--only", choices=["native", "letterbox"], default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("retina_masks_bench needs the GPU")
    for name, B, H0, W0, imgsz, n_inst in CASES:
        H, W = vti_amd.letterbox_shape(H0, W0, imgsz)
        eng = vti_amd.Engine("n", 2, H=H, W=W, max_batch=B, dtype=a.dtype)
        eng.load_weights(vti_amd.random_weights(eng, seed=1), 0)
        rng = np.random.default_rng(0)
        pred = torch.from_numpy(synth_pred(rng, B, 2, 32, eng.num_anchors, H=H, W=W, n_inst=n_inst)).cuda()
        proto = torch.from_numpy(rng.standard_normal((B, H // 4, W // 4, 32)).astype(np.float32)).to(eng.torch_dtype).cuda()
        dets, counts = eng.nms(pred, 0.25, 0.7, 300)
        xyxy = eng.scale_boxes(dets, counts, H0, W0)
        live = int(counts.sum())
        lb_masks, off = eng.masks(dets, counts, proto, "logit", "bits", capacity=live)
        nat_masks, off2 = eng.masks_native(dets, counts, xyxy, proto, H0, W0, "logit", "bits", capacity=live)
        res = {}
        if a.only != "native":
            ms = timed(lambda: eng.masks(dets, counts, proto, "logit", "bits", capacity=live, masks=lb_masks, offsets=off), a.iters)
            res["letterbox (vti_masks)"] = (ms, live * H * W)
        if a.only != "letterbox":
            ms = timed(lambda: eng.masks_native(dets, counts, xyxy, proto, H0, W0, "logit", "bits", capacity=live, masks=nat_masks,
                                                offsets=off2), a.iters)
            res["native (vti_masks_native)"] = (ms, live * H0 * W0)
        print(f"{name}: B={B} frame {W0}x{H0} imgsz {imgsz} ({W}x{H} letterbox), {live} instances, {a.dtype}")
        for k, (ms, px) in res.items():
            print(f"  {k:27s} {ms:8.3f} ms  {px / ms / 1e3:9.0f} Mpx/s  ({px / 1e6:.1f} Mpx)")
        if len(res) == 2:
            (ml, pl), (mn, pn) = res.values()
            print(f"  native / letterbox per output pixel: {(mn / pn) / (ml / pl):.2f}x")
        del eng


if __name__ == "__main__":
    main()
