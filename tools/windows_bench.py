"""Cost of predicting on a window of each frame (vti_predict_windows), device events after warm-up, the three cases interleaved in
groups of `--group` calls, two repeats, both reported:
    python3 tools/windows_bench.py [--dtype h2] [--iters 40] [--group 5] [--B 64] [--imgsz 960] [--margin 32] [--stages]
64 frames of 1280x960 with the reference's settings (conf 0.20, iou 0.25, max_det 200, imgsz 960), window = the default ROI
(10, 300)..(1270, 760) grown by 32 px and clipped to the frame.
  windows      vti_predict_windows on the frames, at the canvas LetterBox gives the window (results in frame px);
  full frame   vti_predict_frames_native on the whole frames at the same imgsz (what a caller without the window form runs);
  work-around  a strided device copy of the window to contiguous crops, vti_predict_frames_native on them, then the shift of the
               boxes and the paste of the bit masks into frame-resolution rows with torch.
Before anything is timed the one-call form is compared with the work-around byte for byte.  Prints the ratio to the full-frame
predict next to the ratio of canvas pixels; --stages times letterbox / scored forward / NMS / scale boxes / masks of the windows
form and of the full-frame form one by one (where a saving falls short of the pixel ratio, the stage that holds it shows here)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

import vti_amd

H0, W0 = 960, 1280
ROI = (10, 300, 1270, 760)


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


def interleaved(title, cases, iters, group):
    """Two repeats; in each the cases alternate in groups of `group` calls.  -> {case: [mean ms of repeat 0, of repeat 1]}"""
    for fn in cases.values():
        timed(fn, 2, warmup=2)
    means = {k: [] for k in cases}
    for rep in range(2):
        acc = {k: [] for k in cases}
        for _ in range(max(iters // group, 1)):
            for k, fn in cases.items():
                acc[k].append(timed(fn, group))
        for k in cases:
            means[k].append(float(np.mean(acc[k])))
            print(f"  {title} repeat {rep}  {k:34s} {np.mean(acc[k]):9.3f} ms/call  (min group {min(acc[k]):.3f}, max {max(acc[k]):.3f})")
    return means


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="h2")
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--group", type=int, default=5)
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--imgsz", type=int, default=960)
    ap.add_argument("--margin", type=int, default=32)
    ap.add_argument("--stages", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("windows_bench needs the GPU")
    B, max_det, conf, iou = a.B, 200, 0.20, 0.25
    x0, y0 = max(0, ROI[0] - a.margin), max(0, ROI[1] - a.margin)
    x1, y1 = min(W0, ROI[2] + 1 + a.margin), min(H0, ROI[3] + 1 + a.margin)
    win = (x0, y0, x1 - x0, y1 - y0)
    w, h = win[2], win[3]
    Hw, Ww = vti_amd.letterbox_shape(h, w, a.imgsz)           # the canvas of the window ...
    Hf, Wf = vti_amd.letterbox_shape(H0, W0, a.imgsz)         # ... and of the whole frame
    print(f"B={B}, {a.dtype}, frames {W0}x{H0}, window (x0, y0, w, h) = {win}; canvas {Ww}x{Hw} for the window, {Wf}x{Hf} for the frame: "
          f"pixel ratio {Ww * Hw / (Wf * Hf):.3f}")
    ew = vti_amd.Engine("n", 2, H=Hw, W=Ww, max_batch=B, dtype=a.dtype)
    blob = vti_amd.random_weights(ew, seed=3, cls_bias=-1.0)
    ew.load_weights(blob, 0)
    ef = vti_amd.Engine("n", 2, H=Hf, W=Wf, max_batch=B, dtype=a.dtype)
    ef.load_weights(blob, 0)
    frames = torch.from_numpy(np.random.Generator(np.random.PCG64(0)).integers(0, 256, (B, H0, W0, 3), dtype=np.uint8)).cuda()
    buf = frames.reshape(-1)                                  # 3 * 960 * 1280 is a multiple of 16: the batch is its own frame buffer
    kw = dict(conf=conf, iou=iou, max_det=max_det)

    wt = ew.pack_windows([(H0, W0)] * B, [win] * B, "cuda")
    assert wt.total_bytes == buf.numel()
    ow = ew.alloc_outputs(B, max_det, 0, native_frames=wt.frames)
    ft, _, _ = ef.pack_frames([(H0, W0)] * B, "cuda")
    of = ef.alloc_outputs(B, max_det, 0, native_frames=ft)
    ct, _, _ = ew.pack_frames([(h, w)] * B, "cuda")
    oc = ew.alloc_outputs(B, max_det, 0, native_frames=ct)
    crops = torch.empty(ct.total_bytes, dtype=torch.uint8, device="cuda")
    assert ct.byte_offsets == [b * 3 * h * w for b in range(B)] or (3 * h * w) % 16
    crop_views = [crops[off:off + 3 * h * w].view(h, w, 3) for off in ct.byte_offsets]
    dense = (3 * h * w) % 16 == 0
    rb_c, rb_f = 8 * -(-w // 64), 8 * -(-W0 // 64)
    pasted = torch.zeros(ow["masks"].numel(), dtype=torch.uint8, device="cuda")
    shifted = torch.empty_like(oc["xyxy"])
    origin = torch.tensor([x0, y0, x0, y0], dtype=torch.float32, device="cuda")
    bit = torch.arange(8, device="cuda", dtype=torch.uint8)
    weights = (1 << torch.arange(8, device="cuda", dtype=torch.int32))

    def windows():
        ew.predict_windows_into(buf, wt, ow, **kw)

    def full_frame():
        ef.predict_frames_into(buf, ft, of, native=True, **kw)

    def workaround():
        # 1. the strided copy to contiguous crops
        if dense:
            crops.view(B, h, w, 3).copy_(frames[:, y0:y0 + h, x0:x0 + w])
        else:
            for b in range(B):
                crop_views[b].copy_(frames[b, y0:y0 + h, x0:x0 + w])
        # 2. today's call on them
        ew.predict_frames_into(crops, ct, oc, native=True, **kw)
        # 3. shift the boxes (rows past the counts stay zero) and paste the bit masks of the live slots into frame-resolution rows.
        #    Frames of one size: the live slots are the first offsets[B] slots of either ragged buffer (one read of that number).
        live = torch.arange(max_det, device="cuda")[None, :] < oc["counts"][:, None]
        torch.add(oc["xyxy"], origin, out=shifted)
        shifted.mul_(live[..., None])
        n = int(oc["offsets"][-1])
        dst = pasted[:n * H0 * rb_f].view(n, H0, rb_f)
        dst.zero_()
        slots = oc["masks"][:n * h * rb_c].view(n, h, rb_c)
        if x0 % 8 == 0:                                           # byte-aligned origin: whole bytes move (the crop's pad bits are 0)
            nb = -(-w // 8)
            dst[:, y0:y0 + h, x0 // 8:x0 // 8 + nb] = slots[..., :nb]
        else:                                                     # any origin: through one byte per pixel
            px = ((slots.unsqueeze(-1) >> bit) & 1).view(n, h, rb_c * 8)[..., :w]
            rows = torch.zeros((n, h, rb_f * 8), dtype=torch.uint8, device="cuda")
            rows[..., x0:x0 + w] = px
            dst[:, y0:y0 + h] = (rows.view(n, h, rb_f, 8).to(torch.int32) * weights).sum(-1).to(torch.uint8)

    # ---- the two routes give the same bytes
    windows()
    workaround()
    torch.cuda.synchronize()
    cnt = ow["counts"].cpu().tolist()
    assert torch.equal(ow["counts"], oc["counts"]) and torch.equal(ow["dets"], oc["dets"]) and torch.equal(ow["input"], oc["input"])
    assert torch.equal(ow["xyxy"], shifted)
    slot_f = H0 * rb_f
    n_inst = sum(cnt)
    assert int(ow["mask_bases"][-1]) == n_inst * slot_f and torch.equal(ow["masks"][:n_inst * slot_f], pasted[:n_inst * slot_f])
    nonempty = int(ow["masks"][:n_inst * slot_f].view(n_inst, -1).amax(1).count_nonzero()) if n_inst else 0
    print(f"{n_inst} instances ({n_inst / B:.1f} per frame), {nonempty} with a non-empty mask: windows == work-around, byte for byte")

    m = interleaved("predict", {"windows (vti_predict_windows)": windows, "full frame (predict_frames_native)": full_frame,
                                "work-around (copy, predict, paste)": workaround}, a.iters, a.group)
    for rep in range(2):
        wv, fv, kv = (m[k][rep] for k in m)
        print(f"  repeat {rep}: windows / full frame = {wv / fv:.3f} (canvas pixels {Ww * Hw / (Wf * Hf):.3f}); "
              f"windows / work-around = {wv / kv:.3f}")
    spread = max(abs(m[k][0] - m[k][1]) / min(m[k]) for k in m)
    print(f"  spread of the two repeats: up to {100 * spread:.1f} %")

    if a.stages:
        for title, eng, o, tab, form in (("windows", ew, ow, wt, "w"), ("full frame", ef, of, ft, "f")):
            best = eng.alloc_best(B, "cuda")
            stages = {
                "letterbox": (lambda: eng.letterbox_windows(buf, tab, out=o["input"])) if form == "w" else
                             (lambda: eng.letterbox_frames(buf, tab, out=o["input"])),
                "forward": lambda: eng.forward(o["input"], True, pred=o["pred"], proto=o["proto"], best=best),
                "nms": lambda: eng.nms(o["pred"], conf, iou, max_det, dets=o["dets"], counts=o["counts"], best=best),
                "scale_boxes": (lambda: eng.scale_boxes_windows(o["dets"], o["counts"], tab, xyxy=o["xyxy"])) if form == "w" else
                               (lambda: eng.scale_boxes(o["dets"], o["counts"], xyxy=o["xyxy"], frames=tab)),
                "masks": (lambda: eng.masks_native_windows(o["dets"], o["counts"], o["proto"], tab, "logit", masks=o["masks"],
                                                           offsets=o["offsets"], mask_bases=o["mask_bases"])) if form == "w" else
                         (lambda: eng.masks_native_frames(o["dets"], o["counts"], o["xyxy"], o["proto"], tab, "logit", masks=o["masks"],
                                                          offsets=o["offsets"], mask_bases=o["mask_bases"])),
            }
            for k, fn in stages.items():
                print(f"  stage  {title:10s} {k:12s} {timed(fn, 10, warmup=2):9.3f} ms/call")


if __name__ == "__main__":
    main()
