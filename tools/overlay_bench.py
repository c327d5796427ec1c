"""vti_overlay cost: the model-check viewer's picture of a selection of one batch, from letterbox-size bit masks (vti_masks) and from
frame-size ones (vti_masks_native), on the SAME detections (synth_pred -> NMS -> scale_boxes), in each of the three modes, timed with
device events after warm-up, next to the floor measured in the same run: a device-to-device copy of the same n_sel frames, which is
what the call must at least do.
    python3 tools/overlay_bench.py [--dtype h2] [--B 8] [--n-inst 40] [--n-sel 8] [--rounds 5] [--max-points 16384] [--size 960 1280]
                                   [--mixed]
The two (overlay, copy) are interleaved in groups of 10 calls, `--rounds` groups each, and the whole measurement runs twice.
Prints per mask form, mode and n_sel: us per call, the copy's us, their ratio, us per selected frame, frames whose contours were skipped.
--mixed: the same frames, detections and masks also go through a frame table (vti_overlay_frames: Engine.overlay(table=); the native
rows then are the ragged buffer of vti_masks_native_frames), timed in the same groups; the pictures must equal the uniform call's."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

import vti_amd
from gpu_util import frames_u8, synth_pred


def group_ms(fn, calls=10):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="h2")
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--n-inst", type=int, default=40)
    ap.add_argument("--n-sel", type=int, nargs="+", default=[8])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-points", type=int, default=16384)
    ap.add_argument("--size", type=int, nargs=2, default=[960, 1280], metavar=("H0", "W0"))
    ap.add_argument("--mixed", action="store_true", help="also time the same batch through a frame table (vti_overlay_frames)")
    a = ap.parse_args()
    H, W, (h, w), B = 736, 960, a.size, a.B
    eng = vti_amd.Engine("n", 2, H=H, W=W, max_batch=B, dtype=a.dtype)
    eng.load_weights(vti_amd.random_weights(eng, 1), 0)
    rng = np.random.default_rng(5)
    pred = torch.from_numpy(synth_pred(rng, B, 2, 32, eng.num_anchors, H=H, W=W, n_inst=a.n_inst)).cuda()
    proto = torch.from_numpy(rng.standard_normal((B, H // 4, W // 4, 32)).astype(np.float32)).cuda()
    proto = vti_amd.h2_encode(proto) if eng.dtype == "h2" else proto.to(eng.torch_dtype)     # the engine's own storage type
    dets, counts = eng.nms(pred, 0.25, 0.7, 200)
    frames = torch.from_numpy(frames_u8(B, h, w, 0)).cuda()
    xyxy = eng.scale_boxes(dets, counts, h, w)
    cap = B * 200
    if a.mixed:
        table, offs, total = eng.pack_frames([(h, w)] * B, "cuda")
        flat = torch.zeros(total, dtype=torch.uint8, device="cuda")
        for b, at in enumerate(offs):
            flat[at:at + 3 * h * w] = frames[b].reshape(-1)
        xyxy_t = eng.scale_boxes(dets, counts, frames=table)
        assert torch.equal(xyxy_t, xyxy)
    print(f"B={B} frames {w}x{h}, {a.n_inst} planted instances per frame ({counts.float().mean().item():.1f} kept), "
          f"max_points {a.max_points}, dtype {a.dtype}")
    for native in (False, True):
        rb = eng.mask_native_layout(h, w)["row_bytes"] if native else W // 8
        buf = torch.zeros((cap, h if native else H, rb), dtype=torch.uint8, device="cuda")
        off = torch.empty((B + 1,), dtype=torch.int32, device="cuda")
        if native:
            eng.masks_native(dets, counts, xyxy, proto, h, w, "logit", "bits", capacity=cap, masks=buf, offsets=off)
        else:
            eng.masks(dets, counts, proto, "logit", "bits", capacity=cap, masks=buf, offsets=off)
        out = dict(dets=dets, xyxy=xyxy, counts=counts, offsets=off, masks=buf)
        out_t = out
        if a.mixed and native:         # the ragged rows of the same detections
            rag, off_t, bases = eng.masks_native_frames(dets, counts, xyxy, proto, table)
            out_t = dict(out, masks=rag, mask_bases=bases, offsets=off_t)
        plates = torch.zeros((cap, 4), dtype=torch.int32, device="cuda")
        box = xyxy.reshape(-1, 4)[:cap].to(torch.int32)
        plates[:, 0], plates[:, 1], plates[:, 2], plates[:, 3] = box[:, 0], box[:, 1] - 26, box[:, 0] + 110, box[:, 1] - 4
        for n_sel in a.n_sel:
            n_sel = min(n_sel, B)
            sel = [(k * (B // n_sel)) % B for k in range(n_sel)]
            idx = torch.tensor(sel, device="cuda")
            res = dict(frames=torch.empty((n_sel, h, w, 3), dtype=torch.uint8, device="cuda"),
                       status=torch.empty((n_sel,), dtype=torch.int32, device="cuda"))
            floor = torch.empty_like(res["frames"])
            picture = torch.empty_like(res["frames"])
            cpy = (lambda: floor.copy_(frames)) if n_sel == B else (lambda: torch.index_select(frames, 0, idx, out=floor))
            for mode in ("both", "draw", "blend"):
                ann = picture if mode == "blend" else None
                call = lambda: eng.overlay(frames, out, sel, native=native, plates=plates, mode=mode, annotated=ann, result=res,
                                           max_points=a.max_points)
                for _ in range(3):
                    call(); cpy()
                torch.cuda.synchronize()
                skipped = int((res["status"] != 0).sum())
                if mode == "draw":
                    picture.copy_(res["frames"])
                if a.mixed:             # the same selection through the frame table
                    pl_t = plates       # per slot index in either form: cap = B * max_det rows
                    ann_t = None
                    if mode == "blend":
                        first = eng.overlay(flat, out_t, sel, native=native, plates=pl_t, mode="draw", max_points=a.max_points, table=table)
                        ann_t = first["buf"].clone()
                    res_t = eng.overlay(flat, out_t, sel, native=native, plates=pl_t, mode=mode, annotated=ann_t, max_points=a.max_points,
                                        table=table)
                    res_t = dict(buf=res_t["buf"], status=res_t["status"])
                    call_t = lambda: eng.overlay(flat, out_t, sel, native=native, plates=pl_t, mode=mode, annotated=ann_t, result=res_t,
                                                 max_points=a.max_points, table=table)
                    got = call_t()
                    call()
                    torch.cuda.synchronize()
                    same = all(torch.equal(got["buf"][at:at + 3 * h * w].view(h, w, 3), res["frames"][k])
                               for k, at in enumerate(got["byte_offsets"])) and torch.equal(got["status"], res["status"])
                for run in range(2):
                    ta, tc, tm = [], [], []
                    for _ in range(a.rounds):
                        ta.append(group_ms(call))
                        if a.mixed:
                            tm.append(group_ms(call_t))
                        tc.append(group_ms(cpy))
                    ma, mc = float(np.median(ta)) * 1e3, float(np.median(tc)) * 1e3
                    print(f"  {'native rows   ' if native else 'letterbox bits'} {mode:5s} n_sel {n_sel:3d} run {run}: overlay {ma:9.1f} us/call "
                          f"(min {min(ta) * 1e3:.1f}), copy {mc:8.1f} us, ratio {ma / mc:6.2f}, {ma / n_sel:8.1f} us/selected frame, "
                          f"contours skipped on {skipped} frames")
                    if a.mixed:
                        mm = float(np.median(tm)) * 1e3
                        print(f"  {'native rows   ' if native else 'letterbox bits'} {mode:5s} n_sel {n_sel:3d} run {run}: frame table "
                              f"{mm:7.1f} us/call (min {min(tm) * 1e3:.1f}), {mm / ma:6.3f} of the uniform call, pictures "
                              f"{'equal' if same else 'DIFFER'}")


if __name__ == "__main__":
    main()
