"""vti_annotate cost: the annotated frames of a selection of one batch, from letterbox-size bit masks (vti_masks) and from
frame-size ones (vti_masks_native), on the SAME detections (synth_pred -> NMS -> scale_boxes -> vti_measure), timed with device
events after warm-up, next to the floor measured in the same run: a device-to-device copy of the same n_sel frames, which is what
the call must at least do.
    python3 tools/annotate_bench.py [--dtype h2] [--B 64] [--n-inst 50] [--n-sel 1 8 64] [--rounds 5] [--max-points 16384]
                                    [--size 960 1280] [--mixed]
--size: the frame size of the uniform batch.  --mixed: vti_annotate_frames instead, on a batch of B frames that cycles the four sizes
of the tests (481 x 333, 720 x 960, 960 x 1280, 1080 x 1920; B = 64: 16 frames each), letterbox bits only, every frame selected; the
floor is a device-to-device copy of the flat frame buffer.  What it replaces is one uniform call per size (--size h w --B 16 --n-sel 16).
The two (annotate, copy) are interleaved in groups of 10 calls, `--rounds` groups each, and the whole measurement runs twice.
Prints per mask form and n_sel: us per call (three launches), the copy's us, their ratio, us per selected frame."""
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
from test_oracle_geometry import load_calib

MIXED_SIZES = [(481, 333), (720, 960), (960, 1280), (1080, 1920)]       # tests/test_gpu_annotate_frames.py


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
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--n-inst", type=int, default=50)
    ap.add_argument("--n-sel", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-points", type=int, default=16384)
    ap.add_argument("--size", type=int, nargs=2, default=[960, 1280], metavar=("H0", "W0"))
    ap.add_argument("--mixed", action="store_true")
    a = ap.parse_args()
    H, W, (h, w), B = 736, 960, a.size, a.B
    eng = vti_amd.Engine("n", 2, H=H, W=W, max_batch=B, dtype=a.dtype)
    eng.load_weights(vti_amd.random_weights(eng, 1), 0)
    rng = np.random.default_rng(5)
    pred = torch.from_numpy(synth_pred(rng, B, 2, 32, eng.num_anchors, H=H, W=W, n_inst=a.n_inst)).cuda()
    proto = torch.from_numpy(rng.standard_normal((B, H // 4, W // 4, 32)).astype(np.float32)).cuda()
    proto = vti_amd.h2_encode(proto) if eng.dtype == "h2" else proto.to(eng.torch_dtype)     # the engine's own storage type
    dets, counts = eng.nms(pred, 0.25, 0.7, 200)
    if a.mixed:
        return mixed(a, eng, dets, counts, proto)
    frames = torch.from_numpy(frames_u8(B, h, w, 0)).cuda()
    xyxy = eng.scale_boxes(dets, counts, h, w)
    cap = B * 200
    params = vti_amd.MeasureParams(*load_calib())
    table = eng.pack_cameras([params], "cuda")
    print(f"B={B} frames {w}x{h}, {a.n_inst} planted instances per frame, max_points {a.max_points}, dtype {a.dtype}")
    for native in (False, True):
        rb = eng.mask_native_layout(h, w)["row_bytes"] if native else W // 8
        buf = torch.zeros((cap, h if native else H, rb), dtype=torch.uint8, device="cuda")
        off = torch.empty((B + 1,), dtype=torch.int32, device="cuda")
        if native:
            eng.masks_native(dets, counts, xyxy, proto, h, w, "logit", "bits", capacity=cap, masks=buf, offsets=off)
        else:
            eng.masks(dets, counts, proto, "logit", "bits", capacity=cap, masks=buf, offsets=off)
        out = dict(dets=dets, xyxy=xyxy, counts=counts, offsets=off, masks=buf)
        meas = eng.measure(out, params, h, w, native=native)
        st = meas["frame_i32"][:, 0].cpu().tolist()
        print(f"{'native rows' if native else 'letterbox bits'}: statuses ok/no_fabric/no_stitches = "
              f"{st.count(0)}/{st.count(1)}/{st.count(2)}, instances per frame {counts.float().mean().item():.1f}")
        for n_sel in a.n_sel:
            n_sel = min(n_sel, B)
            sel = [(k * (B // n_sel)) % B for k in range(n_sel)]
            idx = torch.tensor(sel, device="cuda")
            res = dict(frames=torch.empty((n_sel, h, w, 3), dtype=torch.uint8, device="cuda"),
                       status=torch.empty((n_sel,), dtype=torch.int32, device="cuda"))
            floor = torch.empty_like(res["frames"])
            ann = lambda: eng.annotate(frames, out, meas, table, sel, native=native, result=res, max_points=a.max_points)
            cpy = (lambda: floor.copy_(frames)) if n_sel == B else (lambda: torch.index_select(frames, 0, idx, out=floor))
            for _ in range(3):
                ann(); cpy()
            torch.cuda.synchronize()
            skipped = int((res["status"] != 0).sum())
            for run in range(2):
                ta, tc = [], []
                for _ in range(a.rounds):
                    ta.append(group_ms(ann))
                    tc.append(group_ms(cpy))
                ma, mc = float(np.median(ta)) * 1e3, float(np.median(tc)) * 1e3
                print(f"  n_sel {n_sel:3d} run {run}: annotate {ma:9.1f} us/call (min {min(ta) * 1e3:.1f}), copy {mc:8.1f} us, "
                      f"ratio {ma / mc:5.2f}, {ma / n_sel:8.1f} us/selected frame, outlines skipped {skipped}")


def mixed(a, eng, dets, counts, proto):
    B, cap = a.B, a.B * 200
    shapes = [MIXED_SIZES[b % 4] for b in range(B)]
    ft, offs, total = eng.pack_frames(shapes, "cuda")
    flat = torch.from_numpy(np.random.Generator(np.random.PCG64(0)).integers(0, 256, total, dtype=np.uint8)).cuda()
    params = vti_amd.MeasureParams(*load_calib())
    table = eng.pack_cameras([params], "cuda")
    buf = torch.zeros((cap, eng.H, eng.W // 8), dtype=torch.uint8, device="cuda")
    off = torch.empty((B + 1,), dtype=torch.int32, device="cuda")
    eng.masks(dets, counts, proto, "logit", "bits", capacity=cap, masks=buf, offsets=off)
    out = dict(dets=dets, xyxy=eng.scale_boxes(dets, counts, frames=ft), counts=counts, offsets=off, masks=buf)
    meas = eng.measure(out, table, cameras=torch.zeros(B, dtype=torch.int32, device="cuda"), frames=ft)
    st = meas["frame_i32"][:, 0].cpu().tolist()
    print(f"mixed B={B}: {B // 4} frames of each of {MIXED_SIZES}, {total / 1e6:.1f} MB; statuses ok/no_fabric/no_stitches = "
          f"{st.count(0)}/{st.count(1)}/{st.count(2)}, instances per frame {counts.float().mean().item():.1f}")
    sel = list(range(B))
    res = dict(buf=torch.empty(total, dtype=torch.uint8, device="cuda"), status=torch.empty((B,), dtype=torch.int32, device="cuda"))
    floor = torch.empty_like(flat)
    ann = lambda: eng.annotate(flat, out, meas, table, sel, result=res, max_points=a.max_points, table=ft)
    cpy = lambda: floor.copy_(flat)
    for _ in range(3):
        ann(); cpy()
    torch.cuda.synchronize()
    skipped = int((res["status"] != 0).sum())
    for run in range(2):
        ta, tc = [], []
        for _ in range(a.rounds):
            ta.append(group_ms(ann))
            tc.append(group_ms(cpy))
        ma, mc = float(np.median(ta)) * 1e3, float(np.median(tc)) * 1e3
        print(f"  mixed n_sel {B:3d} run {run}: annotate_frames {ma:9.1f} us/call (min {min(ta) * 1e3:.1f}), copy {mc:8.1f} us, "
              f"ratio {ma / mc:5.2f}, {ma / B:8.1f} us/selected frame, outlines skipped {skipped}")


if __name__ == "__main__":
    main()
