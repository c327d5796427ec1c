"""vti_stamp cost and the bytes that cross the bus with the text burned in on the device, against the raw path (pictures to the host,
cv2.putText and cv2.imwrite there).  One batch of B frames (default 64 of 960 x 1280) on synthetic detections, the text of a typical
record on every frame: `--labels` width labels (default 50) and three lines (the info line, "Stitches | Fabric", the caller's status
line).  vti_annotate, vti_stamp and vti_encode_jpeg are timed in the same run with device events after warm-up, interleaved in groups
of 10 calls, `--rounds` groups each, the whole measurement twice.  vti_stamp is timed on three tables: the text on every picture, no
stamp at all (nothing is launched), and text on picture 0 only (the launch is the same grid; the workgroups of the other pictures leave
after one 16-byte read), which shows that a picture without stamps adds no picture traffic.
    timeout -k 10 600 python3 tools/stamp_bench.py [--B 64] [--size 960 1280] [--labels 50] [--rounds 5] [--quality 95]
The strings are rasterised with cv2.putText where OpenCV is installed; elsewhere with a stand-in that fills, per character, a cell of
putText's size with a fixed dot pattern (the table and the kernel do not care which; the line printed first says which it was)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

import vti_amd
from gpu_util import frames_u8, synth_pred
from test_oracle_geometry import load_calib
from vti_amd import annotate as A


def cell_rasterise(canvas, item):
    """Stand-in for cv2.putText: per character a cell of about the Hershey simplex advance (19 x 22 px at scale 1) above the
    baseline, every other dot of a 5 x 7 pattern taken from the character code set, each dot `thickness` pixels larger."""
    text, (x, y), _, scale, _, thick = item
    cw, ch = max(int(round(19 * scale)), 3), max(int(round(22 * scale)), 4)
    H, W = canvas.shape
    for i, c in enumerate(text):
        if c == " ":
            continue
        bits = (ord(c) * 2654435761) & 0xFFFFFFFFF
        for dot in range(35):
            if not (bits >> dot) & 1:
                continue
            x0 = x + i * cw + (dot % 5) * cw // 6
            y0 = y - ch + (dot // 5) * ch // 7
            xa, xb, ya, yb = max(x0, 0), min(x0 + thick + 1, W), max(y0, 0), min(y0 + thick + 1, H)
            if xa < xb and ya < yb:
                canvas[ya:yb, xa:xb] = 255


def record_items(b, h, w, labels, rng):
    """The items of a typical frame in annotate.text_items' form: `labels` width labels, the info line, the counts, a status line."""
    items = []
    for j in range(labels):
        cx, cy = int(rng.integers(20, w - 60)), int(rng.integers(320, h - 220))
        items.append((f"{rng.uniform(2, 9):.1f}", (cx + 2, cy - 20), A.FONT, 0.60, (0, 0, 0), 2))
    items.append((f"Edge Dist: {rng.uniform(3, 9):.2f}mm | Avg Width: {rng.uniform(2, 6):.2f}mm (n_d={labels}, n_w={labels})", (10, 30), A.FONT, 0.7,
                  (0, 0, 255), 2))
    items.append((f"Stitches: {labels} | Fabric: 1", (10, h - 10), A.FONT, 0.5, (0, 0, 0), 1))
    items.append((f"Frame {b:06d}  OK  12.5 fps", (10, 60), A.FONT, 0.7, (0, 255, 0), 2))
    return items


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
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--size", type=int, nargs=2, default=[960, 1280], metavar=("H0", "W0"))
    ap.add_argument("--labels", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quality", type=int, default=95)
    ap.add_argument("--n-inst", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("stamp_bench: no GPU (a time is measured on the device or not at all)")
    H, W, (h, w), B = 736, 960, a.size, a.B
    try:
        import cv2  # noqa: F401
        rasterise, which = None, "cv2.putText"
    except ImportError:
        rasterise, which = cell_rasterise, "the stand-in cell rasteriser (no OpenCV here)"
    eng = vti_amd.Engine("n", 2, H=H, W=W, max_batch=B, dtype="h2")
    eng.load_weights(vti_amd.random_weights(eng, 1), 0)
    rng = np.random.default_rng(5)
    pred = torch.from_numpy(synth_pred(rng, B, 2, 32, eng.num_anchors, H=H, W=W, n_inst=a.n_inst)).cuda()
    proto = vti_amd.h2_encode(torch.from_numpy(rng.standard_normal((B, H // 4, W // 4, 32)).astype(np.float32)).cuda())
    dets, counts = eng.nms(pred, 0.25, 0.7, 200)
    frames = torch.from_numpy(frames_u8(B, h, w, 0)).cuda()
    xyxy = eng.scale_boxes(dets, counts, h, w)
    cap = B * 200
    params = vti_amd.MeasureParams(*load_calib())
    table = eng.pack_cameras([params], "cuda")
    buf = torch.zeros((cap, H, W // 8), dtype=torch.uint8, device="cuda")
    off = torch.empty((B + 1,), dtype=torch.int32, device="cuda")
    eng.masks(dets, counts, proto, "logit", "bits", capacity=cap, masks=buf, offsets=off)
    out = dict(dets=dets, xyxy=xyxy, counts=counts, offsets=off, masks=buf)
    meas = eng.measure(out, params, h, w)
    sel = list(range(B))
    res = dict(frames=torch.empty((B, h, w, 3), dtype=torch.uint8, device="cuda"), status=torch.empty((B,), dtype=torch.int32, device="cuda"))

    t0 = time.perf_counter()
    per = [A.text_stamps(record_items(b, h, w, a.labels, rng), h, w, rasterise) for b in range(B)]
    t1 = time.perf_counter()
    full = eng.pack_stamps(per, [(h, w)] * B, "cuda")
    t2 = time.perf_counter()
    none = eng.pack_stamps([[]] * B, [(h, w)] * B, "cuda")
    first = eng.pack_stamps([per[0]] + [[]] * (B - 1), [(h, w)] * B, "cuda")
    set_px = sum(int(s[2].sum()) for p in per for s in p)
    print(f"B={B} frames {w}x{h}; text by {which}: {full.n_stamps} stamps ({full.n_stamps / B:.1f} per frame), {set_px / B:.0f} painted pixels "
          f"per frame, table {full.host.numel()} B + bits {4 * full.n_words} B = {full.up_bytes / B:.0f} B per frame going up")
    print(f"host: text_stamps {1e3 * (t1 - t0) / B:.2f} ms per frame, pack_stamps + upload {1e3 * (t2 - t1) / B:.3f} ms per frame")

    ann = lambda: eng.annotate(frames, out, meas, table, sel, result=res)
    enc = lambda: eng.encode_jpeg(res["frames"], quality=a.quality)
    calls = [("vti_annotate", ann), ("vti_stamp, text on every picture", lambda: eng.stamp(res["frames"], full)),
             ("vti_stamp, text on picture 0 only", lambda: eng.stamp(res["frames"], first)),
             ("vti_stamp, no stamps (no launch)", lambda: eng.stamp(res["frames"], none)), ("vti_encode_jpeg", enc)]
    for _ in range(3):
        for _, fn in calls:
            fn()
    torch.cuda.synchronize()
    data, offs = enc()
    file_bytes = int(offs[-1])
    for run in range(2):
        t = {name: [] for name, _ in calls}
        for _ in range(a.rounds):
            for name, fn in calls:
                t[name].append(group_ms(fn))
        for name, _ in calls:
            m = float(np.median(t[name])) * 1e3
            print(f"  run {run}: {name:36s} {m:10.1f} us/call (min {min(t[name]) * 1e3:.1f}), {m / B:8.2f} us/frame")
    raw = 3 * h * w * B
    print(f"bus, burned path: up {full.up_bytes} B (stamps), down {file_bytes + 8 * (B + 1)} B (files at quality {a.quality} + offsets) = "
          f"{(full.up_bytes + file_bytes + 8 * (B + 1)) / B / 1e3:.1f} KB per frame")
    print(f"bus, raw path:    up 0 B, down {raw} B (pictures, 3 bytes per pixel) = {raw / B / 1e3:.1f} KB per frame; ratio "
          f"{raw / (full.up_bytes + file_bytes + 8 * (B + 1)):.1f} x")


if __name__ == "__main__":
    main()
