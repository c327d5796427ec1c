"""What the NMS table costs: 64 frames at the bench's shape (640x640, nc = 80, 8400 anchors; synth_pred: 50 planted instances x 5
duplicates per frame) through the table-free NMS and through the same NMS with a table set -- one row for every frame, and four rows
of the same settings with a per-frame row index -- alternating the three in one run, timed with device events after warm-up.
    python3 tools/nms_table_bench.py [--iters 20] [--frames 64]
Both forms of the candidate filter are timed: vti_nms (nms_scan_kernel reads the class scores) and vti_nms_scored (the (score,
class) pairs).  A fourth line per form has a class set on the row (every second class), which removes about half of the candidates.
The table is set and cleared outside the timed interval (both are host only).  Prints the median and the range of the per-call times
and the ratio of each table line's median to the table-free one's; the outputs of the set-free table lines are compared with the
table-free call's, byte for byte."""
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
from gpu_util import synth_pred
from vti_amd._lib import check

CONF, IOU, MAX_DET = 0.25, 0.7, 300


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--frames", type=int, default=64)
    args = ap.parse_args()
    B, nc = args.frames, 80
    L = vti_amd.lib()
    eng = vti_amd.Engine("n", nc, H=640, W=640, max_batch=B, dtype="h2")
    eng.load_weights(vti_amd.random_weights(eng, seed=1), 0)
    rng = np.random.default_rng(0)
    pred_h = synth_pred(rng, B, nc, 32, eng.num_anchors)
    pred = eng._anchor_major(torch.from_numpy(pred_h).cuda())
    s = pred_h[:, 4:4 + nc]
    best = torch.from_numpy(np.ascontiguousarray(np.stack((s.max(1), s.argmax(1).astype(np.float32)), -1))).cuda()
    P = vti_amd.NmsParams
    one = eng.pack_nms_table([P(CONF, IOU, MAX_DET, False)])
    four = eng.pack_nms_table([P(CONF, IOU, MAX_DET, False)] * 4)
    half = eng.pack_nms_table([P(CONF, IOU, MAX_DET, False, tuple(range(0, nc, 2)))])
    idx = torch.arange(B, dtype=torch.int32, device="cuda") % 4
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    cases = {"table-free": None, "table, one row": (one, None), "table, four rows": (four, idx), "table, one row + class set": (half, None)}
    for scored in (False, True):
        outs = {k: (torch.empty((B, MAX_DET, 38), dtype=torch.float32, device="cuda"), torch.empty((B,), dtype=torch.int32, device="cuda"))
                for k in cases}

        def call(k):
            dets, counts = outs[k]
            if scored:
                check(eng._ctx, L.vti_nms_scored(eng._ctx, ptr(pred), ptr(best), B, CONF, IOU, MAX_DET, 0, ptr(dets), ptr(counts), st))
            else:
                check(eng._ctx, L.vti_nms(eng._ctx, ptr(pred), B, CONF, IOU, MAX_DET, 0, ptr(dets), ptr(counts), st))

        def run(k, events=None):
            t = cases[k]
            if t is not None:
                check(eng._ctx, L.vti_set_nms_table(eng._ctx, C.c_void_p(t[0].host.data_ptr()), ptr(t[0].dev), t[0].n_rows, ptr(t[1])))
            if events:
                events[0].record()
            call(k)
            if events:
                events[1].record()
            if t is not None:
                check(eng._ctx, L.vti_set_nms_table(eng._ctx, None, None, 0, None))

        for _ in range(3):
            for k in cases:
                run(k)
        torch.cuda.synchronize()
        ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.iters)] for k in cases}
        for i in range(args.iters):
            for k in cases:
                run(k, ev[k][i])
        torch.cuda.synchronize()
        print(f"{'vti_nms_scored' if scored else 'vti_nms'}: {B} frames, 640x640, nc {nc}, conf {CONF}, iou {IOU}, max_det {MAX_DET}; "
              f"kept per frame {int(outs['table-free'][1].min())} .. {int(outs['table-free'][1].max())}")
        base = None
        for k in cases:
            ms = [a.elapsed_time(b) for a, b in ev[k]]
            med = float(np.median(ms))
            base = med if base is None else base
            print(f"      {k:30s} median {med * 1e3:9.1f} us   min {min(ms) * 1e3:9.1f}   max {max(ms) * 1e3:9.1f}   ratio {med / base:6.3f}")
        for k in ("table, one row", "table, four rows"):
            same = all(torch.equal(a, b) for a, b in zip(outs[k], outs["table-free"]))
            print(f"      {k}: outputs {'equal' if same else 'DIFFER from'} the table-free call's")
            assert same


if __name__ == "__main__":
    main()
