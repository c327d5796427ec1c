"""vti_annotate_checker next to vti_annotate: both calls on the SAME 64-frame 960x1280 letterbox batch (the sixteen scenes of
tests/test_gpu_checker.py, four times over), every frame selected, timed with device events after warm-up, the two interleaved in
groups of 10 calls, two runs.  The two calls share the outline and raster kernels, so the prep kernel is the only place a difference
can come from; its own duration comes from a kernel trace in a run of its own:
    python3 tools/annotate_checker_bench.py [--iters 100] [--B 64]
    rocprofv3 --kernel-trace --stats -d OUT -- python3 tools/annotate_checker_bench.py --iters 20
Prints us per call and per frame for both, and checks first that the two pictures differ and that each call repeats itself."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

import vti_amd
import test_gpu_checker as tc
from gpu_util import frames_u8


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


def batch(B, h, w, mh, mw):
    """The sixteen scenes repeated to B frames, every slot live: the arrays of one output set, on the device."""
    arr = tc.host_batch(h, w, mh, mw, False, 0)[0]
    reps = -(-B // len(arr["counts"]))
    counts = np.tile(arr["counts"], reps)[:B]
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    masks = np.concatenate([arr["masks"]] * reps)[:int(offsets[-1])]
    o = dict(dets=np.tile(arr["dets"], (reps, 1, 1))[:B], xyxy=np.tile(arr["xyxy"], (reps, 1, 1))[:B], counts=counts, offsets=offsets,
             masks=masks)
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in o.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--B", type=int, default=64)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("annotate_checker_bench needs the GPU")
    mode, h, w, mh, mw = tc.MODES[0]
    B = a.B
    eng = vti_amd.Engine("n", 2, H=mh, W=mw, max_batch=B)
    o = batch(B, h, w, mh, mw)
    frames = torch.from_numpy(frames_u8(B, h, w, 0)).cuda()
    sel = list(range(B))
    cp = vti_amd.CheckerParams(*tc.CALIB)
    mp = vti_amd.MeasureParams(*tc.CALIB, roi_enabled=False, max_px_distance=150)
    cmeas, mmeas = eng.measure_checker(o, cp, h, w), eng.measure(o, mp, h, w)
    cres = eng.annotate_checker(frames, o, cmeas, cp, sel)
    table = eng.pack_cameras([mp], "cuda")
    mres = eng.annotate(frames, o, mmeas, table, sel)
    cases = {"vti_annotate        ": lambda: eng.annotate(frames, o, mmeas, table, sel, result=mres),
             "vti_annotate_checker": lambda: eng.annotate_checker(frames, o, cmeas, cp, sel, result=cres)}
    first = {k: None for k in cases}
    for k, fn in cases.items():
        fn()
        first[k] = (mres if "checker" not in k else cres)["frames"].clone()
        timed(fn, 5, warmup=2)
        assert torch.equal(first[k], (mres if "checker" not in k else cres)["frames"]), k      # each call repeats itself
    assert not torch.equal(*first.values())
    ok = int((cmeas["frame_i32"][:, 0] == 0).sum())
    print(f"B={B} frames {w}x{h}, letterbox {mw}x{mh}, all selected; {int(o['counts'].sum())} instances; checker status 0 in {ok}/{B} frames; "
          f"outline skipped in {int(cres['status'].sum())} / {int(mres['status'].sum())} frames")
    for run in range(2):
        acc = {k: [] for k in cases}
        for _ in range(max(a.iters // 10, 1)):
            for k, fn in cases.items():
                acc[k].append(timed(fn, 10) * 1e3)
        for k in cases:
            print(f"  run {run}  {k}  {np.mean(acc[k]):8.1f} us/call  {np.mean(acc[k]) / B:6.2f} us/frame  "
                  f"(min group {min(acc[k]):.1f}, max {max(acc[k]):.1f})")


if __name__ == "__main__":
    main()
