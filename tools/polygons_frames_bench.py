"""vti_mask_polygons_frames cost: the polygons of a whole batch in one call against what it replaces, timed with device events
after warm-up (no host restatement here: tools/polygons_bench.py has that).
    python3 tools/polygons_frames_bench.py [--iters 10] [--n-inst 50] [--case mixed|uniform|both]
(a) mixed: 64 frames, 16 of each of four sizes, on a 960x960 canvas; synth_pred -> NMS -> masks as tools/polygons_bench.py makes
    them, letterbox bit masks (vti_masks) and the ragged frame-size rows (vti_masks_native_frames) of the SAME detections.  The one
    call against the work-around it replaces, 64 vti_mask_polygons calls on the same slots, in the same run.
(b) uniform: 64 frames of 1280x960 through vti_mask_polygons_frames with a table of equal rows against vti_mask_polygons on the same
    letterbox buffer, alternating the two; each is also timed on a second copy of the buffer with a second scratch, and the
    difference between a call's two medians is the spread to read the comparison against.
Prints per case, mask form and strategy the median and the range of the per-call times."""
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
from vti_amd.engine import POLY_STRATEGIES

MAX_DET = 200


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def timed_each(fns, iters, warmup=2):
    """Every fn of `fns` in turn, `iters` rounds: ms per call of each (device events around every call) -> {name: [ms]}."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)] for k in fns}
    for i in range(iters):
        for k, fn in fns.items():
            ev[k][i][0].record()
            fn()
            ev[k][i][1].record()
    torch.cuda.synchronize()
    return {k: [a.elapsed_time(b) for a, b in v] for k, v in ev.items()}


def show(name, ms):
    print(f"      {name:44s} median {np.median(ms) * 1e3:9.1f} us   min {min(ms) * 1e3:9.1f}   max {max(ms) * 1e3:9.1f}")
    return float(np.median(ms))


def detections(eng, B, H, W, n_inst, seed=0):
    rng = np.random.default_rng(seed)
    pred = torch.from_numpy(synth_pred(rng, B, 2, 32, eng.num_anchors, H=H, W=W, n_inst=n_inst)).cuda()
    proto = torch.from_numpy(rng.standard_normal((B, H // 4, W // 4, 32)).astype(np.float32)).to(eng.torch_dtype).cuda()
    dets, counts = eng.nms(pred, 0.25, 0.7, MAX_DET)
    return dets, counts, proto


def frames_call(eng, masks, native, bases, cbytes, off, table, cap, strategy, ws, po, buf, st):
    def call():
        check(eng._ctx, vti_amd.lib().vti_mask_polygons_frames(
            eng._ctx, ptr(masks), int(native), ptr(bases), cbytes, ptr(off), *table._ptrs(), table.B, cap, POLY_STRATEGIES[strategy],
            ptr(ws), ws.numel(), ptr(po), ptr(buf), buf.shape[0], st))
    return call


def uniform_call(eng, masks, n, n_live, mh, mw, rb, H0, W0, strategy, ws, po, buf, st):
    def call():
        check(eng._ctx, vti_amd.lib().vti_mask_polygons(
            eng._ctx, ptr(masks), n, n_live, mh, mw, rb, H0, W0, POLY_STRATEGIES[strategy], ptr(ws), ws.numel(), ptr(po), ptr(buf),
            buf.shape[0], st))
    return call


def mixed(a, st):
    sizes = [(960, 1280), (720, 960), (1080, 1920), (480, 640)]
    B, H, W = 64, 960, 960
    shapes = [sizes[b % 4] for b in range(B)]
    eng = vti_amd.Engine("n", 2, H=H, W=W, max_batch=B, dtype="h2")
    eng.load_weights(vti_amd.random_weights(eng, seed=1), 0)
    table, _, _ = eng.pack_frames(shapes, "cuda")
    dets, counts, proto = detections(eng, B, H, W, a.n_inst)
    cnt = counts.cpu().tolist()
    live, cap = sum(cnt), B * MAX_DET
    print(f"(a) mixed: {B} frames, 16 each of {sizes}, canvas {W}x{H}; {live} instances ({live / B:.1f} per frame), capacity {cap}")
    xyxy = eng.scale_boxes(dets, counts, frames=table)
    lb, off = eng.masks(dets, counts, proto, "logit", "bits", capacity=cap)
    rg, off2, bases = eng.masks_native_frames(dets, counts, xyxy, proto, table, "logit")
    off_h, bases_h = off.cpu().tolist(), bases.cpu().tolist()
    buf = torch.empty((1 << 22, 2), dtype=torch.float32, device="cuda")
    for native in (False, True):
        need = eng.mask_polygons_frames_scratch_bytes(table, native)
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        po = torch.empty((cap + 1,), dtype=torch.int32, device="cuda")
        per = []                                    # the work-around: frame b's slots as a uniform buffer
        for b, (h0, w0) in enumerate(shapes):
            if native:
                v = eng.frame_masks(rg, table, b, bases_h[b], cnt[b])
                per.append((v, cnt[b], h0, w0, v.shape[2], h0, w0))
            else:
                per.append((lb[off_h[b]:off_h[b] + cnt[b]], cnt[b], H, W, W // 8, h0, w0))
        pos = [torch.empty((n + 1,), dtype=torch.int32, device="cuda") for _, n, *_ in per]
        print(f"  {'ragged frame-size rows' if native else 'letterbox bit masks'}: scratch {need / 2 ** 20:.0f} MiB")
        for strategy in ("largest", "concat"):
            one = frames_call(eng, rg if native else lb, native, bases if native else None, rg.numel() if native else 0,
                              off2 if native else off, table, cap, strategy, ws, po, buf, st)
            calls = [uniform_call(eng, m, n, None, mh, mw, rb, h0, w0, strategy, ws, p, buf, st)
                     for (m, n, mh, mw, rb, h0, w0), p in zip(per, pos) if n]

            def work_around():
                for c in calls:
                    c()
            one()
            total = int(po[cap])
            assert total <= buf.shape[0] and int(ws[:4].view(torch.int32)[0]) == 0
            t = timed_each({"one": one, "64": work_around}, a.iters)
            print(f"    {strategy}: {total} vertices")
            m1 = show("vti_mask_polygons_frames, one call", t["one"])
            m64 = show(f"{len(calls)} vti_mask_polygons calls", t["64"])
            print(f"      one call / work-around = {m1 / m64:.3f}")


def uniform(a, st):
    B, H0, W0 = 64, 960, 1280
    H, W = vti_amd.letterbox_shape(H0, W0, 960)
    eng = vti_amd.Engine("n", 2, H=H, W=W, max_batch=B, dtype="h2")
    eng.load_weights(vti_amd.random_weights(eng, seed=1), 0)
    table, _, _ = eng.pack_frames([(H0, W0)] * B, "cuda")
    dets, counts, proto = detections(eng, B, H, W, a.n_inst)
    live, cap = int(counts.sum()), B * MAX_DET
    print(f"(b) uniform: {B} frames {W0}x{H0}, letterbox {W}x{H}; {live} instances, capacity {cap}")
    X, off = eng.masks(dets, counts, proto, "logit", "bits", capacity=cap)
    Y = X.clone()
    need = eng.mask_polygons_frames_scratch_bytes(table, False)
    assert need == eng.mask_polygons_scratch_bytes(H, W, W // 8)
    wsx, wsy = (torch.empty(need, dtype=torch.uint8, device="cuda") for _ in range(2))
    bx, by = (torch.empty((1 << 22, 2), dtype=torch.float32, device="cuda") for _ in range(2))
    px, py = (torch.empty((cap + 1,), dtype=torch.int32, device="cuda") for _ in range(2))
    n_live = C.c_void_p(off.data_ptr() + 4 * B)
    for strategy in ("largest", "concat"):
        fns = {"vti_mask_polygons, buffer X": uniform_call(eng, X, cap, n_live, H, W, W // 8, H0, W0, strategy, wsx, px, bx, st),
               "vti_mask_polygons_frames, buffer X": frames_call(eng, X, False, None, 0, off, table, cap, strategy, wsx, px, bx, st),
               "vti_mask_polygons, buffer Y": uniform_call(eng, Y, cap, n_live, H, W, W // 8, H0, W0, strategy, wsy, py, by, st),
               "vti_mask_polygons_frames, buffer Y": frames_call(eng, Y, False, None, 0, off, table, cap, strategy, wsy, py, by, st)}
        t = timed_each(fns, a.iters)
        print(f"    {strategy}: {int(px[cap])} vertices")
        med = {k: show(k, v) for k, v in t.items()}
        old = [med["vti_mask_polygons, buffer X"], med["vti_mask_polygons, buffer Y"]]
        new = [med["vti_mask_polygons_frames, buffer X"], med["vti_mask_polygons_frames, buffer Y"]]
        print(f"      spread between the two buffers: vti_mask_polygons {abs(old[0] - old[1]) * 1e3:.1f} us, "
              f"vti_mask_polygons_frames {abs(new[0] - new[1]) * 1e3:.1f} us; frames - uniform, mean of both buffers: "
              f"{(sum(new) - sum(old)) / 2 * 1e3:+.1f} us ({(sum(new) / sum(old) - 1) * 100:+.2f} %)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--n-inst", type=int, default=50)
    ap.add_argument("--case", choices=("mixed", "uniform", "both"), default="both")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("polygons_frames_bench needs the GPU")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if a.case in ("mixed", "both"):
        mixed(a, st)
    if a.case in ("uniform", "both"):
        uniform(a, st)


if __name__ == "__main__":
    main()
