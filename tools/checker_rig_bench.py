"""The stitch-distance checker's rig calls next to the per-size, per-camera calls they replace, and the one-struct calls next to a
parent build's.  64 frames x 50 instances (a fabric, a fabric with an empty mask, 48 stitches), 16 frames of each of four sizes,
four cameras, a 736 x 960 canvas; device events after warm-up, the calls of a comparison interleaved in groups of 10, two runs.
    python3 tools/checker_rig_bench.py [--iters 50] [--parent-lib PATH]
1. vti_measure_checker_frames, vti_measure_checker_frames_native and vti_annotate_checker_frames (every frame selected), each
   against its work-around: the batch regrouped by (size, camera) beforehand -- 16 groups of 4 frames, every group an output set of
   its own, built before the timing -- and one vti_measure_checker / vti_annotate_checker call per group.  The results are compared
   first, word for word and byte for byte.
2. vti_measure_checker and vti_annotate_checker on 64 frames of 960 x 1280 (letterbox masks), called through the bare C ABI on the
   same inputs: this build, this build again with a second context and scratch (what two sets of buffers alone differ by), and
   with --parent-lib PATH (a libvti.so built from the parent commit) that build too, alternating parent, here, here again, twice.
   --part 1 / --part 2 runs one part only."""
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
from gpu_util import frames_u8
from test_gpu_checker_rig import _fab, _st, render
from test_gpu_measure import pack
from test_gpu_measure_cameras import CALIBS

MH, MW, MAX_DET, N_INST = 736, 960, 64, 50
SIZES = [(960, 1280), (720, 960), (1080, 1920), (481, 333)]
KEYS = ("frame_f64", "frame_i32", "stitch_f64", "stitch_i32")


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


def scene():
    return ([_fab(0.04, 0.30, 0.96, 0.93), _fab(0.50, 0.18, 0.90, 0.50, "empty")] +
            [_st(0.08 + 0.075 * k, 0.45 + 0.12 * r, 0.04, 0.03) for r in range(4) for k in range(12)])


def output_set(shapes, native):
    """The output set of a predict on frames of `shapes`, every frame the scene above: letterbox slots u8 [n, MH, MW / 8], or native
    the ragged rows (flat u8, bases).  One rendering per (size, instance), shared by the frames of that size."""
    rng = np.random.default_rng(1)
    insts = scene()
    assert len(insts) == N_INST
    B = len(shapes)
    per = {}
    for hw in sorted(set(shapes)):
        h, w = hw
        r = [render(x, h, w, *((h, w) if native else (MH, MW)), rng) for x in insts]
        per[hw] = (np.stack([pack(m, native, w) for m, _, _ in r]), np.array([f for _, f, _ in r], np.float32),
                   np.array([m for _, _, m in r], np.float32))
    dets = np.zeros((B, MAX_DET, 38), np.float32)
    xyxy = np.zeros((B, MAX_DET, 4), np.float32)
    for b, hw in enumerate(shapes):
        dets[b, :N_INST, :4], xyxy[b, :N_INST] = per[hw][2], per[hw][1]
        dets[b, :N_INST, 4] = 0.9
        dets[b, :N_INST, 5] = [0 if x["role"] == "stitch" else 1 for x in insts]
    counts = np.full(B, N_INST, np.int32)
    offsets = np.arange(B + 1, dtype=np.int32) * N_INST
    o = {k: torch.from_numpy(v).cuda() for k, v in dict(dets=dets, xyxy=xyxy, counts=counts, offsets=offsets).items()}
    dev = {hw: torch.from_numpy(v[0]).cuda() for hw, v in per.items()}
    if native:
        o["masks"] = torch.cat([dev[hw].reshape(-1) for hw in shapes])
        sizes = [dev[hw].numel() for hw in shapes]
        o["mask_bases"] = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64, device="cuda")
    else:
        o["masks"] = torch.cat([dev[hw] for hw in shapes])
    return o


def subset(o, frames, native, hw):
    """The output set of the frames `frames` (all of size hw) as a batch of its own."""
    idx = torch.tensor(frames, device="cuda")
    s = dict(dets=o["dets"][idx].contiguous(), xyxy=o["xyxy"][idx].contiguous(), counts=o["counts"][idx].contiguous(),
             offsets=torch.arange(len(frames) + 1, dtype=torch.int32, device="cuda") * N_INST)
    if native:
        h, w = hw
        rb = 8 * -(-w // 64)
        bases = o["mask_bases"].cpu().tolist()
        s["masks"] = torch.cat([o["masks"][bases[b]:bases[b + 1]] for b in frames]).view(len(frames) * N_INST, h, rb)
    else:
        s["masks"] = torch.cat([o["masks"][b * N_INST:(b + 1) * N_INST] for b in frames])
    return s


def same(a, b, what):
    assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), what


def interleave(cases, iters, B):
    for run in range(2):
        acc = {k: [] for k in cases}
        for _ in range(max(iters // 10, 1)):
            for k, fn in cases.items():
                acc[k].append(timed(fn, 10) * 1e3)
        for k in cases:
            print(f"  run {run}  {k:44s} {np.mean(acc[k]):9.1f} us/call {np.mean(acc[k]) / B:7.2f} us/frame  "
                  f"(min group {min(acc[k]):.1f}, max {max(acc[k]):.1f})")
        base = np.mean(acc[list(cases)[0]])
        for k in list(cases)[1:]:
            print(f"  run {run}  {k.strip()} / {list(cases)[0].strip()} = {np.mean(acc[k]) / base:.3f}")


def rig_part(eng, iters):
    B = 64
    shapes = [SIZES[b % 4] for b in range(B)]
    cams = [(b // 4) % 4 for b in range(B)]
    plist = [vti_amd.CheckerParams(*CALIBS[c % 2], min_stitches=3 - c // 2, envelope_neighborhood=3 + c) for c in range(4)]
    table = eng.pack_checker_cameras(plist, "cuda")
    idx = torch.tensor(cams, dtype=torch.int32, device="cuda")
    ft, at, total = eng.pack_frames(shapes, "cuda")
    groups = {}
    for b in range(B):
        groups.setdefault((shapes[b], cams[b]), []).append(b)
    print(f"1. B={B}, {N_INST} instances per frame, sizes {SIZES}, 4 cameras; the work-around: {len(groups)} groups of "
          f"{len(next(iter(groups.values())))} frames")
    sets = {}
    for native in (False, True):
        o = output_set(shapes, native)
        if native:
            o["native_shapes"] = tuple(ft.shapes)
        res = eng.measure_checker(o, table, cameras=idx, frames=ft, native=native)
        res = {k: v.clone() for k, v in res.items()}
        subs = {g: subset(o, fr, native, g[0]) for g, fr in groups.items()}
        sub_res = {}
        for (hw, c), fr in groups.items():
            r = eng.measure_checker(subs[(hw, c)], plist[c], *hw, native=native)
            sub_res[(hw, c)] = {k: v.clone() for k, v in r.items()}
            for k, b in enumerate(fr):
                same(res["frame_f64"][b], r["frame_f64"][k], ("frame_f64", b))
                same(res["frame_i32"][b], r["frame_i32"][k], ("frame_i32", b))
                same(res["stitch_f64"][b * N_INST:(b + 1) * N_INST], r["stitch_f64"][k * N_INST:(k + 1) * N_INST], ("stitch_f64", b))
                same(res["stitch_i32"][b * N_INST:(b + 1) * N_INST], r["stitch_i32"][k * N_INST:(k + 1) * N_INST], ("stitch_i32", b))
        ok = int((res["frame_i32"][:, 0] == 0).sum())
        print(f" {'native rows' if native else 'letterbox masks'}: status 0 in {ok}/{B} frames, the rig call equals the {len(groups)} calls word for word")
        sets[native] = (o, res, subs, sub_res)

        def rig(o=o, native=native, res=res):
            eng.measure_checker(o, table, cameras=idx, frames=ft, native=native, result=res)

        def regrouped(subs=subs, native=native, sub_res=sub_res):
            for (hw, c), s in subs.items():
                eng.measure_checker(s, plist[c], *hw, native=native, result=sub_res[(hw, c)])
        name = "vti_measure_checker_frames_native" if native else "vti_measure_checker_frames"
        timed(rig, 3), timed(regrouped, 3)
        interleave({f"{len(groups)} x vti_measure_checker": regrouped, name: rig}, iters, B)
    # the pictures, from the letterbox set
    o, res, subs, sub_res = sets[False]
    pics = {hw: torch.from_numpy(frames_u8(1, *hw, 7)[0]).cuda() for hw in SIZES}
    buf = torch.zeros(total, dtype=torch.uint8, device="cuda")
    for b, hw in enumerate(shapes):
        buf[at[b]:at[b] + pics[hw].numel()] = pics[hw].reshape(-1)
    sel = list(range(B))
    out = eng.annotate_checker(buf, o, res, table, sel, cameras=idx, table=ft)
    gframes = {g: pics[g[0]][None].expand(len(fr), -1, -1, -1).contiguous() for g, fr in groups.items()}
    gout = {}
    for (hw, c), fr in groups.items():
        g = eng.annotate_checker(gframes[(hw, c)], subs[(hw, c)], sub_res[(hw, c)], plist[c], list(range(len(fr))))
        gout[(hw, c)] = g
        for k, b in enumerate(fr):
            h, w = hw
            same(out["buf"][out["byte_offsets"][b]:out["byte_offsets"][b] + 3 * h * w], g["frames"][k].reshape(-1), ("picture", b))
    print(f" the pictures: vti_annotate_checker_frames equals the {len(groups)} calls byte for byte; outline skipped in "
          f"{int(out['status'].sum())} frames")

    def rig_draw():
        eng.annotate_checker(buf, o, res, table, sel, cameras=idx, table=ft, result=out)

    def regrouped_draw():
        for (hw, c), fr in groups.items():
            eng.annotate_checker(gframes[(hw, c)], subs[(hw, c)], sub_res[(hw, c)], plist[c], list(range(len(fr))), result=gout[(hw, c)])
    timed(rig_draw, 3), timed(regrouped_draw, 3)
    interleave({f"{len(groups)} x vti_annotate_checker": regrouped_draw, "vti_annotate_checker_frames": rig_draw}, iters, B)


def raw_calls(path, eng, o, res, frames, out, cp, B, h, w, cap, n_sel, dev_sel, host_sel):
    """vti_measure_checker and vti_annotate_checker of the library at `path` on this process's buffers, through ctypes alone."""
    from vti_amd import _lib
    L = C.CDLL(path)
    P, I = C.c_void_p, C.c_int32
    L.vti_create.restype, L.vti_create.argtypes = I, [C.POINTER(_lib.VtiDesc), C.POINTER(P)]
    for name in ("vti_measure_checker", "vti_annotate_checker", "vti_annotate_scratch_bytes", "vti_measure_scratch_bytes"):
        getattr(L, name).restype, getattr(L, name).argtypes = _lib.SIGNATURES[name]
    ctx = P(0)
    desc = _lib.VtiDesc(b"n", 2, 32, 16, eng.H, eng.W, B, _lib.VTI_F16)
    assert L.vti_create(C.byref(desc), C.byref(ctx)) == 0
    ws = torch.empty(max(L.vti_measure_scratch_bytes(ctx, B, cap, w), L.vti_annotate_scratch_bytes(ctx, n_sel, MAX_DET, h, w, 16384)),
                     dtype=torch.uint8, device="cuda")
    pres = {k: torch.empty_like(res[k]) for k in KEYS}
    pout = dict(frames=torch.empty_like(out["frames"]), status=torch.empty_like(out["status"]))
    ptr = lambda t: P(t.data_ptr())
    c = cp.to_c()
    stream = lambda: P(torch.cuda.current_stream().cuda_stream)

    def measure():
        rc = L.vti_measure_checker(ctx, C.byref(c), ptr(o["masks"]), 0, ptr(o["dets"]), ptr(o["xyxy"]), ptr(o["counts"]), ptr(o["offsets"]),
                                   B, MAX_DET, cap, h, w, ptr(ws), ws.numel(), ptr(pres["frame_f64"]), ptr(pres["frame_i32"]),
                                   ptr(pres["stitch_f64"]), ptr(pres["stitch_i32"]), stream())
        assert rc == 0, rc

    def draw():
        rc = L.vti_annotate_checker(ctx, ptr(frames), B, h, w, C.byref(c), ptr(o["masks"]), 0, ptr(o["dets"]), ptr(o["xyxy"]),
                                    ptr(o["counts"]), ptr(o["offsets"]), MAX_DET, cap, ptr(res["frame_i32"]), ptr(res["stitch_f64"]),
                                    ptr(res["stitch_i32"]), P(host_sel.ctypes.data), ptr(dev_sel), n_sel, 16384, ptr(pout["frames"]),
                                    ptr(pout["status"]), ptr(ws), ws.numel(), stream())
        assert rc == 0, rc
    measure(), draw()
    torch.cuda.synchronize()
    for k in KEYS:
        same(pres[k], res[k], ("parent", k))
    same(pout["frames"], out["frames"], "parent picture")
    return measure, draw


def uniform_part(eng, iters, parent_lib):
    B, (h, w) = 64, SIZES[0]
    o = output_set([(h, w)] * B, False)
    cap = o["masks"].shape[0]
    cp = vti_amd.CheckerParams(*CALIBS[0])
    res = eng.measure_checker(o, cp, h, w)
    frames = torch.from_numpy(frames_u8(B, h, w, 0)).cuda()
    sel = list(range(B))
    out = eng.annotate_checker(frames, o, res, cp, sel)
    print(f"2. the one-struct calls through the C ABI, B={B} frames {w}x{h}, letterbox masks, {N_INST} instances per frame, all selected")
    names = ("vti_measure_checker", "vti_annotate_checker")
    host_sel = np.arange(B, dtype=np.int32)
    args = (eng, o, res, frames, out, cp, B, h, w, cap, B, torch.from_numpy(host_sel).cuda(), host_sel)
    # each set of calls has a context, a scratch and result buffers of its own; "here again" is this build a second time, which
    # shows what two sets of buffers alone differ by
    sets = {"parent": dict(zip(names, raw_calls(parent_lib, *args)))} if parent_lib else {}
    sets["here"] = dict(zip(names, raw_calls(vti_amd.LIB_PATH, *args)))
    sets["here again"] = dict(zip(names, raw_calls(vti_amd.LIB_PATH, *args)))
    if parent_lib:
        print("   the parent build's results equal this build's, word for word and byte for byte")
    for name in names:
        for calls in sets.values():
            timed(calls[name], 5)
        for run in range(2):                    # parent, here, here again, parent, here, here again
            for who, calls in sets.items():
                print(f"  run {run}  {who:10s} {name:22s} {timed(calls[name], iters) * 1e3:9.1f} us/call")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--part", type=int, default=0, choices=(0, 1, 2))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("checker_rig_bench needs the GPU")
    eng = vti_amd.Engine("n", 2, H=MH, W=MW, max_batch=64, dtype="fp16")
    if a.part in (0, 1):
        rig_part(eng, a.iters)
    if a.part in (0, 2):
        uniform_part(eng, a.iters, a.parent_lib)


if __name__ == "__main__":
    main()
