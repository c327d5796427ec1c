"""vti_annotate_frames_native and vti_annotate_checker_frames_native next to the work-around they replace.  64 frames x 50 instances
(a fabric, a fabric with an empty mask, 48 stitches: tools/checker_rig_bench.py's scene), 16 frames of each of four sizes, four
cameras, a 736 x 960 canvas, the ragged frame-size rows of vti_masks_native_frames, every frame selected; device events after
warm-up, the calls of a comparison interleaved in groups of 10, two runs.
    python3 tools/annotate_native_frames_bench.py [--iters 50]
The work-around a caller had: the batch regrouped by frame size -- per group the frames gathered from the flat frame buffer into a
dense [n, H0, W0, 3] batch, the mask runs into a uniform [n * instances, H0, row_bytes] buffer, the rows of dets, xyxy, counts and of
the measurement gathered with them -- and one vti_annotate(native = 1) (checker: vti_annotate_checker_cameras(native = 1)) per group.
It is timed twice: with the regrouping (what every batch costs), and the calls alone on buffers regrouped beforehand.  The pictures
are compared first, byte for byte.  Reads nothing but the package and the scene helpers of the tests."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch

import vti_amd
from checker_rig_bench import MAX_DET, MH, MW, N_INST, SIZES, interleave, output_set, same, timed
from gpu_util import frames_u8
from test_gpu_measure_cameras import CALIBS


def family(eng, checker):
    if checker:
        plist = [vti_amd.CheckerParams(*CALIBS[c % 2], min_stitches=3 - c // 2, envelope_neighborhood=3 + c) for c in range(4)]
        return eng.pack_checker_cameras(plist, "cuda"), eng.measure_checker, eng.annotate_checker, "vti_annotate_checker_frames_native", \
            "vti_annotate_checker_cameras(native=1)"
    plist = [vti_amd.MeasureParams(*CALIBS[c % 2], roi_enabled=bool(c % 2), roi=(5, 100, 1900, 1000), min_stitches=3 - c // 2) for c in range(4)]
    return eng.pack_cameras(plist, "cuda"), eng.measure, eng.annotate, "vti_annotate_frames_native", "vti_annotate(native=1)"


def run(eng, iters, checker):
    B = 64
    shapes = [SIZES[b % 4] for b in range(B)]
    cams = [(b // 4) % 4 for b in range(B)]
    table, measure, draw, name, uniform_name = family(eng, checker)
    idx = torch.tensor(cams, dtype=torch.int32, device="cuda")
    ft, at, total = eng.pack_frames(shapes, "cuda")
    o = output_set(shapes, True)
    o["native_shapes"] = tuple(ft.shapes)
    bases = o["mask_bases"].cpu().tolist()
    meas = {k: v.clone() for k, v in measure(o, table, cameras=idx, frames=ft, native=True).items()}
    pics = {hw: torch.from_numpy(frames_u8(1, *hw, 7)[0]).cuda() for hw in SIZES}
    buf = torch.zeros(total, dtype=torch.uint8, device="cuda")
    for b, hw in enumerate(shapes):
        buf[at[b]:at[b] + pics[hw].numel()] = pics[hw].reshape(-1)
    sel = list(range(B))
    out = draw(buf, o, meas, table, sel, cameras=idx, table=ft, native=True)
    ok = int((meas["frame_i32"][:, 0] == 0).sum())
    print(f"{name}: B={B}, {N_INST} instances per frame, sizes {SIZES}, 4 cameras, all selected; measure status 0 in {ok}/{B} frames, "
          f"{o['masks'].numel() / 2 ** 20:.0f} MiB of ragged rows")

    # the work-around's buffers, one set per size
    groups = {}
    for b in range(B):
        groups.setdefault(shapes[b], []).append(b)
    g = {}
    for hw, fr in groups.items():
        h, w = hw
        n, rb = len(fr), 8 * -(-w // 64)
        fi = torch.tensor(fr, device="cuda")
        g[hw] = dict(fr=fr, fi=fi, rows=(fi[:, None] * N_INST + torch.arange(N_INST, device="cuda")[None]).reshape(-1),
                     dense=torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda"),
                     set=dict(dets=torch.empty((n, MAX_DET, 38), device="cuda"), xyxy=torch.empty((n, MAX_DET, 4), device="cuda"),
                              counts=torch.empty(n, dtype=torch.int32, device="cuda"),
                              offsets=torch.arange(n + 1, dtype=torch.int32, device="cuda") * N_INST,
                              masks=torch.empty((n * N_INST, h, rb), dtype=torch.uint8, device="cuda")),
                     meas=dict(frame_i32=torch.empty((n, 6), dtype=torch.int32, device="cuda"),
                               stitch_f64=torch.empty((n * N_INST, 7), dtype=torch.float64, device="cuda"),
                               stitch_i32=torch.empty((n * N_INST, 2), dtype=torch.int32, device="cuda")),
                     cams=torch.empty(n, dtype=torch.int32, device="cuda"), sel=list(range(n)), out=None)

    def regroup():
        for (h, w), q in g.items():
            slot = N_INST * h * q["set"]["masks"].shape[2]
            flat_masks = q["set"]["masks"].view(-1)
            for k, b in enumerate(q["fr"]):
                q["dense"][k].view(-1).copy_(buf[at[b]:at[b] + 3 * h * w])
                flat_masks[k * slot:(k + 1) * slot].copy_(o["masks"][bases[b]:bases[b + 1]])
            for key in ("dets", "xyxy", "counts"):
                torch.index_select(o[key], 0, q["fi"], out=q["set"][key])
            torch.index_select(meas["frame_i32"], 0, q["fi"], out=q["meas"]["frame_i32"])
            torch.index_select(meas["stitch_f64"], 0, q["rows"], out=q["meas"]["stitch_f64"])
            torch.index_select(meas["stitch_i32"], 0, q["rows"], out=q["meas"]["stitch_i32"])
            torch.index_select(idx, 0, q["fi"], out=q["cams"])

    def calls():
        for (h, w), q in g.items():
            q["out"] = draw(q["dense"], q["set"], q["meas"], table, q["sel"], native=True, cameras=q["cams"], result=q["out"])

    def work_around():
        regroup()
        calls()

    def ragged():
        draw(buf, o, meas, table, sel, cameras=idx, table=ft, native=True, result=out)

    work_around()
    ragged()
    torch.cuda.synchronize()
    for (h, w), q in g.items():
        for k, b in enumerate(q["fr"]):
            same(out["buf"][out["byte_offsets"][b]:out["byte_offsets"][b] + 3 * h * w], q["out"]["frames"][k].reshape(-1), ("picture", b))
        assert int(q["out"]["status"].sum()) == 0
    drawn = sum(int((out["buf"][out["byte_offsets"][b]:out["byte_offsets"][b] + pics[shapes[b]].numel()] != pics[shapes[b]].reshape(-1)).any())
                for b in range(B))
    print(f" the pictures equal those of the {len(g)} uniform calls byte for byte; {drawn}/{B} frames drawn on, outline skipped in "
          f"{int(out['status'].sum())}")
    timed(work_around, 3), timed(calls, 3), timed(ragged, 3)
    interleave({f"{len(g)} x (regroup + {uniform_name})": work_around, f"{len(g)} x {uniform_name}, regrouped beforehand": calls, name: ragged},
               iters, B)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--family", default="both", choices=("both", "annotate", "checker"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("annotate_native_frames_bench needs the GPU")
    eng = vti_amd.Engine("n", 2, H=MH, W=MW, max_batch=64, dtype="fp16")
    for checker in (False, True):
        if a.family in ("both", "checker" if checker else "annotate"):
            run(eng, a.iters, checker)


if __name__ == "__main__":
    main()
