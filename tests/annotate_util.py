"""Scenes and helpers shared by tests/test_annotate.py (CPU: what the scenes exercise) and tests/test_gpu_annotate.py (GPU: the
device against the restatement on the same scenes).  TEST INFRASTRUCTURE (not collected: no test_ prefix)."""
import numpy as np

import measure_ref as mr
from test_gpu_measure import DH, DW, MAX_DET, MODES, SETTINGS, _fabric, _stitch, pack, render, scenes
from test_oracle_geometry import load_calib

CALIB = load_calib()
SETTING_NAMES = ("kmeans", "nb64_iters0")          # two entries of test_gpu_measure.SETTINGS, the second with drop_empty
MAX_POINTS = 16384                                   # the outline room the parity tests give every frame
SMALL_MAX_POINTS = 700                               # the status test's: below the jagged scene's outline, above its neighbours'


def roi_for(h, w, k=0):
    """Camera k's ROI on an h x w frame: config.py's (10, 300, 1270, 760) scaled, and three others."""
    sx, sy = w / DW, h / DH
    base = [(10, 300, 1270, 760), (200, 250, 1100, 720), (0, 0, 1279, 959), (300, 400, 900, 700)][k]
    return (int(base[0] * sx), int(base[1] * sy), int(base[2] * sx), int(base[3] * sy))


def settings_for(name, h, w, k=0):
    return dict(SETTINGS[name], roi=roi_for(h, w, k))


def jagged_scenes():
    """Three frames for the status test: the middle one's fabric is a comb (one tooth per 4 px: ~4 vertices each), its neighbours'
    are plain; all have a row of stitches."""
    def row():
        return [_stitch(150 + 100 * k, 630) for k in range(10)]
    plain = [_fabric(60, 300, 1220, 700, bottom=680, amp=0.0)]
    comb = [_fabric(60, 300, 1220, 640, bottom=630, amp=0.0)] + [_fabric(64 + 4 * k, 600, 66 + 4 * k, 700, bottom=690, amp=0.0)
                                                                 for k in range(190)]
    return [plain + row(), comb + row(), plain + row()]


def host_batch(frames, h, w, mh, mw, native, dead=0, seed=1):
    """test_gpu_measure.build_batch on the host: -> (arrays dict(dets, xyxy, counts, offsets, masks), per frame (cls, xyxy, masks),
    offsets, capacity).  The last `dead` slots are past the capacity."""
    rng = np.random.default_rng(seed)
    B = len(frames)
    counts = np.array([len(f) for f in frames], np.int32)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    cap = int(offsets[-1]) - dead
    dets = np.zeros((B, MAX_DET, 38), np.float32)
    xyxy = np.zeros((B, MAX_DET, 4), np.float32)
    rb = 8 * -(-w // 64) if native else mw // 8
    masks = np.full((max(cap, 1), mh, rb), 0xFF, np.uint8)
    ref = []
    for b, insts in enumerate(frames):
        cls, boxes, ms = [], [], []
        for i, inst in enumerate(insts):
            m, fbox, mbox = render(inst, h, w, mh, mw, rng)
            dets[b, i, :4] = mbox
            dets[b, i, 4] = 0.9 - 0.001 * i
            dets[b, i, 5] = inst["cls"]
            dets[b, i, 6:] = rng.standard_normal(32)
            xyxy[b, i] = fbox
            s = offsets[b] + i
            if s < cap:
                masks[s] = pack(m, native, w)
            cls.append(inst["cls"])
            boxes.append(fbox)
            ms.append(m if s < cap else None)
        ref.append((np.array(cls), np.array(boxes, np.float32).reshape(-1, 4), ms))
    return dict(dets=dets, xyxy=xyxy, counts=counts, offsets=offsets, masks=masks[:cap]), ref, offsets, cap


def ref_rows(h, w, cls, boxes, ms, settings):
    """vti_measure's outputs for one frame as the restatement in measure_ref.py gives them: the `rows` of annotate.display_list and
    annotate.text_items (CPU tests only: the GPU tests take the rows the device wrote)."""
    rec, st = mr.measure_frame(h, w, cls, boxes, ms, CALIB, **settings)
    n = len(cls)
    flags, rank, f64 = np.zeros(n, np.int32), np.full(n, -1, np.int32), np.full((n, 7), np.nan)
    for j, s in enumerate(st):
        flags[s["i"]], rank[s["i"]] = s["flags"], j
        f64[s["i"]] = [s["cx"], s["cy"], s["left"], s["right"], s["width"], s["edge_y"], s["dist"]]
    return dict(status=rec["status"], n_stitch=rec["n_stitch"], n_fabric=rec["n_fabric"], n_dist=rec["n_dist"], n_width=rec["n_width"],
                flags=flags, rank=rank, f64=f64), rec


def device_rows(meas, b, offsets, cap, n):
    """The same dict from vti_measure's host-side outputs (frame_i32, stitch_f64, stitch_i32 as numpy) for frame b with n instances;
    instances past the capacity have no row (flags 0, rank -1)."""
    flags, rank, f64 = np.zeros(n, np.int32), np.full(n, -1, np.int32), np.full((n, 7), np.nan)
    lo = int(offsets[b])
    live = max(0, min(n, cap - lo))
    flags[:live] = meas["stitch_i32"][lo:lo + live, 0]
    rank[:live] = meas["stitch_i32"][lo:lo + live, 1]
    f64[:live] = meas["stitch_f64"][lo:lo + live]
    i32 = meas["frame_i32"][b]
    return dict(status=int(i32[0]), n_stitch=int(i32[1]), n_fabric=int(i32[2]), n_dist=int(i32[4]), n_width=int(i32[5]),
                flags=flags, rank=rank, f64=f64)
