"""-m gpu: the stitch-distance checker on a rig -- vti_measure_checker_cameras / _frames / _frames_native and
vti_annotate_checker_cameras / _frames.  Frame b of a rig call is compared word for word (64- and 32-bit words, NaN included) and
byte for byte with the one-struct call under that frame's camera at that frame's size, and with the restatement in
tests/checker_ref.py (counts and flags exactly, floats within test_gpu_checker.py's 1e-12 relative).  The output sets are made on the
host: a 96 x 128 canvas, 16 detections per frame, six frame sizes that cross every per-frame decision of the kernels (see SIZES).
`plan_facts` states, from the restatement alone, what the batches exercise; the tests assert it before they compare anything."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import checker_ref as cr
from gpu_util import frames_u8, need_gpu
from test_gpu_measure import _close, _engine, pack
from test_gpu_measure_cameras import CALIBS

pytestmark = pytest.mark.gpu

MH, MW, MAX_DET = 96, 128, 16
# the identity; a smaller frame; three 64-column groups, the last partial (native row 24 bytes); smaller than the canvas (mask rows
# without a frame row; native row 8 bytes); larger than the canvas (frame rows that share a mask row); a native row of one word pair
SIZES = [(96, 128), (72, 96), (61, 131), (37, 53), (150, 200), (40, 64)]
BAD = 9                                     # a camera index outside the table
# camera -> (calibration, settings): class ids swapped, and every other setting a row carries
CAMS = [(0, dict()),
        (1, dict(stitch_id=1, fabric_id=0, min_stitches=1, envelope_neighborhood=1, skip_cluster=True)),
        (0, dict(drop_empty=True, min_stitches=2, envelope_neighborhood=5, max_px_distance=14.0, kmeans_iters=2))]
KEYS = ("frame_f64", "frame_i32", "stitch_f64", "stitch_i32")


def settings(cam, drop=None):
    s = dict(CAMS[cam][1])
    if drop is not None:
        s["drop_empty"] = drop
    return s


def params(cam, drop=None):
    import vti_amd
    return vti_amd.CheckerParams(*CALIBS[CAMS[cam][0]], **settings(cam, drop))


# ---- scenes, in fractions of the frame ------------------------------------------------------------------------------------------
def _fab(x1, y1, x2, y2, kind="top"):
    return dict(role="fabric", box=(x1, y1, x2, y2), kind=kind)


def _st(x, y, w=0.09, h=0.08, kind="rect"):
    return dict(role="stitch", box=(x - w / 2, y - h / 2, x + w / 2, y + h / 2), kind=kind)


def scene(name):
    fab = _fab(0.04, 0.30, 0.96, 0.93)
    if name == "ok":        # a wavy top edge, a fabric instance whose mask is empty (its box joins the union), two rows of stitches
        return ([fab, _fab(0.50, 0.18, 0.90, 0.50, "empty")] + [_st(0.15 + 0.2 * k, 0.50 + 0.01 * (k % 2)) for k in range(4)] +
                [_st(0.25 + 0.2 * k, 0.78) for k in range(3)] + [_st(0.6, 0.12), _st(0.9, 0.6, kind="empty")])
    if name == "nofab":
        return [_st(0.2 + 0.2 * k, 0.5) for k in range(4)]
    if name == "nost":
        return [fab, _fab(0.3, 0.4, 0.9, 0.8)]
    if name == "single":
        return [_st(0.5, 0.6), fab]
    if name == "none":
        return []
    raise KeyError(name)


def many():
    """260 instances: the second 256-lane trip of the list loops."""
    return [_fab(0.04, 0.30, 0.96, 0.93)] + [_st(0.06 + 0.045 * (k % 20), 0.36 + 0.043 * (k // 20), 0.03, 0.035) for k in range(259)]


def plan_mixed():
    """(scene, frame size, camera): every size with an OK frame, every status, two or three cameras, an empty frame at the end."""
    S = SIZES
    return [("ok", S[0], 0), ("ok", S[1], 1), ("nofab", S[2], 0), ("ok", S[2], 2), ("ok", S[3], 0), ("nost", S[4], 1), ("ok", S[4], 0),
            ("ok", S[5], 1), ("ok", S[1], BAD), ("single", S[3], 1), ("ok", S[0], 2), ("none", S[5], 0)]


def plan_uniform(hw):
    return [(name, hw, cam) for name, _, cam in plan_mixed()]


def render(inst, h, w, mh, mw, rng):
    """One instance's mask at the mask resolution (mh x mw) for an h x w frame, its frame-px box and its mask-px box; the set pixels
    stay inside the box."""
    x1, y1, x2, y2 = inst["box"]
    fbox = (x1 * w + 0.3, y1 * h + 0.6, x2 * w + 0.3, y2 * h + 0.6)
    kx, ky = mw / w, mh / h
    mbox = (fbox[0] * kx, fbox[1] * ky, fbox[2] * kx, fbox[3] * ky)
    m = np.zeros((mh, mw), np.uint8)
    r0, r1 = max(0, int(np.ceil(mbox[1]))), min(mh, int(np.floor(mbox[3])))
    c0, c1 = max(0, int(np.ceil(mbox[0]))), min(mw, int(np.floor(mbox[2])))
    if inst["kind"] == "empty" or r1 <= r0 or c1 <= c0:
        return m, fbox, mbox
    if inst["kind"] == "top":
        cols = np.arange(c0, c1)
        top = r0 + 0.08 * mh * (1 + np.sin(cols / (0.03 * mw))) / 2
        for c, yt in zip(cols, top):
            m[min(int(yt), r1 - 1):r1, c] = 1
    else:
        m[r0:r1, c0:c1] = rng.uniform(size=(r1 - r0, c1 - c0)) < 0.7
        m[r0, c0] = 1
    return m, fbox, mbox


@functools.lru_cache(maxsize=None)
def host_set(plan, native, max_det=MAX_DET):
    """The output set of a predict on `plan`, hand-made and kept on the host: dets (canvas px), xyxy (frame px), counts, offsets, and
    per frame (cls, boxes, masks at the canvas size or, native, at the frame's own size)."""
    rng = np.random.default_rng(3)
    B = len(plan)
    insts = [many() if name == "many" else scene(name) for name, _, _ in plan]
    counts = np.array([len(x) for x in insts], np.int32)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    dets = np.zeros((B, max_det, 38), np.float32)
    xyxy = np.zeros((B, max_det, 4), np.float32)
    ref = []
    for b, (_, (h, w), cam) in enumerate(plan):
        ids = settings(cam if cam != BAD else 0)
        cls, ms = [], []
        for i, inst in enumerate(insts[b]):
            m, fbox, mbox = render(inst, h, w, *((h, w) if native else (MH, MW)), rng)
            c = ids.get("stitch_id", 0) if inst["role"] == "stitch" else ids.get("fabric_id", 1)
            dets[b, i, :4], dets[b, i, 4], dets[b, i, 5] = mbox, 0.9 - 0.001 * i, c
            dets[b, i, 6:] = rng.standard_normal(32)
            xyxy[b, i] = fbox
            cls.append(c)
            ms.append(m)
        ref.append((np.array(cls), xyxy[b, :len(cls)].copy(), ms))
    return dict(dets=dets, xyxy=xyxy, counts=counts, offsets=offsets), ref


def letterbox_masks(plan, max_det=MAX_DET):
    """u8 [total, MH, MW / 8]: the canvas-size bit masks of the plan's instances, frame-major."""
    _, ref = host_set(plan, False, max_det)
    return np.stack([pack(m, False, MW) for _, _, ms in ref for m in ms])


def native_masks(plan, hw, max_det=MAX_DET):
    """u8 [total, h, row bytes]: the frame-size rows of the instances of the frames of size hw; the other frames' slots are 0xFF."""
    _, ref = host_set(plan, True, max_det)
    h, w = hw
    out = [pack(m, True, w) if plan[b][1] == hw else np.full((h, 8 * -(-w // 64)), 0xFF, np.uint8)
           for b, (_, _, ms) in enumerate(ref) for m in ms]
    return np.stack(out)


def ragged_masks(plan):
    """(flat u8, bases i64 [B + 1]): every frame's slots at its own size, back to back, frame-major (vti_masks_native_frames)."""
    _, ref = host_set(plan, True)
    parts, bases = [], [0]
    for b, (_, _, ms) in enumerate(ref):
        w = plan[b][1][1]
        mine = [pack(m, True, w).ravel() for m in ms]
        parts += mine
        bases.append(bases[-1] + sum(p.size for p in mine))
    return np.concatenate(parts), np.array(bases, np.int64)


def dev_set(plan, native, masks, max_det=MAX_DET, **extra):
    arrays, _ = host_set(plan, native, max_det)
    out = {k: torch.from_numpy(v).cuda() for k, v in arrays.items()}
    out["masks"] = torch.from_numpy(masks).cuda()
    out.update(extra)
    return out


def reference(plan, native, live=None, drop=None, max_det=MAX_DET):
    """The restatement per frame at the frame's own size under its own camera (None for a bad camera).  live(b, i) -> False: the
    instance has no live slot (an empty mask that still has its box)."""
    _, ref = host_set(plan, native, max_det)
    out = []
    for b, ((cls, boxes, ms), (_, (h, w), cam)) in enumerate(zip(ref, plan)):
        if cam == BAD:
            out.append(None)
            continue
        ms = [m if live is None or live(b, i) else None for i, m in enumerate(ms)]
        out.append(cr.measure_frame(h, w, cls, boxes, ms, CALIBS[CAMS[cam][0]], **settings(cam, drop)))
    return out


def plan_facts(plan, exp, native):
    """What the batch exercises, from the restatement alone."""
    _, ref = host_set(plan, native)
    statuses = [3 if e is None else e[0]["status"] for e in exp]
    ok_sizes = {plan[b][1] for b, e in enumerate(exp) if e is not None and e[0]["status"] == cr.OK and e[0]["n_dist"] >= 1 and e[0]["n_width"] >= 1}
    box_branch = False
    for b, e in enumerate(exp):
        if e is None or e[0]["status"] != cr.OK or settings(plan[b][2]).get("drop_empty"):
            continue
        cls, _, ms = ref[b]
        fabric_id = settings(plan[b][2]).get("fabric_id", 1)
        box_branch |= any(c == fabric_id and not m.any() for c, m in zip(cls, ms))
    return statuses, ok_sizes, box_branch


def assert_facts(plan, exp, native, table=True):
    statuses, ok_sizes, box_branch = plan_facts(plan, exp, native)
    assert {cr.OK, cr.NO_FABRIC, cr.NO_STITCHES} <= set(statuses) and (not table or 3 in statuses), statuses
    assert ok_sizes == {hw for _, hw, _ in plan}, (ok_sizes, statuses)
    assert box_branch


def poisoned(B, rows):
    return dict(frame_f64=torch.full((B, 2), -7.0, dtype=torch.float64, device="cuda"),
                frame_i32=torch.full((B, 6), -7, dtype=torch.int32, device="cuda"),
                stitch_f64=torch.full((rows, 7), -7.0, dtype=torch.float64, device="cuda"),
                stitch_i32=torch.full((rows, 2), -7, dtype=torch.int32, device="cuda"))


def host(res):
    return {k: res[k].cpu().numpy() for k in KEYS}


def same_words(a, b, frame, lo, hi, what):
    """Frame `frame` and the slot rows [lo, hi) of two results, as raw 64- and 32-bit words."""
    assert a["frame_f64"][frame].tobytes() == b["frame_f64"][frame].tobytes(), (what, frame, a["frame_f64"][frame], b["frame_f64"][frame])
    assert a["frame_i32"][frame].tobytes() == b["frame_i32"][frame].tobytes(), (what, frame, a["frame_i32"][frame], b["frame_i32"][frame])
    assert a["stitch_f64"][lo:hi].tobytes() == b["stitch_f64"][lo:hi].tobytes(), (what, frame)
    assert a["stitch_i32"][lo:hi].tobytes() == b["stitch_i32"][lo:hi].tobytes(), (what, frame)


def check_ref(got, plan, exp, offsets, live_end=None):
    """`got` against the restatement: counts, flags and ranks exactly, floats 1e-12 relative, NaN where it has None; a bad camera's
    frame as the header states it.  live_end[b]: the frame's first slot without a row (default: every instance has one)."""
    for b, e in enumerate(exp):
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        end = hi if live_end is None else max(lo, min(hi, live_end[b]))
        if e is None:
            assert got["frame_i32"][b].tolist() == [3, 0, 0, 0, 0, 0] and np.isnan(got["frame_f64"][b]).all(), b
            assert (got["stitch_i32"][lo:end] == np.array([0, -1])).all() and np.isnan(got["stitch_f64"][lo:end]).all(), b
            continue
        rec, st = e
        want = [rec["status"], rec["n_stitch"], rec["n_fabric"], rec["n_selected"], rec["n_dist"], rec["n_width"]]
        assert got["frame_i32"][b].tolist() == want, (b, got["frame_i32"][b].tolist(), want)
        assert _close(got["frame_f64"][b, 0], rec["avg_dist"]) and _close(got["frame_f64"][b, 1], rec["avg_width"]), (b, got["frame_f64"][b], rec)
        rank = {s["i"]: (j, s) for j, s in enumerate(st)}
        for slot in range(lo, end):
            i = slot - lo
            if i not in rank:
                assert got["stitch_i32"][slot].tolist() == [0, -1] and np.isnan(got["stitch_f64"][slot]).all(), (b, i)
                continue
            j, s = rank[i]
            assert got["stitch_i32"][slot].tolist() == [s["flags"], j], (b, i, got["stitch_i32"][slot].tolist(), s["flags"], j)
            for k, key in enumerate(("cx", "cy", "left", "right", "width", "edge_y", "dist")):
                assert _close(got["stitch_f64"][slot, k], s[key]), (b, i, key, got["stitch_f64"][slot, k], s[key])
        assert (got["stitch_i32"][end:hi] == -7).all() and (got["stitch_f64"][end:hi] == -7.0).all(), b


def cam_index(plan):
    return torch.tensor([cam for _, _, cam in plan], dtype=torch.int32, device="cuda")


def test_the_plans_exercise_what_they_claim():
    """Host only: the conditions of the parity batches hold in the restatement, at every size and for both kinds of masks."""
    plan = tuple(plan_mixed())
    assert len({hw for _, hw, _ in plan}) == len(SIZES) and {cam for _, _, cam in plan} == {0, 1, 2, BAD}
    for native in (False, True):
        assert_facts(plan, reference(plan, native), native)
    for hw in (SIZES[2], SIZES[4]):
        for native in (False, True):
            p = tuple(plan_uniform(hw))
            assert_facts(p, reference(p, native), native)


# ---- 1. vti_measure_checker_cameras ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("native", [False, True], ids=["letterbox", "native"])
@pytest.mark.parametrize("hw", [SIZES[2], SIZES[4]], ids=["61x131", "150x200"])
def test_cameras_is_the_one_struct_call_per_camera_and_the_restatement(hw, native):
    need_gpu()
    eng = _engine(MH, MW, 16)
    h, w = hw
    plan = tuple(plan_uniform(hw))
    B = len(plan)
    exp = reference(plan, native)
    assert_facts(plan, exp, native)
    dev = dev_set(plan, native, native_masks(plan, hw) if native else letterbox_masks(plan))
    offsets = dev["offsets"].cpu().numpy()
    total = int(offsets[-1])
    table = eng.pack_checker_cameras([params(c) for c in range(len(CAMS))], "cuda")
    got = host(eng.measure_checker(dev, table, h, w, native=native, cameras=cam_index(plan), result=poisoned(B, total + 5)))
    assert (got["stitch_i32"][total:] == -7).all() and (got["stitch_f64"][total:] == -7.0).all()      # rows no slot owns
    for c in range(len(CAMS)):
        one = host(eng.measure_checker(dev, params(c), h, w, native=native, result=poisoned(B, total + 5)))
        for b in range(B):
            if plan[b][2] == c:
                same_words(got, one, b, offsets[b], offsets[b + 1], f"camera {c}")
    check_ref(got, plan, exp, offsets)
    bad = [b for b in range(B) if plan[b][2] == BAD]
    assert bad and offsets[bad[0] + 1] > offsets[bad[0]]
    # the list-of-params and host-sequence forms are the same call
    again = host(eng.measure_checker(dev, [params(c) for c in range(len(CAMS))], h, w, native=native,
                                     cameras=[min(cam, 2) for _, _, cam in plan], result=poisoned(B, total + 5)))
    for b in range(B):
        if plan[b][2] != BAD:
            same_words(got, again, b, offsets[b], offsets[b + 1], "host sequence")


# ---- 2. vti_measure_checker_frames ----------------------------------------------------------------------------------------------
def test_frames_is_cameras_at_every_frames_size_from_the_same_slots():
    need_gpu()
    eng = _engine(MH, MW, 16)
    plan = tuple(plan_mixed())
    B = len(plan)
    shapes = [hw for _, hw, _ in plan]
    exp = reference(plan, False)
    assert_facts(plan, exp, False)
    dev = dev_set(plan, False, letterbox_masks(plan))
    offsets = dev["offsets"].cpu().numpy()
    total = int(offsets[-1])
    ft, _, _ = eng.pack_frames(shapes, "cuda")
    table = eng.pack_checker_cameras([params(c) for c in range(len(CAMS))], "cuda")
    idx = cam_index(plan)
    eng.measure_checker(dev, table, cameras=idx, frames=ft, result=poisoned(B, total + 5))      # sizes the scratch ...
    eng._measure_ws.fill_(0x55)                  # ... whose envelope columns beyond a narrow frame's W0 must never reach a result
    got = host(eng.measure_checker(dev, table, cameras=idx, frames=ft, result=poisoned(B, total + 5)))
    assert (got["stitch_i32"][total:] == -7).all() and (got["stitch_f64"][total:] == -7.0).all()
    for h, w in sorted(set(shapes)):
        eng._measure_ws.fill_(0x55)
        uni = host(eng.measure_checker(dev, table, h, w, cameras=idx, result=poisoned(B, total + 5)))
        for b in range(B):
            if shapes[b] == (h, w):
                same_words(got, uni, b, offsets[b], offsets[b + 1], f"{h}x{w}")
    check_ref(got, plan, exp, offsets)
    # one params for every frame: the table form without `cameras`
    one = host(eng.measure_checker(dev, params(0), frames=ft, result=poisoned(B, total + 5)))
    for b in range(B):
        if plan[b][2] == 0:
            same_words(got, one, b, offsets[b], offsets[b + 1], "one params")
    with pytest.raises(ValueError, match="mask_bases"):
        eng.measure_checker(dev, table, cameras=idx, frames=ft, native=True)


# ---- 3. vti_measure_checker_frames_native ---------------------------------------------------------------------------------------
def _ragged_set(eng, plan, ft):
    flat, bases = ragged_masks(plan)
    return dev_set(plan, True, flat, mask_bases=torch.from_numpy(bases).cuda(), native_shapes=tuple(ft.shapes)), bases


def test_frames_native_is_the_uniform_native_call_per_frame():
    need_gpu()
    eng = _engine(MH, MW, 16)
    plan = tuple(plan_mixed())
    B = len(plan)
    shapes = [hw for _, hw, _ in plan]
    exp = reference(plan, True)
    assert_facts(plan, exp, True)
    ft, _, _ = eng.pack_frames(shapes, "cuda")
    dev, bases = _ragged_set(eng, plan, ft)
    offsets = dev["offsets"].cpu().numpy()
    total = int(offsets[-1])
    assert {8 * -(-w // 64) for _, w in shapes} >= {8, 16, 24, 32}
    table = eng.pack_checker_cameras([params(c) for c in range(len(CAMS))], "cuda")
    idx = cam_index(plan)
    got = host(eng.measure_checker(dev, table, cameras=idx, frames=ft, native=True, result=poisoned(B, B * MAX_DET)))
    assert (got["stitch_i32"][total:] == -7).all() and (got["stitch_f64"][total:] == -7.0).all()
    for hw in sorted(set(shapes)):
        uni_dev = dev_set(plan, True, native_masks(plan, hw))
        uni = host(eng.measure_checker(uni_dev, table, *hw, native=True, cameras=idx, result=poisoned(B, total + 5)))
        for b in range(B):
            if shapes[b] == hw:
                same_words(got, uni, b, offsets[b], offsets[b + 1], hw)
    check_ref(got, plan, exp, offsets)


def test_frames_native_with_the_bytes_cut_keeps_the_boxes_of_what_did_not_fit():
    """capacity_bytes ends after the first slot of frame 6: the rest of that frame and every later frame are empty masks that still
    have their boxes (drop_empty = 0 in every camera): the fabric's filled rectangle, the stitch's int-box centroid."""
    need_gpu()
    eng = _engine(MH, MW, 16)
    plan = tuple(plan_mixed())
    B = len(plan)
    shapes = [hw for _, hw, _ in plan]
    ft, _, _ = eng.pack_frames(shapes, "cuda")
    dev, bases = _ragged_set(eng, plan, ft)
    offsets = dev["offsets"].cpu().numpy()
    total = int(offsets[-1])
    k, keep = 6, 1
    hk, wk = shapes[k]
    cut_bytes = int(bases[k]) + keep * hk * 8 * -(-wk // 64)
    cut_slot = int(offsets[k]) + keep
    live = lambda b, i: offsets[b] + i < cut_slot
    exp = reference(plan, True, live=live, drop=False)
    # from the restatement alone: frames after the cut are measured from boxes only, and still give distances and widths
    later = [e[0] for b, e in enumerate(exp) if e is not None and b > k]
    assert exp[k][0]["status"] == cr.OK and exp[k][0]["n_fabric"] == 2
    assert any(r["status"] == cr.OK and r["n_dist"] >= 1 and r["n_width"] >= 1 and r["n_fabric"] >= 1 for r in later), later
    assert all(not (s["flags"] & cr.MASK) for b, e in enumerate(exp) if e is not None and b > k for s in e[1])
    full = reference(plan, True, drop=False)
    assert any(a is not None and a[0] != b[0] for a, b in zip(exp, full))               # the cut changes records
    table = eng.pack_checker_cameras([params(c, drop=False) for c in range(len(CAMS))], "cuda")
    idx = cam_index(plan)
    cut = dict(dev, masks=dev["masks"][:cut_bytes])
    got = host(eng.measure_checker(cut, table, cameras=idx, frames=ft, native=True, result=poisoned(B, B * MAX_DET)))
    live_end = [cut_slot] * B
    check_ref(got, plan, exp, offsets, live_end)
    for hw in sorted(set(shapes)):
        uni_dev = dev_set(plan, True, native_masks(plan, hw)[:cut_slot])                 # the uniform call with the capacity cut there
        uni = host(eng.measure_checker(uni_dev, table, *hw, native=True, cameras=idx, result=poisoned(B, B * MAX_DET)))
        for b in range(B):
            if shapes[b] == hw:
                same_words(got, uni, b, offsets[b], offsets[b + 1], hw)


# ---- 4. more instances than one trip of the list loops ---------------------------------------------------------------------------
@pytest.mark.parametrize("native", [False, True], ids=["letterbox", "native"])
def test_260_instances_take_the_second_trip_of_the_list_loops(native):
    need_gpu()
    eng = _engine(MH, MW, 16)
    hw = SIZES[1]
    plan = (("many", hw, 0), ("ok", hw, 1))
    max_det = 300
    exp = reference(plan, native, max_det=max_det)
    assert exp[0][0]["status"] == cr.OK and exp[0][0]["n_stitch"] == 259 and exp[0][0]["n_dist"] >= 3 and exp[0][0]["n_width"] >= 3
    assert any(s["i"] >= 256 for s in exp[0][1])
    masks = native_masks(plan, hw, max_det) if native else letterbox_masks(plan, max_det)
    dev = dev_set(plan, native, masks, max_det)
    offsets = dev["offsets"].cpu().numpy()
    total = int(offsets[-1])
    assert total == 260 + len(scene("ok"))
    table = eng.pack_checker_cameras([params(0), params(1)], "cuda")
    idx = cam_index(plan)
    got = host(eng.measure_checker(dev, table, *hw, native=native, cameras=idx, result=poisoned(2, total + 5)))
    for c in range(2):
        one = host(eng.measure_checker(dev, params(c), *hw, native=native, result=poisoned(2, total + 5)))
        same_words(got, one, c, offsets[c], offsets[c + 1], f"camera {c}")
    check_ref(got, plan, exp, offsets)
    ft, _, _ = eng.pack_frames([hw, hw], "cuda")
    if native:
        flat = np.concatenate([m.ravel() for m in masks])
        slot = masks[0].size
        bases = torch.tensor([0, 260 * slot, total * slot], dtype=torch.int64, device="cuda")
        dev = dict(dev, masks=torch.from_numpy(flat).cuda(), mask_bases=bases, native_shapes=tuple(ft.shapes))
    tab = host(eng.measure_checker(dev, table, cameras=idx, frames=ft, native=native, result=poisoned(2, 2 * max_det)))
    for b in range(2):
        same_words(got, tab, b, offsets[b], offsets[b + 1], "frames form")


# ---- 5. the pictures ------------------------------------------------------------------------------------------------------------
POISON = 0xA5


def _params_list(drop=None):
    return [params(c, drop) for c in range(len(CAMS))]


@pytest.mark.parametrize("native", [False, True], ids=["letterbox", "native"])
def test_the_cameras_picture_is_the_one_struct_picture_per_camera(native):
    need_gpu()
    from vti_amd import annotate as A
    eng = _engine(MH, MW, 16)
    hw = SIZES[2]
    h, w = hw
    plan = tuple(plan_uniform(hw))
    B = len(plan)
    dev = dev_set(plan, native, native_masks(plan, hw) if native else letterbox_masks(plan))
    table = eng.pack_checker_cameras(_params_list(), "cuda")
    idx = cam_index(plan)
    meas = eng.measure_checker(dev, table, h, w, native=native, cameras=idx)
    statuses = meas["frame_i32"][:, 0].cpu().tolist()
    assert {0, 1, 2, 3} <= set(statuses)
    frames = frames_u8(B, h, w, 5)
    dframes = torch.from_numpy(frames).cuda()
    sel = list(range(B))
    flat = torch.full((B * h * w * 3 + 4096,), POISON, dtype=torch.uint8, device="cuda")
    res = dict(frames=flat[:B * h * w * 3].view(B, h, w, 3), status=torch.full((B,), -7, dtype=torch.int32, device="cuda"))
    eng.annotate_checker(dframes, dev, meas, table, sel, native=native, cameras=idx)       # sizes the scratch, which is then poisoned
    eng._annotate_ws.fill_(POISON)
    out = eng.annotate_checker(dframes, dev, meas, table, sel, native=native, cameras=idx, result=res)
    got = out["frames"].cpu().numpy()
    assert (flat[B * h * w * 3:] == POISON).all() and out["status"].cpu().tolist() == [0] * B
    assert torch.equal(dframes, torch.from_numpy(frames).cuda())
    drawn = 0
    for c in range(len(CAMS)):
        mine = [b for b in range(B) if plan[b][2] == c]
        one = eng.annotate_checker(dframes, dev, meas, params(c), mine, native=native)["frames"].cpu().numpy()
        for k, b in enumerate(mine):
            assert np.array_equal(got[b], one[k]), (c, b, int((got[b] != one[k]).any(axis=-1).sum()))
            drawn += int((got[b] != frames[b]).any())
    assert drawn >= 6
    for b in range(B):
        if plan[b][2] == BAD:
            assert np.array_equal(got[b], frames[b])                                     # a bad camera: the plain copy
    # a NULL index array: row 0 for every frame
    zero = eng.annotate_checker(dframes, dev, meas, table, [0, 4], native=native)["frames"].cpu().numpy()
    assert np.array_equal(zero[0], got[0]) and np.array_equal(zero[1], got[4])
    # one picture against the restatement
    import annotate_util as U
    _, ref = host_set(plan, native)
    mh = host(meas)
    offsets = dev["offsets"].cpu().numpy()
    b = 0
    cls, boxes, ms = ref[b]
    rows = U.device_rows(mh, b, offsets, int(offsets[-1]), len(cls))
    want = A.rasterise(frames[b], A.checker_display_list(h, w, cls, boxes, ms, rows, params(plan[b][2]), max_points=U.MAX_POINTS))
    assert np.array_equal(got[b], want), int((got[b] != want).any(axis=-1).sum())
    assert (want != frames[b]).any()


def test_the_frames_pictures_are_the_cameras_pictures_at_every_size():
    need_gpu()
    eng = _engine(MH, MW, 16)
    plan = tuple(plan_mixed())
    B = len(plan)
    shapes = [hw for _, hw, _ in plan]
    dev = dev_set(plan, False, letterbox_masks(plan))
    ft, at, total_bytes = eng.pack_frames(shapes, "cuda")
    table = eng.pack_checker_cameras(_params_list(), "cuda")
    idx = cam_index(plan)
    meas = eng.measure_checker(dev, table, cameras=idx, frames=ft)
    pics = [frames_u8(1, h, w, 20 + b)[0] for b, (h, w) in enumerate(shapes)]
    flat_in = np.full(total_bytes + 64, 0x3C, np.uint8)
    for b, p in enumerate(pics):
        flat_in[at[b]:at[b] + p.size] = p.ravel()
    assert any(3 * h * w % 16 for h, w in shapes)                                        # there are gaps between the frames
    buf = torch.from_numpy(flat_in[:total_bytes]).cuda()
    before = buf.clone()
    sel = [6, 1, 8, 4, 4, 11, 3, 0, 7, 9, 2, 5, 10, 6]                                   # any order, duplicates, the bad camera's frame
    assert set(sel) == set(range(B))
    eng.annotate_checker(buf, dev, meas, table, sel, cameras=idx, table=ft)              # sizes the scratch and the out table
    eng._annotate_ws.fill_(POISON)
    out_table = eng._out_table(tuple(shapes[b] for b in sel), buf.device)
    guard = torch.full((out_table.total_bytes + 4096,), POISON, dtype=torch.uint8, device="cuda")
    out = eng.annotate_checker(buf, dev, meas, table, sel, cameras=idx, table=ft, result=dict(buf=guard))
    assert out["buf"] is guard and out["shapes"] == [shapes[b] for b in sel] and out["status"].cpu().tolist() == [0] * len(sel)
    assert torch.equal(buf, before)                                                      # dev_frames is read only
    got = guard.cpu().numpy()
    covered = np.zeros(got.size, bool)
    for (h, w), o in zip(out["shapes"], out["byte_offsets"]):
        covered[o:o + 3 * h * w] = True
    assert (~covered[:out_table.total_bytes]).any() and (got[~covered] == POISON).all()  # the gaps and the bytes past the last picture
    drawn = 0
    for hw in sorted(set(shapes)):
        h, w = hw
        mine = [b for b in range(B) if shapes[b] == hw]
        uni = np.zeros((B, h, w, 3), np.uint8)
        for b in mine:
            uni[b] = pics[b]
        # the rows of the frames of this size are those of the cameras call at this size (test 2), so `meas` serves both
        one = eng.annotate_checker(torch.from_numpy(uni).cuda(), dev, meas, table, mine, cameras=idx)["frames"].cpu().numpy()
        for k, b in enumerate(sel):
            if shapes[b] != hw:
                continue
            o = out["byte_offsets"][k]
            pic = got[o:o + 3 * h * w].reshape(h, w, 3)
            want = one[mine.index(b)]
            assert np.array_equal(pic, want), (k, b, hw, int((pic != want).any(axis=-1).sum()))
            if plan[b][2] == BAD:
                assert np.array_equal(pic, pics[b])
            else:
                drawn += int((pic != pics[b]).any())
    assert drawn >= 8
    # the result feeds encode_jpeg(table=) unchanged
    from vti_amd import jpeg
    data, off = eng.encode_jpeg(out["buf"], quality=90, table=out["table"])
    off = off.cpu().numpy()
    k = 3
    h, w = out["shapes"][k]
    o = out["byte_offsets"][k]
    assert data[int(off[k]):int(off[k + 1])].cpu().numpy().tobytes() == jpeg.encode(got[o:o + 3 * h * w].reshape(h, w, 3), 90)
    with pytest.raises(ValueError, match="native"):
        eng.annotate_checker(buf, dev, meas, table, sel, cameras=idx, table=ft, native=True)


# ---- 6. end to end ---------------------------------------------------------------------------------------------------------------
def _strip(rec, *more):
    return {k: v for k, v in rec.items() if k not in ("timestamp",) + more}


@pytest.mark.parametrize("retina", [False, True], ids=["annotate_encode", "retina_masks"])
def test_multi_camera_checker_equals_one_checker_per_camera_over_predict(retina):
    """A mixed list over a real predict.  The frames are square, so every size is letterboxed onto the canvas the uniform call of
    that size uses too (imgsz x imgsz): the per-camera StitchDistanceChecker runs on the uniform sub-batches see the same network
    input, and records, text and files must be equal."""
    need_gpu()
    import vti_amd
    model = vti_amd.YOLO(None, scale="n", nc=2, seed=3, cls_bias=-1.0)
    base = vti_amd.CheckerParams(*CALIBS[0])
    cams_p = [base, dataclasses.replace(vti_amd.CheckerParams(*CALIBS[1]), stitch_id=1, fabric_id=0, min_stitches=1)]
    sides = [960, 640, 960, 640, 480, 480]
    cams = [0, 1, 0, 1, 0, 1]
    kw = dict(conf=0.20, iou=0.45, max_det=200, imgsz=640)
    mc = vti_amd.MultiCameraChecker(model, cams_p, frame_buffer=8)
    singles = [vti_amd.StitchDistanceChecker(model, p, frame_buffer=8) for p in cams_p]
    seen = 0
    for seed in (0, 1):
        frames = [frames_u8(1, s, s, 10 * seed + k)[0] for k, s in enumerate(sides)]
        if retina:
            records = mc.process_frames(frames, cams, retina_masks=True, mixed=True, **kw)
            annotated = None
        else:
            annotated, records = mc.process_frames(frames, cams, annotate="all", encode="jpeg", mixed=True, **kw)
            assert [a[0] for a in annotated] == list(range(len(frames)))
        assert [r["camera"] for r in records] == cams
        for c in range(2):
            mine = [b for b in range(len(frames)) if cams[b] == c]
            runs = []                                                # consecutive frames of one size: a uniform sub-batch
            for b in mine:
                if runs and sides[runs[-1][-1]] == sides[b]:
                    runs[-1].append(b)
                else:
                    runs.append([b])
            for run in runs:
                sub = np.stack([frames[b] for b in run])
                if retina:
                    want = singles[c].process_frames(sub, retina_masks=True, **kw)
                else:
                    want_a, want = singles[c].process_frames(sub, annotate="all", encode="jpeg", **kw)
                for k, b in enumerate(run):
                    assert _strip(records[b], "camera") == _strip(want[k]), (seed, b, records[b], want[k])
                    seen += records[b]["edge_distance_mm"] is not None
                    if not retina:
                        assert annotated[b][1] == want_a[k][1], (seed, b)                  # the JPEG file
                        assert annotated[b][2] == want_a[k][2], (seed, b)                  # the text items
    print("frames with a distance:", seen)
    assert seen >= 2                                 # the deques are in use, or the carry-over between batches is not tested
    with pytest.raises(ValueError, match="annotate needs frames of one size"):
        mc.process_frames(frames, cams, annotate="all", **kw)
