"""-m gpu: vti_measure_checker (the stitch-distance checker's measurement on the device) against the restatement in
tests/checker_ref.py.  Statuses, counts, flags and ranks exactly; floats within 1e-12 relative (test_gpu_measure.py's rule), NaN
exactly where the restatement has None.  The scenes are test_gpu_measure.py's twelve plus four drawn for the checker: a fabric with
a wavy TOP edge, a row of stitches that straddles that edge, fabric instances with empty masks, and a dead fabric slot."""
import functools

import numpy as np
import pytest
import torch

import checker_ref as cr
import test_gpu_measure as tg
from gpu_util import frames_u8, need_gpu

pytestmark = pytest.mark.gpu

CALIB, MAX_DET, DW, DH = tg.CALIB, tg.MAX_DET, tg.DW, tg.DH
SENTINEL_F, SENTINEL_I = -12345.5, -777


def _params(calib=CALIB, **kw):
    import vti_amd
    return vti_amd.CheckerParams(*calib, **kw)


# ---- scenes --------------------------------------------------------------------------------------------------------------
def _fabric_top(x1, y1, x2, y2, top, amp=30.0):
    """A fabric whose mask runs from a wavy top edge (top .. top + amp) down to the bottom of its box."""
    return dict(cls=1, box=(x1, y1, x2, y2), kind="fabric_top", top=top, amp=amp)


def _empty_fabric(x1, y1, x2, y2):
    return dict(cls=1, box=(x1, y1, x2, y2), kind="empty")


def scenes():
    rng = np.random.default_rng(7)
    wavy = _fabric_top(60, 290, 1220, 700, top=300)
    below = [wavy] + tg._row(380, rng=rng) + tg._row(520, x0=170, rng=rng)            # the upper row lies 50-80 px below the edge
    straddle = tg._row(316, n=11, x0=120, rng=rng) + [wavy]                           # one row across the wave: some above the edge
    boxes = ([_fabric_top(60, 290, 700, 700, top=300), _empty_fabric(650.6, 250.4, 1220.2, 700.9)] + tg._row(360, rng=rng) +
             [_empty_fabric(-40.5, 100.2, 30.7, 2000.0), _empty_fabric(1300.0, 10.0, 1400.0, 50.0)])
    dead = tg._row(400, n=6, rng=rng) + [_empty_fabric(100.3, 350.2, 900.8, 600.1), tg._stitch(950, 300), tg._stitch(1000, 420),
                                         tg._fabric(60, 330, 1220, 700, bottom=680)]      # build_batch(dead=3): the last three have no slot
    return tg.scenes() + [below, straddle, boxes, dead]


I_BELOW, I_STRADDLE, I_BOXES, I_DEAD = 12, 13, 14, 15


def render(inst, h, w, mh, mw, rng):
    if inst["kind"] != "fabric_top":
        return tg.render(inst, h, w, mh, mw, rng)
    m, fbox, mbox = tg.render(dict(inst, kind="empty"), h, w, mh, mw, rng)
    sx, sy = w / DW, h / DH
    kx, ky = mw / w, mh / h
    r0, r1 = max(0, int(np.ceil(mbox[1]))), min(mh, int(np.floor(mbox[3])))
    c0, c1 = max(0, int(np.ceil(mbox[0]))), min(mw, int(np.floor(mbox[2])))
    cols = np.arange(c0, c1)
    top = inst["top"] * sy * ky + inst["amp"] * sy * ky * (1 + np.sin(cols / (37.0 * kx * sx + 1e-9))) / 2
    for c, yt in zip(cols, top):
        m[min(max(r0, int(yt)), r1 - 1):r1, c] = 1
    return m, fbox, mbox


@functools.lru_cache(maxsize=None)
def host_batch(h, w, mh, mw, native, dead):
    """test_gpu_measure.build_batch with this file's render, kept on the host: (arrays, per-frame restatement inputs, offsets, cap).
    dead > 0: the last `dead` slots lie past the capacity; dead < 0: -dead slots of 0xFF past the live count."""
    rng = np.random.default_rng(1)
    frames = scenes()
    B = len(frames)
    counts = np.array([len(f) for f in frames], np.int32)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    cap = int(offsets[-1]) - dead
    dets = np.zeros((B, MAX_DET, 38), np.float32)
    xyxy = np.zeros((B, MAX_DET, 4), np.float32)
    rb = 8 * -(-w // 64) if native else mw // 8
    masks = np.full((cap, mh, rb), 0xFF, np.uint8)
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
                masks[s] = tg.pack(m, native, w)
            cls.append(inst["cls"])
            boxes.append(fbox)
            ms.append(m if s < cap else None)
        ref.append((np.array(cls), np.array(boxes, np.float32).reshape(-1, 4), ms))
    return dict(dets=dets, xyxy=xyxy, counts=counts, offsets=offsets, masks=masks), ref, offsets, cap


@functools.lru_cache(maxsize=None)
def device_batch(h, w, mh, mw, native, dead):
    arrays = host_batch(h, w, mh, mw, native, dead)[0]
    return {k: torch.from_numpy(v).cuda() for k, v in arrays.items()}


@functools.lru_cache(maxsize=None)
def reference(h, w, mh, mw, native, dead, name, calib_id="real"):
    """The restatement on every scene, once per (shape, settings)."""
    ref = host_batch(h, w, mh, mw, native, dead)[1]
    calib = CALIB if calib_id == "real" else degenerate_calib(h, w, mh, mw, native, dead)
    return [cr.measure_frame(h, w, cls, boxes, ms, calib, **SETTINGS[name]) for cls, boxes, ms in ref]


def degenerate_calib(h, w, mh, mw, native, dead):
    """tests/test_checker_ref.py's calibration (dist = 0, plane normal = the camera's x axis) with K02 on the left column of the
    first final stitch of scene I_BELOW: world(left, cy) is None there, world(cx, cy) exists, so the width is the estimate."""
    _, st = reference(h, w, mh, mw, native, dead, "defaults")[I_BELOW]
    left = [s["left"] for s in st if s["flags"] & cr.WIDTH][0]
    K = np.array([[1000.0, 0.0, float(left)], [0.0, 1000.0, h / 2.0], [0.0, 0.0, 1.0]])
    R = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])
    return K, np.zeros(5), R, np.array([0.5, 0.0, 1.0])


SETTINGS = {
    "defaults": dict(), "skip_cluster": dict(skip_cluster=True), "drop_empty": dict(drop_empty=True),
    "nb0_iters1": dict(envelope_neighborhood=0, min_stitches=1, kmeans_iters=1), "nb64": dict(envelope_neighborhood=64),
}
MODES = tg.MODES           # letterbox 736x960 masks for 960x1280 frames, native 960x1280, native 481x333


def _close(a, b):
    return tg._close(a, b, 1e-12)


def run_and_compare(h, w, mh, mw, native, dead, name, calib_id="real"):
    """One vti_measure_checker call on the sixteen scenes -> (the restatement's records and stitches, the device result).  Every
    frame and every slot is compared; the rows no slot owns must keep their sentinels."""
    eng = tg._engine(736, 960, 16)
    dev = device_batch(h, w, mh, mw, native, dead)
    _, ref, offsets, cap = host_batch(h, w, mh, mw, native, dead)
    exp = reference(h, w, mh, mw, native, dead, name, calib_id)
    calib = CALIB if calib_id == "real" else degenerate_calib(h, w, mh, mw, native, dead)
    extra = 5
    pre = dict(stitch_f64=torch.full((cap + extra, 7), SENTINEL_F, dtype=torch.float64, device="cuda"),
               stitch_i32=torch.full((cap + extra, 2), SENTINEL_I, dtype=torch.int32, device="cuda"))
    res = eng.measure_checker(dev, _params(calib, **SETTINGS[name]), h, w, native=native, result=pre)
    f64, i32 = res["frame_f64"].cpu().numpy(), res["frame_i32"].cpu().numpy()
    sf64, si32 = res["stitch_f64"].cpu().numpy(), res["stitch_i32"].cpu().numpy()
    written = np.zeros(cap + extra, bool)
    for b, ((cls, boxes, ms), (rec, st)) in enumerate(zip(ref, exp)):
        want = [rec["status"], rec["n_stitch"], rec["n_fabric"], rec["n_selected"], rec["n_dist"], rec["n_width"]]
        assert i32[b].tolist() == want, (b, i32[b].tolist(), want)
        assert _close(f64[b, 0], rec["avg_dist"]) and _close(f64[b, 1], rec["avg_width"]), (b, f64[b], rec)
        rank = {s["i"]: (j, s) for j, s in enumerate(st)}
        for i in range(len(cls)):
            slot = offsets[b] + i
            if slot >= cap:
                continue
            written[slot] = True
            if i not in rank:
                assert si32[slot].tolist() == [0, -1] and np.isnan(sf64[slot]).all(), (b, i)
                continue
            j, s = rank[i]
            assert si32[slot].tolist() == [s["flags"], j], (b, i, si32[slot].tolist(), s["flags"], j)
            for k, key in enumerate(("cx", "cy", "left", "right", "width", "edge_y", "dist")):
                assert _close(sf64[slot, k], s[key]), (b, i, key, sf64[slot, k], s[key])
    assert (sf64[~written] == SENTINEL_F).all() and (si32[~written] == SENTINEL_I).all()
    assert (~written).sum() == extra + max(-dead, 0)
    return exp, res


def _cases(recs):
    """What the scenes exercise, from the restatement alone: -> (sign rejections, fall-backs) as lists of scene indices."""
    sign, fall = [], []
    for b, (rec, st) in enumerate(recs):
        if rec["status"] != cr.OK:
            continue
        sel = [s for s in st if s["flags"] & cr.SELECTED]
        if not any(s["flags"] & cr.NEAR for s in sel):
            fall.append(b)
        elif any(s["img_dist"] is not None and s["img_dist"] <= 0 for s in sel):
            sign.append(b)
    return sign, fall


@pytest.mark.parametrize("name", list(SETTINGS))
@pytest.mark.parametrize("mode,h,w,mh,mw", MODES, ids=["letterbox", "native", "native_odd"])
def test_scenes_match_the_restatement(mode, h, w, mh, mw, name):
    need_gpu()
    native = mode == "native"
    exp, _ = run_and_compare(h, w, mh, mw, native, 3, name)
    st = [rec["status"] for rec, _ in exp]
    assert st[3] == cr.NO_FABRIC and st[4] == cr.NO_STITCHES
    if h != 960:                # the scenes are drawn for the reference frame; at the odd size they only have to agree
        return
    assert st.count(cr.OK) >= 9 and cr.NO_FABRIC in st and cr.NO_STITCHES in st, st
    sign, fall = _cases(exp)
    # a selected stitch on or above the edge is rejected while others pass (the row across the wave); nothing passes in
    # test_gpu_measure's first scene, whose rows lie 200+ px below the top edge, so its final set is the selected set
    assert I_STRADDLE in sign and 0 in fall, (sign, fall)
    if name == "skip_cluster":
        rec, _ = exp[I_STRADDLE]
        assert rec["n_selected"] == 11 and 0 < rec["n_dist"] < 11
    # the box fall-back changes the envelope of I_BOXES (not under drop_empty, where the instance does not exist)
    cls, boxes, ms = host_batch(h, w, mh, mw, native, 3)[1][I_BOXES]
    env = cr.fabric_envelope(h, w, cls, boxes, ms, **SETTINGS[name])[0]
    env_without = cr.fabric_envelope(h, w, cls, boxes, ms, drop_empty=True)[0]
    assert ((env != env_without).sum() > 400) == (name != "drop_empty")
    assert exp[I_BOXES][0]["n_fabric"] == (1 if name == "drop_empty" else 4)
    # the fabric of I_DEAD that has no slot is an empty mask: its box and the empty-mask instance's are all the fabric there is
    if name == "drop_empty":
        assert (exp[I_DEAD][0]["status"], exp[I_DEAD][0]["n_fabric"]) == (cr.NO_FABRIC, 0)
    else:
        assert (exp[I_DEAD][0]["status"], exp[I_DEAD][0]["n_fabric"]) == (cr.OK, 2)


@pytest.mark.parametrize("mode,h,w,mh,mw", MODES[:2], ids=["letterbox", "native"])
def test_rows_past_the_live_count_and_past_the_capacity_stay_untouched(mode, h, w, mh, mw):
    """A buffer with four slots of 0xFF past the live count: their rows, and the rows past the capacity, keep the sentinels (checked
    in run_and_compare); the dead fabric of I_DEAD now has its slot and is measured from its mask."""
    need_gpu()
    exp, _ = run_and_compare(h, w, mh, mw, mode == "native", -4, "defaults")
    assert exp[I_DEAD][0]["status"] == cr.OK and exp[I_DEAD][0]["n_fabric"] == 2


def test_the_width_estimate_on_the_degenerate_plane():
    need_gpu()
    mode, h, w, mh, mw = MODES[1]
    exp, _ = run_and_compare(h, w, mh, mw, True, 3, "defaults", "degenerate")
    rec, st = exp[I_BELOW]
    est = [s for s in st if s.get("estimated")]
    assert rec["status"] == cr.OK and len(est) >= 1 and all(s["flags"] & cr.WIDTH and s["width"] > 0 for s in est)
    assert rec["n_width"] == sum(1 for s in st if s["flags"] & cr.WIDTH) >= 3 and rec["avg_width"] is not None


def test_the_record_differs_from_vti_measures_on_the_same_inputs():
    """Same inputs, the nearest settings process_frame has (no ROI, max_px_distance 150): the checker measures to the other edge."""
    need_gpu()
    import vti_amd
    mode, h, w, mh, mw = MODES[0]
    exp, res = run_and_compare(h, w, mh, mw, False, 3, "defaults")
    dev = device_batch(h, w, mh, mw, False, 3)
    other = tg._engine(736, 960, 16).measure(dev, vti_amd.MeasureParams(*CALIB, roi_enabled=False, max_px_distance=150), h, w)
    a, b = res["frame_f64"].cpu().numpy(), other["frame_f64"].cpu().numpy()
    assert exp[I_BELOW][0]["avg_dist"] is not None and not np.isnan(b[I_BELOW, 0])
    assert abs(a[I_BELOW, 0] - b[I_BELOW, 0]) > 1.0                      # mm: the top edge against the bottom edge
    assert not np.array_equal(res["frame_i32"].cpu().numpy(), other["frame_i32"].cpu().numpy())


@pytest.mark.parametrize("retina", [False, True])
def test_stitch_distance_checker_equals_the_restatement_over_predict(retina):
    """Wiring: process_frames over two consecutive batches == the restatement over predict()'s Results, smoothing and text included."""
    need_gpu()
    import vti_amd
    model = vti_amd.YOLO(None, scale="n", nc=2, seed=3, cls_bias=-1.0)
    ck = vti_amd.StitchDistanceChecker(model, _params(), frame_buffer=8)
    smooth = cr.Smoother(8, 3)
    kw = dict(conf=0.20, iou=0.45, max_det=200, imgsz=640, retina_masks=retina)
    drop = bool(model.drop_empty_masks)
    for seed in (0, 1):
        frames = frames_u8(2, 960, 1280, seed)
        got, rows = ck.process_frames(frames, rows=True, **kw) if seed else (ck.process_frames(frames, **kw), None)
        results = model.predict(frames, swap_rb=False, **kw)
        assert len(got) == len(results) == 2
        for b, (g, r) in enumerate(zip(got, results)):
            n = len(r)
            masks = [m for m in r.masks.data_u8.cpu().numpy()] if n else []
            rec, st = cr.measure_frame(960, 1280, r.boxes.cls.cpu().numpy(), r.boxes.xyxy.cpu().numpy(), masks, CALIB, drop_empty=drop)
            exp = smooth(rec)
            assert set(g) - {"timestamp"} == set(exp), (g, exp)
            for k, v in exp.items():
                assert (g[k] is None) == (v is None) and (v is None or isinstance(v, str) and g[k] == v or
                                                          abs(g[k] - v) <= 1e-12 * max(1.0, abs(v))), (k, g, exp)
            if rows is not None:
                assert [rows[b]["status"], rows[b]["n_stitch"], rows[b]["n_fabric"]] == [rec["status"], rec["n_stitch"], rec["n_fabric"]]
                assert sorted(int(f) for f in rows[b]["flags"] if f) == sorted(s["flags"] for s in st)
                items = vti_amd.checker_text_items(g, rows[b], 960)
                assert items[-1][0] == f"Stitches: {rec['n_stitch']} | Fabric: {rec['n_fabric']}" or rec["status"] != cr.OK
    one = ck.process_frame(frames_u8(1, 960, 1280, 7)[0], **kw)
    assert "stitch_count" in one and "info_text" in one and "timestamp" in one
