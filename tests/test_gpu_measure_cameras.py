"""-m gpu: vti_measure_cameras (one measurement call for a batch that mixes cameras) against the per-frame restatement in
tests/measure_ref.py, each frame with its own camera's calibration and settings.  Statuses, counts, flags and ranks exactly; floats
within 1e-12 relative (tests/test_gpu_measure.py's tolerances).  Against vti_measure the results are compared byte for byte."""
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

import measure_ref as mr
import oracle.geometry as og
from gpu_util import frames_u8, need_gpu
from test_gpu_measure import DH, DW, MODES, _close, _engine, build_batch, scenes

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _calib(extrinsics):
    c = json.load(open(os.path.join(G, "camera_calibration.json")))
    e = json.load(open(os.path.join(G, extrinsics)))
    return (np.array(c["camera_matrix"], dtype=np.float64), np.array(c["dist_coeffs"], dtype=np.float64).ravel(),
            og.rodrigues(np.array(e["rvec"], dtype=np.float64)), np.array(e["tvec"], dtype=np.float64))


CALIBS = [_calib("extrinsics.json"), _calib("camera_extrinsics.json")]
ALT = dict(roi=(10, 200, 1270, 900), skip_cluster=True, min_stitches=1, envelope_neighborhood=1)
# camera -> (calibration file, settings): both files with config.py's defaults, and each again with other settings
CAMERAS = [(0, dict()), (1, dict()), (0, dict(ALT, drop_empty=True)), (1, dict(ALT))]
OUT_KEYS = ("frame_f64", "frame_i32", "stitch_f64", "stitch_i32")
MODE_IDS = ["letterbox", "native", "native_odd"]


def _settings(cam, h, w):
    """Camera `cam`'s settings for an h x w frame (the ROI is drawn for 1280 x 960 and scaled with the frame, as test_gpu_measure)."""
    sx, sy = w / DW, h / DH
    s = dict(CAMERAS[cam][1])
    x1, y1, x2, y2 = s.pop("roi", (10, 300, 1270, 760))
    return dict(s, roi=(int(x1 * sx), int(y1 * sy), int(x2 * sx), int(y2 * sy)))


def _params(cam, h, w):
    import vti_amd
    return vti_amd.MeasureParams(*CALIBS[CAMERAS[cam][0]], **_settings(cam, h, w))


def _host(res):
    return {k: res[k].cpu().numpy() for k in OUT_KEYS}


def _poisoned(B, cap):
    """Result tensors prefilled, so that rows a call must leave untouched compare equal between two calls."""
    return dict(frame_f64=torch.full((B, 2), -7.0, dtype=torch.float64, device="cuda"),
                frame_i32=torch.full((B, 6), -7, dtype=torch.int32, device="cuda"),
                stitch_f64=torch.full((cap, 7), -7.0, dtype=torch.float64, device="cuda"),
                stitch_i32=torch.full((cap, 2), -7, dtype=torch.int32, device="cuda"))


def check_frame(host, b, frame_ref, offsets, cap, h, w, cam):
    """Frame b of `host` against the restatement under camera `cam`; -> the restatement's record."""
    cls, boxes, ms = frame_ref
    rec, st = mr.measure_frame(h, w, cls, boxes, ms, CALIBS[CAMERAS[cam][0]], **_settings(cam, h, w))
    f64, i32, sf64, si32 = (host[k] for k in OUT_KEYS)
    exp = [rec["status"], rec["n_stitch"], rec["n_fabric"], rec["n_selected"], rec["n_dist"], rec["n_width"]]
    assert i32[b].tolist() == exp, (b, cam, i32[b].tolist(), exp)
    assert _close(f64[b, 0], rec["avg_dist"]) and _close(f64[b, 1], rec["avg_width"]), (b, cam, f64[b], rec)
    rank = {s["i"]: (j, s) for j, s in enumerate(st)}
    for i in range(len(cls)):
        slot = offsets[b] + i
        if slot >= cap:
            continue
        if i not in rank:
            assert si32[slot].tolist() == [0, -1] and np.isnan(sf64[slot]).all(), (b, i)
            continue
        j, s = rank[i]
        assert si32[slot].tolist() == [s["flags"], j], (b, i, si32[slot].tolist(), s["flags"], j)
        for k, key in enumerate(("cx", "cy", "left", "right", "width", "edge_y", "dist")):
            assert _close(sf64[slot, k], s[key]), (b, i, key, sf64[slot, k], s[key])
    return rec


def _mixed(mode, h, w, mh, mw, cams=None):
    """The twelve scenes with round-robin cameras (or `cams`) through one vti_measure_cameras call."""
    native = mode == "native"
    eng = _engine(736, 960, 16)
    dev, ref, offsets, cap = build_batch(scenes(), h, w, mh, mw, native, dead=3)
    B = len(ref)
    rr = [b % len(CAMERAS) for b in range(B)]
    table = eng.pack_cameras([_params(c, h, w) for c in range(len(CAMERAS))], "cuda")
    idx = torch.tensor(rr if cams is None else cams, dtype=torch.int32, device="cuda")
    res = eng.measure(dev, table, h, w, native=native, cameras=idx, result=_poisoned(B, cap))
    return eng, dev, ref, offsets, cap, rr, _host(res)


@pytest.mark.parametrize("mode,h,w,mh,mw", MODES, ids=MODE_IDS)
def test_mixed_batch_matches_the_restatement_per_frame(mode, h, w, mh, mw):
    need_gpu()
    eng, dev, ref, offsets, cap, rr, host = _mixed(mode, h, w, mh, mw)
    recs = [check_frame(host, b, ref[b], offsets, cap, h, w, rr[b]) for b in range(len(ref))]
    st = [r["status"] for r in recs]
    print("statuses", st)
    assert st[3] == mr.NO_FABRIC and st[4] == mr.NO_STITCHES
    if h == 960:
        assert st.count(mr.OK) >= 9, st
    # the test must not be able to pass on a camera mix-up: the other calibration file gives other millimetres
    with_dist = 0
    for b, rec in enumerate(recs):
        if rec["avg_dist"] is None:
            continue
        cls, boxes, ms = ref[b]
        other, _ = mr.measure_frame(h, w, cls, boxes, ms, CALIBS[1 - CAMERAS[rr[b]][0]], **_settings(rr[b], h, w))
        assert other["avg_dist"] is not None
        rel = abs(other["avg_dist"] - rec["avg_dist"]) / abs(rec["avg_dist"])
        print("frame", b, "camera", rr[b], "avg_dist", rec["avg_dist"], "other calibration", other["avg_dist"], "rel", rel)
        assert rel > 1e-6, (b, rec["avg_dist"], other["avg_dist"])
        with_dist += 1
    assert with_dist >= 1


@pytest.mark.parametrize("mode,h,w,mh,mw", MODES[:2], ids=MODE_IDS[:2])
def test_one_row_table_is_vti_measure_byte_for_byte(mode, h, w, mh, mw):
    need_gpu()
    native = mode == "native"
    eng = _engine(736, 960, 16)
    dev, ref, offsets, cap = build_batch(scenes(), h, w, mh, mw, native, dead=3)
    B = len(ref)
    p = _params(0, h, w)
    plain = _host(eng.measure(dev, p, h, w, native=native, result=_poisoned(B, cap)))
    table = eng.pack_cameras([p], "cuda")
    idx = torch.zeros(B, dtype=torch.int32, device="cuda")
    one = _host(eng.measure(dev, table, h, w, native=native, cameras=idx, result=_poisoned(B, cap)))
    for k in OUT_KEYS:
        assert plain[k].tobytes() == one[k].tobytes(), k
    # the host-sequence and list-of-params forms are the same call
    again = _host(eng.measure(dev, [p], h, w, native=native, cameras=[0] * B, result=_poisoned(B, cap)))
    for k in OUT_KEYS:
        assert plain[k].tobytes() == again[k].tobytes(), k


@pytest.mark.parametrize("mode,h,w,mh,mw", MODES[:2], ids=MODE_IDS[:2])
def test_frame_b_is_vti_measure_with_its_camera_byte_for_byte(mode, h, w, mh, mw):
    need_gpu()
    native = mode == "native"
    eng, dev, ref, offsets, cap, rr, mixed = _mixed(mode, h, w, mh, mw)
    B = len(ref)
    for cam in range(len(CAMERAS)):
        plain = _host(eng.measure(dev, _params(cam, h, w), h, w, native=native, result=_poisoned(B, cap)))
        for b in range(B):
            if rr[b] != cam:
                continue
            assert mixed["frame_f64"][b].tobytes() == plain["frame_f64"][b].tobytes(), (cam, b)
            assert mixed["frame_i32"][b].tobytes() == plain["frame_i32"][b].tobytes(), (cam, b)
            lo, hi = min(offsets[b], cap), min(offsets[b + 1], cap)
            assert mixed["stitch_f64"][lo:hi].tobytes() == plain["stitch_f64"][lo:hi].tobytes(), (cam, b)
            assert mixed["stitch_i32"][lo:hi].tobytes() == plain["stitch_i32"][lo:hi].tobytes(), (cam, b)


def test_a_camera_index_outside_the_table_is_reported_per_frame():
    """camera_of_frame -1 (frame 1) and n_cams (frame 6): status VTI_MEASURE_BAD_CAMERA, NaN averages, zero counts, their slots
    flags 0 / rank -1 / NaN; every other frame as in the mixed-batch test.  The kernels compare the index with [0, n_cams) before
    they form a table address (consumer.hip: envelope_bits_kernel, measure_frames_kernel)."""
    need_gpu()
    import vti_amd
    mode, h, w, mh, mw = MODES[0]
    rr = [b % len(CAMERAS) for b in range(12)]
    cams = list(rr)
    cams[1], cams[6] = -1, len(CAMERAS)
    eng, dev, ref, offsets, cap, _, host = _mixed(mode, h, w, mh, mw, cams=cams)
    assert vti_amd._lib.VTI_MEASURE_BAD_CAMERA == 3
    for b in range(12):
        if b in (1, 6):
            assert host["frame_i32"][b].tolist() == [3, 0, 0, 0, 0, 0], host["frame_i32"][b]
            assert np.isnan(host["frame_f64"][b]).all()
            lo, hi = min(offsets[b], cap), min(offsets[b + 1], cap)
            assert hi > lo
            assert (host["stitch_i32"][lo:hi] == np.array([0, -1])).all() and np.isnan(host["stitch_f64"][lo:hi]).all()
        else:
            check_frame(host, b, ref[b], offsets, cap, h, w, rr[b])
    # rows past the live slots stay untouched
    assert (host["stitch_i32"][min(offsets[-1], cap):] == -7).all()
    with pytest.raises(ValueError):       # the host-sequence form is refused before the call
        eng.measure(dev, eng.pack_cameras([_params(0, h, w)], "cuda"), h, w, cameras=cams)


@pytest.mark.parametrize("retina", [False, True])
def test_multi_camera_measurer_equals_one_stitch_measurer_per_camera_over_predict(retina):
    """Wiring: two consecutive mixed batches through MultiCameraMeasurer == one StitchMeasurer per camera fed only its own frames in
    the same order (the second batch also pins the carry-over of every camera's deques)."""
    need_gpu()
    import vti_amd
    model = vti_amd.YOLO(None, scale="n", nc=2, seed=3, cls_bias=-1.0)
    params = [dataclasses.replace(_params(c, 960, 1280), drop_empty=False) for c in range(len(CAMERAS))]
    mc = vti_amd.MultiCameraMeasurer(model, params, frame_buffer=8)
    singles = [vti_amd.StitchMeasurer(model, p, frame_buffer=8) for p in params]
    kw = dict(conf=0.20, iou=0.25, max_det=200, imgsz=960, retina_masks=retina)
    for seed, cams in ((0, [0, 1, 2, 3, 1, 0]), (1, [3, 3, 0, 2, 0, 1])):
        frames = frames_u8(6, 960, 1280, seed)
        got = mc.process_frames(frames, cams, **kw)
        assert [g["camera"] for g in got] == cams
        assert sum(g["edge_distance_mm"] is not None for g in got) >= 2      # the deques are in use, or the carry-over is not tested
        exp = [None] * len(cams)
        for c in range(len(CAMERAS)):
            mine = [b for b, x in enumerate(cams) if x == c]
            for b, rec in zip(mine, singles[c].process_frames(frames[mine], **kw)):
                exp[b] = rec
        for b, (g, e) in enumerate(zip(got, exp)):
            print("frame", b, "camera", cams[b], {k: v for k, v in g.items() if k != "timestamp"})
            assert {k: v for k, v in g.items() if k not in ("timestamp", "camera")} == {k: v for k, v in e.items() if k != "timestamp"}, b
    with pytest.raises(ValueError):
        mc.process_frames(frames, [0, 1, 2, 3, 4, 0], **kw)
    with pytest.raises(ValueError):
        mc.process_frames(frames, [0, 1], **kw)
