"""annotate.checker_display_list + rasterise against OpenCV itself, where OpenCV is installed (skipped elsewhere): the checker's own
drawing calls (Utils/check_stitch_distance.py:323-336, 349-360, 485-486, 497-499, 510, 543-545), issued with cv2 from the same inputs
and rows, must give the picture the restatement gives.  Text is left out on both sides (the package draws it last, on the host)."""
import numpy as np
import pytest

cv2 = pytest.importorskip("cv2")

import checker_ref as cr                                # noqa: E402
import test_gpu_checker as tc                           # noqa: E402
from oracle import consumer as oc                       # noqa: E402
from vti_amd import annotate as A                       # noqa: E402


def _rows(h, w, cls, boxes, ms, calib, **settings):
    """vti_measure_checker's rows as the restatement in checker_ref.py gives them."""
    rec, st = cr.measure_frame(h, w, cls, boxes, ms, calib, **settings)
    n = len(cls)
    flags, rank, f64 = np.zeros(n, np.int32), np.full(n, -1, np.int32), np.full((n, 7), np.nan)
    for j, s in enumerate(st):
        if ms[s["i"]] is not None:
            flags[s["i"]], rank[s["i"]] = s["flags"], j
            f64[s["i"]] = [s["cx"], s["cy"], s["left"], s["right"], s["width"], s["edge_y"], s["dist"]]
    return dict(status=rec["status"], flags=flags, rank=rank, f64=f64), st


def _checker_draws(frame, cls, boxes, ms, rows, st, calib, drop_empty):
    """The checker's cv2 calls in its order, on the per-stitch values of `rows` (what the device reports)."""
    from oracle import geometry as og
    h, w = frame.shape[:2]
    K, dist, R, t = calib
    n_c, d_c = og.compute_camera_plane(R, t)
    img = frame.copy()
    fabric = []
    for i in range(len(cls)):
        if drop_empty and (ms[i] is None or not np.count_nonzero(ms[i])):
            continue
        x1, y1, x2, y2 = (int(v) for v in boxes[i])
        if int(cls[i]) == 0:
            cv2.rectangle(img, (x1, y1), (x2, y2), (255, 255, 0), 1)
        elif int(cls[i]) == 1:
            mask = None if ms[i] is None else oc.instance_bitmap(np.asarray(ms[i]), h, w)
            if mask is None:
                mask = np.zeros((h, w), np.uint8)
                cv2.rectangle(mask, (x1, y1), (x2, y2), 1, -1)
            fabric.append(mask)
            cv2.rectangle(img, (x1, y1), (x2, y2), (255, 0, 255), 2)
    union = oc.combine_masks(fabric, h, w)
    if union is None or not np.count_nonzero(union):
        return img
    env = cr.upper_envelope(union)
    pts = [(x, int(env[x])) for x in range(w) if env[x] >= 0]
    if pts:
        cv2.polylines(img, [np.array(pts[::max(1, int(len(pts) / 1000))], dtype=np.int32)], isClosed=False, color=(255, 128, 0), thickness=2)
    if rows["status"] != A.OK:
        return img
    final = [s for s in st if s["flags"] & A.SELECTED and s["flags"] & A.NEAR] or [s for s in st if s["flags"] & A.SELECTED]
    for s in final:
        if ms[s["i"]] is None:
            continue                                    # no slot, no row: the device has nothing to draw it from
        cx, cy = s["cx"], s["cy"]
        if s["flags"] & A.DIST:
            e = (int(np.clip(int(round(cx)), 0, w - 1)), int(round(s["edge_y"])))
            cv2.line(img, e, (int(round(cx)), int(round(cy))), (0, 255, 0), 1)
            cv2.circle(img, e, 2, (255, 0, 255), -1)
        p_l = og.pixel_to_world_using_camera_plane(s["left"], cy, K, dist, R, t, n_c, d_c)
        p_r = og.pixel_to_world_using_camera_plane(s["right"], cy, K, dist, R, t, n_c, d_c)
        if p_l is not None and p_r is not None:
            a, b = (int(round(s["left"])), int(round(cy))), (int(round(s["right"])), int(round(cy)))
            cv2.circle(img, a, 3, (200, 200, 0), -1)
            cv2.circle(img, b, 3, (200, 200, 0), -1)
            cv2.line(img, a, b, (200, 200, 0), 1)
        cv2.circle(img, (int(round(cx)), int(round(cy))), 4, (0, 255, 0), -1)
    contours, _ = cv2.findContours((union > 0).astype(np.uint8), cv2.RETR_EXTERNAL, cv2.CHAIN_APPROX_SIMPLE)
    if contours:
        cv2.drawContours(img, contours, -1, (255, 128, 0), 2)
    return img


@pytest.mark.parametrize("drop_empty", [False, True])
@pytest.mark.parametrize("scene", [0, 3, 4, tc.I_BELOW, tc.I_STRADDLE, tc.I_BOXES, tc.I_DEAD])
def test_the_checkers_own_drawing_calls_give_the_restatements_picture(scene, drop_empty):
    mode, h, w, mh, mw = tc.MODES[0]
    cls, boxes, ms = tc.host_batch(h, w, mh, mw, False, 3)[1][scene]
    rows, st = _rows(h, w, cls, boxes, ms, tc.CALIB, drop_empty=drop_empty)
    K, dist, R, t = tc.CALIB
    params = dict(stitch_id=0, fabric_id=1, drop_empty=drop_empty, K=K, dist=dist, R=R, t=t)
    frame = np.random.default_rng(scene).integers(0, 256, (h, w, 3), dtype=np.uint8)
    got = A.rasterise(frame, A.checker_display_list(h, w, cls, boxes, ms, rows, params))
    want = _checker_draws(frame, cls, boxes, ms, rows, st, tc.CALIB, drop_empty)
    assert np.array_equal(got, want), int((got != want).any(axis=-1).sum())
