"""Restatement of the measurement part of measurement.py's process_frame (lines 240-510, drawing left out), composed from
oracle.consumer and oracle.geometry.  TEST INFRASTRUCTURE (not collected: no test_ prefix).

measure_frame() follows the reference step by step on one frame's instances, in detection order, and returns the per-stitch
intermediates next to the per-frame record, in the shapes vti_measure reports them.  Smoother is the reference's frame buffer.
"""
from collections import deque

import numpy as np

from oracle import consumer as oc
from oracle import geometry as og

KEPT, MASK, SELECTED, NEAR, DIST, WIDTH = 1, 2, 4, 8, 16, 32
OK, NO_FABRIC, NO_STITCHES = 0, 1, 2

DEFAULTS = dict(stitch_id=0, fabric_id=1, roi=(10, 300, 1270, 760), roi_enabled=True, min_stitches=3, max_px_distance=250,
                envelope_neighborhood=3, skip_cluster=False, two_row_threshold_px=30, kmeans_iters=10, drop_empty=False)


def _neighbourhood(envelope, c, nb, w):
    xs = [int(np.clip(c + dx, 0, w - 1)) for dx in range(-nb, nb + 1)]
    return [envelope[x] for x in xs if envelope[x] >= 0]


def measure_frame(h, w, cls, xyxy, masks, calib, **settings):
    """h, w: frame size.  cls [n], xyxy f32 [n,4] (frame px, vti_scale_boxes), masks: per instance the mask as predict returns it
    (u8/bool, letterbox HxW or frame h x w) or None for a slot past the capacity (an empty mask).  calib = (K, dist, R, t).
    -> (record dict, stitches: list of dicts in stitch_meta order, each with its detection index `i`)."""
    p = dict(DEFAULTS, **settings)
    K, dist, R, t = calib
    n_c, d_c = og.compute_camera_plane(R, t)

    def p2w(u, v):
        return og.pixel_to_world_using_camera_plane(float(u), float(v), K, dist, R, t, n_c, d_c)

    nb = p["envelope_neighborhood"]
    xyxy = np.asarray(xyxy, dtype=np.float32).reshape(-1, 4)
    # step 1: instances (drop_empty: as YOLO(drop_empty_masks=True), on the mask predict returns)
    live = [i for i in range(len(cls)) if not p["drop_empty"] or (masks[i] is not None and np.count_nonzero(masks[i]) > 0)]
    # step 2: ROI (measurement.py:220-238, 251-260)
    if p["roi_enabled"]:
        keep, ib = oc.roi_keep(xyxy, h, w, p["roi"])
    else:
        keep, ib = np.ones(len(xyxy), bool), np.trunc(xyxy.astype(np.float64)).astype(np.int64)
    stitch_masks, stitch_boxes, stitch_idx, fabric_masks = [], [], [], []
    for i in live:
        cid = int(cls[i])
        if not keep[i]:
            continue
        x1, y1, x2, y2 = (int(v) for v in ib[i])
        # step 3: get_instance_mask_as_bitmap (measurement.py:70-86)
        mask = None if masks[i] is None else oc.instance_bitmap(np.asarray(masks[i]), h, w)
        if cid == p["stitch_id"]:
            stitch_masks.append(mask)
            stitch_boxes.append((x1, y1, x2, y2))
            stitch_idx.append(i)
        elif cid == p["fabric_id"]:
            if mask is not None:
                fabric_masks.append(mask)
    # step 5 (its values do not depend on the status; vti_measure reports them for every frame)
    stitches = []
    for j, mask in enumerate(stitch_masks):
        cx, cy, _, left, right = oc.stitch_stats(mask, stitch_boxes[j])
        stitches.append(dict(i=stitch_idx[j], cx=cx, cy=cy, left=left, right=right, width=np.nan, edge_y=np.nan, dist=np.nan,
                             flags=KEPT | (MASK if mask is not None else 0)))
    rec = dict(status=OK, n_stitch=len(stitches), n_fabric=len(fabric_masks), n_selected=0, n_dist=0, n_width=0,
               avg_dist=None, avg_width=None)
    # step 4: fabric (measurement.py:280-289)
    fabric_mask = oc.combine_masks(fabric_masks, h, w)
    if fabric_mask is None or np.count_nonzero(fabric_mask) == 0:
        rec["status"] = NO_FABRIC
        return rec, stitches
    envelope = oc.lower_envelope(fabric_mask)
    if len(stitches) == 0:
        rec["status"] = NO_STITCHES
        return rec, stitches
    centroids_y = [s["cy"] for s in stitches]
    # step 6: widths (measurement.py:340-368)
    all_widths = []
    for s in stitches:
        pl, pr = p2w(s["left"], s["cy"]), p2w(s["right"], s["cy"])
        if pl is not None and pr is not None:
            s["width"] = float(np.linalg.norm(pr - pl)) * 1000.0
            s["flags"] |= WIDTH
            all_widths.append(s["width"])
    # step 7: row selection (measurement.py:370-406)
    if p["skip_cluster"]:
        vals = np.array(centroids_y)
        if len(vals) >= 2:
            median_y = np.median(vals)
            if vals.max() - vals.min() > p["two_row_threshold_px"]:
                selected = [i for i, cy in enumerate(centroids_y) if cy >= median_y]
            else:
                selected = list(range(len(centroids_y)))
        else:
            selected = list(range(len(centroids_y)))
    else:
        if len(centroids_y) >= 2:
            vals = np.array(centroids_y)
            labels, _ = og.kmeans_1d_two_clusters(vals, p["kmeans_iters"])
            fabric_valid = envelope[envelope >= 0]
            if fabric_valid.size > 0:
                fabric_mean_y = float(np.mean(fabric_valid))
                c0 = float(vals[labels == 0].mean()) if (labels == 0).any() else 1e9
                c1 = float(vals[labels == 1].mean()) if (labels == 1).any() else 1e9
                chosen = 0 if abs(c0 - fabric_mean_y) < abs(c1 - fabric_mean_y) else 1
            else:
                chosen = 0
            selected = [i for i, lab in enumerate(labels) if lab == chosen]
        else:
            selected = list(range(len(centroids_y)))
    for j in selected:
        stitches[j]["flags"] |= SELECTED
    # step 8: proximity (measurement.py:408-431); NEAR is reported for every stitch, the filter uses the selected ones
    for j, s in enumerate(stitches):
        env_vals = _neighbourhood(envelope, int(round(s["cx"])), nb, w)
        if env_vals:
            env_y = int(round(float(np.median(env_vals))))
            if abs(float(s["cy"]) - float(env_y)) < p["max_px_distance"]:
                s["flags"] |= NEAR
    final = [j for j in selected if stitches[j]["flags"] & NEAR]
    if not final:
        final = selected
    # step 9: distances (measurement.py:433-462)
    per_dists = []
    for j in final:
        s = stitches[j]
        cx_int = int(np.clip(int(round(s["cx"])), 0, w - 1))
        env_vals = _neighbourhood(envelope, cx_int, nb, w)
        if env_vals:
            edge_y = float(np.median(env_vals))
            s["edge_y"] = edge_y
            ps, pe = p2w(s["cx"], s["cy"]), p2w(s["cx"], edge_y)
            if ps is not None and pe is not None:
                s["dist"] = float(np.linalg.norm(ps - pe)) * 1000.0
                s["flags"] |= DIST
                per_dists.append(s["dist"])
    # step 10: averages (measurement.py:469-472)
    rec.update(n_selected=len(selected), n_dist=len(per_dists), n_width=len(all_widths),
               avg_dist=float(np.mean(per_dists)) if len(per_dists) >= p["min_stitches"] else None,
               avg_width=float(np.mean(all_widths)) if len(all_widths) >= p["min_stitches"] else None)
    return rec, stitches


class Smoother:
    """Step 11 (measurement.py:474-484, 505-510, error returns 285-287, 333-337)."""

    def __init__(self, frame_buffer=8):
        self.d, self.w = deque(maxlen=frame_buffer), deque(maxlen=frame_buffer)

    def __call__(self, rec):
        if rec["status"] == NO_FABRIC:
            return dict(edge_distance_mm=None, stitch_width_mm=None, stitch_count=0, error="Fabric not detected")
        if rec["status"] == NO_STITCHES:
            return dict(edge_distance_mm=None, stitch_width_mm=None, stitch_count=0, error="No stitches detected")
        sd = sw = None
        if rec["avg_dist"] is not None:
            self.d.append(rec["avg_dist"])
            sd = float(np.median(self.d))
        if rec["avg_width"] is not None:
            self.w.append(rec["avg_width"])
            sw = float(np.median(self.w))
        return dict(edge_distance_mm=sd, stitch_width_mm=sw, stitch_count=rec["n_dist"])
