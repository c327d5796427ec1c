"""Restatement of the measurement part of Utils/check_stitch_distance.py's process_frame (lines 281-553, drawing left out), on
explicit inputs.  TEST INFRASTRUCTURE (not collected: no test_ prefix).

measure_frame() follows the checker's text step by step on one frame's instances, in detection order, and returns the per-stitch
intermediates next to the per-frame record, in the shapes vti_measure_checker reports them.  Smoother is the checker's pair of
frame buffers and its info text.  Where the checker's text equals measurement.py's, the helper of oracle.consumer / oracle.geometry
/ measure_ref that restates it is used; the three places where it differs (the fall-back rectangles, the upper envelope and the
k-means) are written out here from the checker's own lines.
"""
from collections import deque

import numpy as np

from measure_ref import DIST, KEPT, MASK, NEAR, NO_FABRIC, NO_STITCHES, OK, SELECTED, WIDTH, _neighbourhood
from oracle import consumer as oc
from oracle import geometry as og

# check_stitch_distance.py:20-39
DEFAULTS = dict(stitch_id=0, fabric_id=1, min_stitches=3, max_px_distance=150, envelope_neighborhood=3, skip_cluster=False,
                kmeans_iters=10, drop_empty=False)


def kmeans_1d_two_clusters(values, max_iters=10):
    """check_stitch_distance.py:143-171, literally: `labels = new_labels` on both early exits (measurement.py's keeps the previous
    labels there)."""
    if values.size < 2:
        return np.zeros(values.shape[0], dtype=int), (float(values.mean()), float(values.mean()))
    c0 = float(values.min())
    c1 = float(values.max())
    labels = np.zeros(values.shape[0], dtype=int)
    for _ in range(max_iters):
        d0 = np.abs(values - c0)
        d1 = np.abs(values - c1)
        new_labels = (d1 < d0).astype(int)
        if new_labels.sum() == 0 or new_labels.sum() == len(values):
            labels = new_labels
            break
        new_c0 = float(values[new_labels == 0].mean()) if (new_labels == 0).any() else c0
        new_c1 = float(values[new_labels == 1].mean()) if (new_labels == 1).any() else c1
        if new_c0 == c0 and new_c1 == c1:
            labels = new_labels
            break
        c0, c1 = new_c0, new_c1
        labels = new_labels
    return labels, (c0, c1)


def filled_rectangle(h, w, x1, y1, x2, y2):
    """:332-333: tmp = zeros; cv2.rectangle(tmp, (x1i, y1i), (x2i, y2i), 1, -1): both corners inclusive, in either order, clipped."""
    tmp = np.zeros((h, w), dtype=np.uint8)
    xa, xb, ya, yb = min(x1, x2), max(x1, x2), min(y1, y2), max(y1, y2)
    r0, r1, c0, c1 = max(ya, 0), min(yb, h - 1), max(xa, 0), min(xb, w - 1)
    if r0 <= r1 and c0 <= c1:                       # (a slice with a negative end would count from the far side)
        tmp[r0:r1 + 1, c0:c1 + 1] = 1
    return tmp


def upper_envelope(fabric_mask):
    """:238-251."""
    h, w = fabric_mask.shape
    envelope = np.full((w,), -1, dtype=int)
    has_any = fabric_mask.any(axis=0)
    idx_top = np.argmax(fabric_mask > 0, axis=0)
    for x in range(w):
        envelope[x] = idx_top[x] if has_any[x] else -1
    return envelope


def fabric_envelope(h, w, cls, xyxy, masks, **settings):
    """The union of :310-336 + :344 and its upper envelope (None: the union is None or empty)."""
    p = dict(DEFAULTS, **settings)
    xyxy = np.asarray(xyxy, dtype=np.float32).reshape(-1, 4)
    fabric_masks = []
    for i in range(len(cls)):
        if p["drop_empty"] and (masks[i] is None or np.count_nonzero(masks[i]) == 0):
            continue
        if int(cls[i]) != p["fabric_id"]:
            continue
        x1, y1, x2, y2 = (int(v) for v in xyxy[i])
        mask = None if masks[i] is None else oc.instance_bitmap(np.asarray(masks[i]), h, w)
        fabric_masks.append(mask if mask is not None else filled_rectangle(h, w, x1, y1, x2, y2))
    fabric_mask = oc.combine_masks(fabric_masks, h, w)
    if fabric_mask is None or np.count_nonzero(fabric_mask) == 0:
        return None, len(fabric_masks)
    return upper_envelope(fabric_mask), len(fabric_masks)


def measure_frame(h, w, cls, xyxy, masks, calib, **settings):
    """h, w: frame size.  cls [n], xyxy f32 [n,4] (frame px), masks: per instance the mask as predict returns it (u8/bool, letterbox
    HxW or frame h x w) or None for a slot past the capacity (an empty mask).  calib = (K, dist, R, t).
    -> (record dict, stitches: list of dicts in stitch_meta order, each with its detection index `i`)."""
    p = dict(DEFAULTS, **settings)
    K, dist, R, t = calib
    n_c, d_c = og.compute_camera_plane(R, t)

    def p2w(u, v):
        return og.pixel_to_world_using_camera_plane(float(u), float(v), K, dist, R, t, n_c, d_c)

    nb = p["envelope_neighborhood"]
    xyxy = np.asarray(xyxy, dtype=np.float32).reshape(-1, 4)
    # :310-336 (drop_empty: as YOLO(drop_empty_masks=True), on the mask predict returns); there is no ROI
    stitch_masks, stitch_boxes, stitch_idx = [], [], []
    for i in range(len(cls)):
        if p["drop_empty"] and (masks[i] is None or np.count_nonzero(masks[i]) == 0):
            continue
        if int(cls[i]) == p["stitch_id"]:
            stitch_masks.append(None if masks[i] is None else oc.instance_bitmap(np.asarray(masks[i]), h, w))
            stitch_boxes.append(tuple(int(v) for v in xyxy[i]))
            stitch_idx.append(i)
    envelope, n_fabric = fabric_envelope(h, w, cls, xyxy, masks, **settings)
    # :362-402 (its values do not depend on the status; vti_measure_checker reports them for every frame)
    stitches = []
    for j, mask in enumerate(stitch_masks):
        cx, cy, px_width, left, right = oc.stitch_stats(mask, stitch_boxes[j])
        stitches.append(dict(i=stitch_idx[j], cx=cx, cy=cy, left=left, right=right, px_width=px_width, width=np.nan, edge_y=np.nan,
                             dist=np.nan, img_dist=None, flags=KEPT | (MASK if mask is not None else 0)))
    rec = dict(status=OK, n_stitch=len(stitches), n_fabric=n_fabric, n_selected=0, n_dist=0, n_width=0, avg_dist=None, avg_width=None)
    if envelope is None:                            # :344-347
        rec["status"] = NO_FABRIC
        return rec, stitches
    if len(stitches) == 0:                          # :404-406
        rec["status"] = NO_STITCHES
        return rec, stitches
    centroids_y = [s["cy"] for s in stitches]
    # :408-429
    labels = np.zeros(len(centroids_y), dtype=int)
    chosen_label = 0
    if not p["skip_cluster"] and len(centroids_y) >= 2:
        vals = np.array(centroids_y)
        labels, _ = kmeans_1d_two_clusters(vals, p["kmeans_iters"])
        fabric_valid = envelope[envelope >= 0]
        if fabric_valid.size > 0:
            fabric_mean_y = float(np.mean(fabric_valid))
            c0_mean = float(vals[labels == 0].mean()) if (labels == 0).any() else 1e9
            c1_mean = float(vals[labels == 1].mean()) if (labels == 1).any() else 1e9
            chosen_label = 0 if abs(c0_mean - fabric_mean_y) < abs(c1_mean - fabric_mean_y) else 1
    selected = [i for i, lab in enumerate(labels) if lab == chosen_label]
    for j in selected:
        stitches[j]["flags"] |= SELECTED
    # :431-454; NEAR is reported for every stitch, the filter uses the selected ones
    for s in stitches:
        env_vals = _neighbourhood(envelope, int(round(s["cx"])), nb, w)
        if env_vals:
            env_y = int(round(float(np.median(env_vals))))
            img_dist = s["img_dist"] = float(s["cy"]) - float(env_y)
            if 0 < img_dist < p["max_px_distance"]:
                s["flags"] |= NEAR
    final = [j for j in selected if stitches[j]["flags"] & NEAR]
    if len(final) == 0:
        final = selected
    # :462-507
    per_dists, per_widths = [], []
    for j in final:
        s = stitches[j]
        cx, cy = s["cx"], s["cy"]
        cx_int = int(np.clip(int(round(cx)), 0, w - 1))
        env_vals = _neighbourhood(envelope, cx_int, nb, w)
        if len(env_vals) > 0:
            edge_y = float(np.median(env_vals))
            s["edge_y"] = edge_y
            p_stitch, p_edge = p2w(cx, cy), p2w(cx, edge_y)
            if p_stitch is not None and p_edge is not None:
                s["dist"] = float(np.linalg.norm(p_stitch - p_edge)) * 1000.0
                s["flags"] |= DIST
                per_dists.append(s["dist"])
        p_left, p_right = p2w(s["left"], cy), p2w(s["right"], cy)
        if p_left is not None and p_right is not None:
            s["width"] = float(np.linalg.norm(p_right - p_left)) * 1000.0
            s["flags"] |= WIDTH
            per_widths.append(s["width"])
        else:
            p_a, p_b = p2w(cx, cy), p2w(cx + 10, cy)
            if p_a is not None and p_b is not None:
                mm_per_10px = float(np.linalg.norm(p_b - p_a)) * 1000.0
                s["width"] = (s["px_width"] / 10.0) * mm_per_10px
                s["flags"] |= WIDTH
                s["estimated"] = True
                per_widths.append(s["width"])
    # :515-517
    rec.update(n_selected=len(selected), n_dist=len(per_dists), n_width=len(per_widths),
               avg_dist=float(np.mean(per_dists)) if len(per_dists) >= p["min_stitches"] else None,
               avg_width=float(np.mean(per_widths)) if len(per_widths) >= p["min_stitches"] else None)
    return rec, stitches


def info_text(smooth_dist, smooth_width, n_found, min_stitches):
    """:533-540."""
    if smooth_dist is not None and smooth_width is not None:
        return f"Edge Dist: {smooth_dist:.2f}mm | Avg Width: {smooth_width:.2f}mm (n={n_found})"
    elif smooth_dist is not None:
        return f"Edge Distance: {smooth_dist:.2f}mm (n={n_found})"
    elif smooth_width is not None:
        return f"Avg Width: {smooth_width:.2f}mm (n={n_found})"
    return f"Insufficient stitches (found {n_found}, need {min_stitches})"


class Smoother:
    """:519-540 and the early returns :345-347, :404-406."""

    def __init__(self, frame_buffer=8, min_stitches=3):
        self.d, self.w, self.min_stitches = deque(maxlen=frame_buffer), deque(maxlen=frame_buffer), min_stitches

    def __call__(self, rec):
        if rec["status"] != OK:
            text = "Fabric not detected" if rec["status"] == NO_FABRIC else "No stitches detected"
            return dict(edge_distance_mm=None, stitch_width_mm=None, stitch_count=0, info_text=text, error=text)
        sd = sw = None
        if rec["avg_dist"] is not None:
            self.d.append(rec["avg_dist"])
            sd = float(np.median(self.d))
        if rec["avg_width"] is not None:
            self.w.append(rec["avg_width"])
            sw = float(np.median(self.w))
        return dict(edge_distance_mm=sd, stitch_width_mm=sw, stitch_count=rec["n_width"],
                    info_text=info_text(sd, sw, rec["n_width"], self.min_stitches))
