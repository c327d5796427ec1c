"""process_frame's annotated frame (measurement.py:219-504) -- the host SPECIFICATION of vti_annotate.

The product draws the overlay on the device (libvti.so `vti_annotate`, csrc/annotate.hip, Engine.annotate), byte for byte what
`rasterise(frame, display_list(...))` returns; the functions below stay as the statement of the semantics and as the reference of
tests/test_gpu_annotate.py (pure Python: about a second per frame, so the package never calls them on the hot path).

Two parts.  `display_list` restates WHAT the reference draws, in its order, with its BGR colours and thicknesses; `rasterise`
restates WHICH PIXELS each primitive covers, following OpenCV's drawing.cpp for LINE_8 and shift = 0: Line (the 8-connected
LineIterator on the clipped segment), ThickLine (the 16.16 fixed-point quad: its four edges by Line2, its interior by
FillConvexPoly's scanline rule, a filled Circle of radius thickness/2 at the ends), Circle (the midpoint circle's spans), PolyLine
and rectangle (their edges as ThickLines).  cv2 is not available here, so PARITY IS UNPINNED against OpenCV itself; the rules are
pinned by closed-form cases in tests/test_annotate.py and compared with cv2 where it exists (tests/test_annotate_cv2.py).

Text stays on the host: the strings hold the smoothed values of the host's deques and need OpenCV's Hershey glyphs.  `text_items`
returns what the reference passes to cv2.putText, `put_text` draws it when cv2 is importable.  One deviation: the reference draws a
stitch's width label before the next stitch's markers, so a later marker can cover an earlier label; here all text comes last.

Text IN the picture on the device: `text_stamps` rasterises each item once on the host into a 1-bit stamp (cv2.putText where OpenCV
is installed, or any rasteriser the caller passes), libvti's vti_stamp paints the stamps onto the drawn pictures before they are
copied or encoded (process_frames(..., burn_text=True)); `stamp` is the numpy statement of what it paints.
"""
import math

import numpy as np

from . import polygons

XY_SHIFT = 16
XY_ONE = 1 << XY_SHIFT
_HALF = XY_ONE >> 1

# BGR, as the reference passes them to cv2 (config.py ROI_BORDER_COLOR; measurement.py:268, 272, 296, 360-364, 460-462, 499)
ROI_COLOUR = (144, 238, 144)
STITCH_BOX_COLOUR = (255, 255, 0)
FABRIC_BOX_COLOUR = (255, 0, 255)
ENVELOPE_COLOUR = (255, 128, 0)
WIDTH_COLOUR = (200, 200, 0)
CENTRE_COLOUR = (200, 0, 0)
DIST_COLOUR = (0, 255, 0)
EDGE_POINT_COLOUR = (255, 0, 255)
OUTLINE_COLOUR = (0, 0, 255)
COLOURS = (ROI_COLOUR, STITCH_BOX_COLOUR, FABRIC_BOX_COLOUR, ENVELOPE_COLOUR, WIDTH_COLOUR, CENTRE_COLOUR, DIST_COLOUR,
           OUTLINE_COLOUR)          # the eight distinct ones (the edge point shares the fabric box's)

OK, NO_FABRIC, NO_STITCHES, BAD_CAMERA = 0, 1, 2, 3
KEPT, MASK, SELECTED, NEAR, DIST, WIDTH = 1, 2, 4, 8, 16, 32
STATUS_OUTLINE = 1      # dev_status bit: the fabric outline needed more than max_points vertices (or the tracer hit its bound)


_DEFAULTS = dict(stitch_id=0, fabric_id=1, roi=(10, 300, 1270, 760), roi_enabled=True, drop_empty=False)    # config.py's


def _get(params, name):
    return params.get(name, _DEFAULTS[name]) if isinstance(params, dict) else getattr(params, name)


# ---- what is drawn ------------------------------------------------------------------------------------------------------
def roi_bounds(h, w, params):
    """measurement.py:220-238: the ROI clamped to the frame, None when disabled or degenerate."""
    if not _get(params, "roi_enabled"):
        return None
    r = _get(params, "roi")
    x_min, x_max = max(0, min(int(r[0]), w - 1)), max(0, min(int(r[2]), w - 1))
    y_min, y_max = max(0, min(int(r[1]), h - 1)), max(0, min(int(r[3]), h - 1))
    return (x_min, y_min, x_max, y_max) if x_min < x_max and y_min < y_max else None


def frame_bitmap(mask, h, w):
    """get_instance_mask_as_bitmap (measurement.py:70-86) without the None: the mask at the frame size (cv2.INTER_NEAREST)."""
    arr = np.asarray(mask)
    if arr.shape != (h, w):
        sh, sw = arr.shape
        ys = np.minimum(np.floor(np.arange(h) * (1.0 / (h / sh))).astype(np.int64), sh - 1)
        xs = np.minimum(np.floor(np.arange(w) * (1.0 / (w / sw))).astype(np.int64), sw - 1)
        arr = arr[ys][:, xs]
    return (arr > 0).astype(np.uint8)


def instance_keep(h, w, cls, xyxy, rows, params, live, nonempty):
    """Which instances the reference draws a box for (measurement.py:249-272): the ROI box-centre test on the int-truncated box and,
    with drop_empty, only instances whose mask as predict returns it is not empty.  A stitch with a per-slot row takes the answer
    vti_measure already gave (VTI_STITCH_KEPT).  -> bool [n], int boxes [n,4]."""
    n = len(cls)
    ib = np.trunc(np.asarray(xyxy, dtype=np.float64).reshape(-1, 4)).astype(np.int64)
    roi = roi_bounds(h, w, params)
    keep = np.ones(n, bool)
    for i in range(n):
        if roi is not None:
            sx, sy = ib[i, 0] + ib[i, 2], ib[i, 1] + ib[i, 3]
            keep[i] = 2 * roi[0] <= sx <= 2 * roi[2] and 2 * roi[1] <= sy <= 2 * roi[3]
        if _get(params, "drop_empty") and not (live[i] and nonempty[i]):
            keep[i] = False
        if int(cls[i]) == _get(params, "stitch_id") and live[i]:
            keep[i] = bool(int(rows["flags"][i]) & KEPT)
    return keep, ib


def display_list(h, w, cls, xyxy, masks_or_union, rows, params, live=None, nonempty=None, max_points=None, with_status=False):
    """The ordered primitives of measurement.py:219-504 for one h x w frame.
    cls [n], xyxy f32 [n,4] (frame px), in detection order.  masks_or_union: a list of the n masks as predict returns them (letterbox
    or frame size, None for a slot past the capacity), or the h x w union of the kept fabric masks (then `live` [n] says which
    instances have a slot, and with drop_empty `nonempty` [n] which masks have a set pixel).  rows: vti_measure's outputs for this
    frame: dict(status=frame_i32[b,0], flags [n], rank [n] (stitch_i32 of the frame's slots), f64 [n,7] (stitch_f64)); entries of
    instances without a slot are ignored.  params: MeasureParams (or a dict with stitch_id, fabric_id, roi, roi_enabled, drop_empty).
    max_points: vti_annotate's bound on the outline's vertices; when the outline needs more, step 8 is left out.
    -> [primitive] (with_status: and the status word), a primitive being one of
       ("rect", (x1, y1), (x2, y2), colour, thickness)   ("line", (x1, y1), (x2, y2), colour, thickness)
       ("circle", (cx, cy), radius, colour)  [filled]    ("polyline", int [n,2] (x, y), closed, colour, thickness)"""
    n = len(cls)
    status = int(rows["status"])
    done = lambda prims, word=0: (prims, word) if with_status else prims
    if status == BAD_CAMERA:
        return done([])
    union = None
    if isinstance(masks_or_union, np.ndarray) and masks_or_union.ndim == 2:      # the union (a list of masks is a list)
        union = (masks_or_union > 0).astype(np.uint8)
        live = np.ones(n, bool) if live is None else np.asarray(live, bool)
        nonempty = np.ones(n, bool) if nonempty is None else np.asarray(nonempty, bool)
    else:
        masks = list(masks_or_union)
        live = np.array([m is not None for m in masks], bool)
        nonempty = np.array([m is not None and np.count_nonzero(m) > 0 for m in masks], bool)
    prims = []
    # 1. the ROI (measurement.py:222-238)
    roi = roi_bounds(h, w, params)
    if roi is not None:
        prims.append(("rect", (roi[0], roi[1]), (roi[2], roi[3]), ROI_COLOUR, 2))
    # 2. boxes in detection order (measurement.py:249-272)
    keep, ib = instance_keep(h, w, cls, xyxy, rows, params, live, nonempty)
    stitch_id, fabric_id = _get(params, "stitch_id"), _get(params, "fabric_id")
    for i in range(n):
        if not keep[i]:
            continue
        box = tuple(int(v) for v in ib[i])
        if int(cls[i]) == stitch_id:
            prims.append(("rect", box[:2], box[2:], STITCH_BOX_COLOUR, 1))
        elif int(cls[i]) == fabric_id:
            prims.append(("rect", box[:2], box[2:], FABRIC_BOX_COLOUR, 2))
    # 3. no fabric: the reference returns here (measurement.py:280-287)
    if status == NO_FABRIC:
        return done(prims)
    if union is None:
        union = np.zeros((h, w), np.uint8)
        for i in range(n):
            if keep[i] and int(cls[i]) == fabric_id and masks[i] is not None:
                union |= frame_bitmap(masks[i], h, w)
    # 4. the lower envelope (measurement.py:289-296)
    rev = union[::-1] > 0
    has = rev.any(axis=0)
    env = np.where(has, h - 1 - np.argmax(rev, axis=0), -1)
    pts = [(x, int(env[x])) for x in range(w) if env[x] >= 0]
    if pts:
        step = max(1, len(pts) // 1000)
        prims.append(("polyline", np.array(pts[::step], dtype=np.int32).reshape(-1, 2), False, ENVELOPE_COLOUR, 2))
    # 5. no stitches (measurement.py:332-337)
    if status == NO_STITCHES:
        return done(prims)
    f64 = np.asarray(rows["f64"], dtype=np.float64).reshape(-1, 7)
    order = sorted((int(rows["rank"][i]), i) for i in range(n) if live[i] and int(rows["flags"][i]) & KEPT and int(rows["rank"][i]) >= 0)
    # 6. width markers of every stitch of stitch_meta, in its order (measurement.py:359-364)
    for _, i in order:
        cx, cy, left, right = (float(v) for v in f64[i, :4])
        a, b = (int(round(left)), int(round(cy))), (int(round(right)), int(round(cy)))
        prims += [("circle", a, 3, WIDTH_COLOUR), ("circle", b, 3, WIDTH_COLOUR), ("line", a, b, WIDTH_COLOUR, 1),
                  ("circle", (int(round(cx)), int(round(cy))), 3, CENTRE_COLOUR)]
    # 7. stitch-to-edge lines of the stitches that gave a distance (measurement.py:440-462)
    for _, i in order:
        if not int(rows["flags"][i]) & DIST:
            continue
        cx, cy, edge_y = float(f64[i, 0]), float(f64[i, 1]), float(f64[i, 5])
        e = (int(np.clip(int(round(cx)), 0, w - 1)), int(round(edge_y)))
        prims += [("line", e, (int(round(cx)), int(round(cy))), DIST_COLOUR, 1), ("circle", e, 2, EDGE_POINT_COLOUR)]
    # 8. the fabric outline (measurement.py:496-499)
    contours = polygons.find_external_contours(union)
    if max_points is not None and sum(len(c) for c in contours) > max_points:
        return done(prims, STATUS_OUTLINE)
    for c in contours:
        prims.append(("polyline", np.asarray(c, dtype=np.int32).reshape(-1, 2), True, OUTLINE_COLOUR, 2))
    return done(prims)


# ---- what the stitch-distance checker draws (Utils/check_stitch_distance.py:293-545) -----------------------------------------
CHECKER_CENTRE_COLOUR = (0, 255, 0)         # :510 (the distance line's green); the checker's outline is drawn in ENVELOPE_COLOUR (:545)
CHECKER_CENTRE_RADIUS = 4


def world_point_exists(u, v, K, dist, R, t):
    """Whether pixel_to_world_using_camera_plane (:477-503) returns a point for pixel (u, v): cv2.undistortPoints' five fixed-point
    steps (5-coefficient model), then |n . ray| >= 1e-9 with n = R[:, 2].  Float64 in the order libvti's pixel_to_world evaluates it
    (csrc/measure_dev.h), so host and device agree on the threshold to the last bit."""
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    k1, k2, p1, p2, k3 = (float(d) for d in np.asarray(dist, dtype=np.float64).ravel()[:5])
    ifx, ify = 1.0 / float(K[0, 0]), 1.0 / float(K[1, 1])
    x = (float(u) - float(K[0, 2])) * ifx
    y = (float(v) - float(K[1, 2])) * ify
    x0, y0 = x, y
    for _ in range(5):
        r2 = x * x + y * y
        icdist = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
        if icdist < 0:
            x, y = x0, y0
            break
        dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
        x, y = (x0 - dx) * icdist, (y0 - dy) * icdist
    denom = (float(R[0, 2]) * x + float(R[1, 2]) * y) + float(R[2, 2])
    return abs(denom) >= 1e-9


def checker_union(h, w, cls, xyxy, masks, params):
    """The checker's fabric union (:310-336, :344) as vti_measure_checker defines it, and which instances exist.  Per existing
    fabric instance: its mask at the frame size (cv2.INTER_NEAREST) when that has a set pixel, else the filled rectangle of its
    int-truncated box, corners inclusive, clipped to the frame.  With drop_empty an instance whose mask is None (a slot past the
    capacity) or empty as predict returns it does not exist.  -> (union u8 [h,w], exists bool [n], int boxes [n,4])."""
    n = len(cls)
    ib = np.trunc(np.asarray(xyxy, dtype=np.float64).reshape(-1, 4)).astype(np.int64)
    drop, fabric_id = bool(_get(params, "drop_empty")), int(_get(params, "fabric_id"))
    exists = np.array([not drop or (masks[i] is not None and np.count_nonzero(masks[i]) > 0) for i in range(n)], bool)
    union = np.zeros((h, w), np.uint8)
    for i in range(n):
        if not exists[i] or int(cls[i]) != fabric_id:
            continue
        bitmap = None if masks[i] is None else frame_bitmap(masks[i], h, w)
        if bitmap is not None and bitmap.any():
            union |= bitmap
            continue
        x1, y1, x2, y2 = (int(v) for v in ib[i])
        r0, r1, c0, c1 = max(min(y1, y2), 0), min(max(y1, y2), h - 1), max(min(x1, x2), 0), min(max(x1, x2), w - 1)
        if r0 <= r1 and c0 <= c1:
            union[r0:r1 + 1, c0:c1 + 1] = 1
    return union, exists, ib


def checker_display_list(h, w, cls, xyxy, masks, rows, params, max_points=None, with_status=False):
    """The ordered primitives of Utils/check_stitch_distance.py:293-545 for one h x w frame, in display_list's form: rasterise(frame,
    checker_display_list(...)) is the byte-for-byte specification of vti_annotate_checker's picture.
    cls [n], xyxy f32 [n,4] (frame px), in detection order.  masks: the n masks as predict returns them (letterbox or frame size;
    None for a slot past the capacity).  rows: vti_measure_checker's outputs for this frame: dict(status=frame_i32[b,0], flags [n],
    rank [n], f64 [n,7]); entries of instances without a slot are ignored (flags 0).  params: a CheckerParams (or a dict with
    stitch_id, fabric_id, drop_empty, K, dist, R, t).  max_points, with_status: as display_list.
    The order: a. a box per existing instance; b. [NO_FABRIC stops]; c. the upper envelope of the union; d. [NO_STITCHES stops];
    e. per stitch of the final set, in rank order: distance line and edge point, width ends and line, centroid; f. the outline."""
    n = len(cls)
    status = int(rows["status"])
    done = lambda prims, word=0: (prims, word) if with_status else prims
    if status not in (OK, NO_FABRIC, NO_STITCHES):
        return done([])
    masks = list(masks)
    stitch_id, fabric_id = int(_get(params, "stitch_id")), int(_get(params, "fabric_id"))
    union, exists, ib = checker_union(h, w, cls, xyxy, masks, params)
    prims = []
    # a. boxes in detection order (:323-336): no ROI, no keep test
    for i in range(n):
        if not exists[i]:
            continue
        box = tuple(int(v) for v in ib[i])
        if int(cls[i]) == stitch_id:
            prims.append(("rect", box[:2], box[2:], STITCH_BOX_COLOUR, 1))
        elif int(cls[i]) == fabric_id:
            prims.append(("rect", box[:2], box[2:], FABRIC_BOX_COLOUR, 2))
    # b. no fabric (:345-347)
    if status == NO_FABRIC:
        return done(prims)
    # c. the upper envelope (:349-360)
    has = union.any(axis=0)
    top = np.argmax(union > 0, axis=0)
    pts = [(x, int(top[x])) for x in range(w) if has[x]]
    if pts:
        step = max(1, len(pts) // 1000)
        prims.append(("polyline", np.array(pts[::step], dtype=np.int32).reshape(-1, 2), False, ENVELOPE_COLOUR, 2))
    # d. no stitches (:404-406)
    if status == NO_STITCHES:
        return done(prims)
    # e. the final set in rank order (:431-454, :465-510), as measure.checker_text_items derives it
    f64 = np.asarray(rows["f64"], dtype=np.float64).reshape(-1, 7)
    flags = [int(f) for f in rows["flags"]]
    order = [i for _, i in sorted((int(rows["rank"][i]), i) for i in range(n)
                                  if masks[i] is not None and flags[i] & KEPT and int(rows["rank"][i]) >= 0)]
    any_near = any(flags[i] & (SELECTED | NEAR) == SELECTED | NEAR for i in order)
    geom = tuple(params[name] if isinstance(params, dict) else getattr(params, name) for name in ("K", "dist", "R", "t"))
    for i in order:
        if not (flags[i] & SELECTED and (not any_near or flags[i] & NEAR)):
            continue
        cx, cy, left, right = (float(v) for v in f64[i, :4])
        centre = (int(round(cx)), int(round(cy)))
        if flags[i] & DIST:
            e = (int(np.clip(centre[0], 0, w - 1)), int(round(float(f64[i, 5]))))
            prims += [("line", e, centre, DIST_COLOUR, 1), ("circle", e, 2, EDGE_POINT_COLOUR)]
        # a width from the local-scale estimate (:500-507) sets WIDTH too but draws nothing: both ends need a world point
        if flags[i] & WIDTH and world_point_exists(left, cy, *geom) and world_point_exists(right, cy, *geom):
            a, b = (int(round(left)), centre[1]), (int(round(right)), centre[1])
            prims += [("circle", a, 3, WIDTH_COLOUR), ("circle", b, 3, WIDTH_COLOUR), ("line", a, b, WIDTH_COLOUR, 1)]
        prims.append(("circle", centre, CHECKER_CENTRE_RADIUS, CHECKER_CENTRE_COLOUR))
    # f. the outline of the same union (:543-545)
    contours = polygons.find_external_contours(union)
    if max_points is not None and sum(len(c) for c in contours) > max_points:
        return done(prims, STATUS_OUTLINE)
    for c in contours:
        prims.append(("polyline", np.asarray(c, dtype=np.int32).reshape(-1, 2), True, ENVELOPE_COLOUR, 2))
    return done(prims)


# ---- which pixels: OpenCV's drawing.cpp, LINE_8, shift = 0 ----------------------------------------------------------------
def _tdiv(a, b):
    """C's integer division (truncation towards zero)."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def clip_line(width, height, x1, y1, x2, y2):
    """cv::clipLine(Size2l, Point2l&, Point2l&): -> (visible, x1, y1, x2, y2).  The intersections are computed in double and
    truncated, as OpenCV does."""
    right, bottom = width - 1, height - 1
    if width <= 0 or height <= 0:
        return False, x1, y1, x2, y2
    c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8
    c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8
    if (c1 & c2) == 0 and (c1 | c2) != 0:
        if c1 & 12:
            a = 0 if c1 < 8 else bottom
            x1 += int(float(a - y1) * float(x2 - x1) / float(y2 - y1))
            y1 = a
            c1 = (x1 < 0) + (x1 > right) * 2
        if c2 & 12:
            a = 0 if c2 < 8 else bottom
            x2 += int(float(a - y2) * float(x2 - x1) / float(y2 - y1))
            y2 = a
            c2 = (x2 < 0) + (x2 > right) * 2
        if (c1 & c2) == 0 and (c1 | c2) != 0:
            if c1:
                a = 0 if c1 == 1 else right
                y1 += int(float(a - x1) * float(y2 - y1) / float(x2 - x1))
                x1 = a
                c1 = 0
            if c2:
                a = 0 if c2 == 1 else right
                y2 += int(float(a - x2) * float(y2 - y1) / float(x2 - x1))
                x2 = a
                c2 = 0
    return (c1 | c2) == 0, x1, y1, x2, y2


def _put(img, x, y, colour):
    if 0 <= x < img.shape[1] and 0 <= y < img.shape[0]:
        img[y, x] = colour


def _hline(img, y, x1, x2, colour):
    if x1 <= x2:
        img[y, x1:x2 + 1] = colour


def _line8(img, p1, p2, colour):
    """Line(): every pixel of LineIterator(img, pt1, pt2, 8, leftToRight=true)."""
    h, w = img.shape[:2]
    (x1, y1), (x2, y2) = p1, p2
    if not (0 <= x1 < w and 0 <= x2 < w and 0 <= y1 < h and 0 <= y2 < h):
        ok, x1, y1, x2, y2 = clip_line(w, h, x1, y1, x2, y2)
        if not ok:
            return
    dx, dy, sx, sy = x2 - x1, y2 - y1, 1, 1
    if dx < 0:                      # left to right
        dx, dy, x1, y1 = -dx, -dy, x2, y2
    if dy < 0:
        dy, sy = -dy, -1
    vert = dy > dx
    if vert:
        dx, dy = dy, dx
    err, plus, minus = dx - 2 * dy, 2 * dx, -2 * dy
    x, y = x1, y1
    for _ in range(dx + 1):
        img[y, x] = colour
        m = err < 0
        err += minus + (plus if m else 0)
        if vert:
            y += sy
            x += sx if m else 0
        else:
            x += sx
            y += sy if m else 0


def _line2(img, p1, p2, colour):
    """Line2(): the line between two 16.16 fixed-point points that FillConvexPoly outlines a polygon with."""
    h, w = img.shape[:2]
    ok, x1, y1, x2, y2 = clip_line(w << XY_SHIFT, h << XY_SHIFT, p1[0], p1[1], p2[0], p2[1])
    if not ok:
        return
    dx, dy = x2 - x1, y2 - y1
    ax, ay = abs(dx), abs(dy)
    if ax > ay:
        if dx < 0:
            dy, x1, y1, x2, y2 = -dy, x2, y2, x1, y1
        x_step, y_step = XY_ONE, _tdiv(dy * XY_ONE, ax | 1)
        ecount = (x2 - x1) >> XY_SHIFT
    else:
        if dy < 0:
            dx, x1, y1, x2, y2 = -dx, x2, y2, x1, y1
        x_step, y_step = _tdiv(dx * XY_ONE, ay | 1), XY_ONE
        ecount = (y2 - y1) >> XY_SHIFT
    x1 += _HALF
    y1 += _HALF
    _put(img, (x2 + _HALF) >> XY_SHIFT, (y2 + _HALF) >> XY_SHIFT, colour)
    if ax > ay:
        x1 >>= XY_SHIFT
        for _ in range(ecount + 1):
            _put(img, x1, y1 >> XY_SHIFT, colour)
            x1 += 1
            y1 += y_step
    else:
        y1 >>= XY_SHIFT
        for _ in range(ecount + 1):
            _put(img, x1 >> XY_SHIFT, y1, colour)
            x1 += x_step
            y1 += 1


def _fill_convex(img, v, colour):
    """FillConvexPoly(img, v, npts, colour, LINE_8, shift = XY_SHIFT): the outline by Line2, then one span per scanline between the
    two edge chains that start at the top-most vertex."""
    h, w = img.shape[:2]
    n = len(v)
    xmin = xmax = v[0][0]
    ymin = ymax = v[0][1]
    imin = 0
    p0 = v[n - 1]
    for i, p in enumerate(v):
        if p[1] < ymin:
            ymin, imin = p[1], i
        ymax, xmax, xmin = max(ymax, p[1]), max(xmax, p[0]), min(xmin, p[0])
        _line2(img, p0, p, colour)
        p0 = p
    xmin, xmax = (xmin + _HALF) >> XY_SHIFT, (xmax + _HALF) >> XY_SHIFT
    ymin, ymax = (ymin + _HALF) >> XY_SHIFT, (ymax + _HALF) >> XY_SHIFT
    if n < 3 or xmax < 0 or ymax < 0 or xmin >= w or ymin >= h:
        return
    ymax = min(ymax, h - 1)
    e_idx, e_ye, e_di, e_x, e_dx = [imin, imin], [ymin, ymin], [1, n - 1], [-XY_ONE, -XY_ONE], [0, 0]
    edges, y = n, ymin
    while True:
        for i in (0, 1):
            if y >= e_ye[i]:
                idx0, di = e_idx[i], e_di[i]
                idx = idx0 + di
                if idx >= n:
                    idx -= n
                while True:
                    edges -= 1
                    if edges < 0:               # `for (; edges-- > 0; )` ran out
                        break
                    ty = (v[idx][1] + _HALF) >> XY_SHIFT
                    if ty > y:
                        xs, xe = v[idx0][0], v[idx][0]
                        e_ye[i], e_dx[i], e_x[i], e_idx[i] = ty, _tdiv((xe - xs) * 2 + (ty - y), 2 * (ty - y)), xs, idx
                        break
                    idx0 = idx
                    idx += di
                    if idx >= n:
                        idx -= n
        if edges < 0:
            break
        if y >= 0:
            left, right = (1, 0) if e_x[0] > e_x[1] else (0, 1)
            xx1, xx2 = (e_x[left] + _HALF) >> XY_SHIFT, (e_x[right] + _HALF) >> XY_SHIFT
            if xx2 >= 0 and xx1 < w:
                _hline(img, y, max(xx1, 0), min(xx2, w - 1), colour)
        e_x[0] += e_dx[0]
        e_x[1] += e_dx[1]
        y += 1
        if y > ymax:
            break


def circle_spans(radius):
    """Circle()'s midpoint walk: [(dy, half_width)] -- the rows cy -+ dy are filled over [cx - half_width, cx + half_width]."""
    spans = []
    err, dx, dy, plus, minus = 0, radius, 0, 1, (radius << 1) - 1
    while dx >= dy:
        spans += [(dy, dx), (dx, dy)]
        dy += 1
        err += plus
        plus += 2
        if err > 0:
            err -= minus
            dx -= 1
            minus -= 2
    return spans


def _circle(img, centre, radius, colour):
    """Circle(img, centre, radius, colour, fill = 1), clipped to the image."""
    h, w = img.shape[:2]
    cx, cy = centre
    for dy, hw in circle_spans(radius):
        x1, x2 = max(cx - hw, 0), min(cx + hw, w - 1)
        for y in (cy - dy, cy + dy):
            if 0 <= y < h:
                _hline(img, y, x1, x2, colour)


def _thick_line(img, p0, p1, colour, thickness, flags=3):
    """ThickLine(img, p0, p1, colour, thickness, LINE_8, flags, shift = 0); flags: 1 = a round cap at p0, 2 = at p1."""
    if thickness <= 1:
        _line8(img, p0, p1, colour)
        return
    x0, y0, x1, y1 = p0[0] << XY_SHIFT, p0[1] << XY_SHIFT, p1[0] << XY_SHIFT, p1[1] << XY_SHIFT
    dx, dy = (x0 - x1) * (1.0 / XY_ONE), (y1 - y0) * (1.0 / XY_ONE)
    r = dx * dx + dy * dy
    odd = thickness & 1
    th = thickness << (XY_SHIFT - 1)
    if abs(r) > 2.220446049250313e-16:
        r = (th + odd * XY_ONE * 0.5) / math.sqrt(r)
        dpx, dpy = int(round(dy * r)), int(round(dx * r))       # cvRound: half to even, as Python's round
        _fill_convex(img, [(x0 + dpx, y0 + dpy), (x0 - dpx, y0 - dpy), (x1 - dpx, y1 - dpy), (x1 + dpx, y1 + dpy)], colour)
    for k, (x, y) in enumerate(((x0, y0), (x1, y1))):
        if flags & (k + 1):
            _circle(img, ((x + _HALF) >> XY_SHIFT, (y + _HALF) >> XY_SHIFT), (th + _HALF) >> XY_SHIFT, colour)


def _poly_line(img, pts, closed, colour, thickness):
    """PolyLine(): the edges as ThickLines, a cap at the end of each (and at the start of an open one)."""
    n = len(pts)
    if n == 0:
        return
    flags = 2 + (not closed)
    p0 = pts[n - 1] if closed else pts[0]
    for i in range(0 if closed else 1, n):
        _thick_line(img, p0, pts[i], colour, thickness, flags)
        p0, flags = pts[i], 2


def rasterise(frame, primitives):
    """-> a copy of the BGR frame with the primitives painted in list order (a later one overwrites an earlier one)."""
    img = np.array(frame, dtype=np.uint8, copy=True)
    for p in primitives:
        kind = p[0]
        if kind == "line":
            _thick_line(img, tuple(map(int, p[1])), tuple(map(int, p[2])), p[3], p[4])
        elif kind == "rect":        # cv::rectangle with thickness >= 0: the closed polyline of its corners
            (x1, y1), (x2, y2) = (tuple(map(int, p[1])), tuple(map(int, p[2])))
            _poly_line(img, [(x1, y1), (x2, y1), (x2, y2), (x1, y2)], True, p[3], p[4])
        elif kind == "circle":
            _circle(img, tuple(map(int, p[1])), int(p[2]), p[3])
        elif kind == "polyline":
            _poly_line(img, [(int(x), int(y)) for x, y in np.asarray(p[1]).reshape(-1, 2)], bool(p[2]), p[3], p[4])
        else:
            raise ValueError(f"unknown primitive {kind!r}")
    return img


# ---- text (host) --------------------------------------------------------------------------------------------------------
FONT = "FONT_HERSHEY_SIMPLEX"


def text_items(record, rows, h, min_stitches=3):
    """What the reference passes to cv2.putText for one frame: [(text, org, fontFace name, scale, colour, thickness)].
    record: the frame's record (StitchMeasurer / MultiCameraMeasurer), whose values are the smoothed ones; rows: dict(status,
    n_stitch, n_fabric, n_dist, n_width (frame_i32[b,0], [1], [2], [4], [5]), flags [n], rank [n], f64 [n,7]) of the frame's slots."""
    status = int(rows["status"])
    if status == NO_FABRIC:
        return [("Fabric not detected", (10, 55), FONT, 0.7, (0, 0, 255), 2)]
    if status == NO_STITCHES:
        return [("No stitches detected", (10, 55), FONT, 0.7, (0, 0, 255), 2)]
    if status != OK:
        return []
    items = []
    f64 = np.asarray(rows["f64"], dtype=np.float64).reshape(-1, 7)
    order = sorted((int(r), i) for i, r in enumerate(rows["rank"]) if int(rows["flags"][i]) & KEPT and int(r) >= 0)
    last = None
    for _, i in order:              # measurement.py:365-368: the label shows all_widths[-1], the last width computed so far
        if int(rows["flags"][i]) & WIDTH:
            last = float(f64[i, 4])
        if last is not None:
            items.append((f"{last:.1f}", (int(round(float(f64[i, 0]))) + 2, int(round(float(f64[i, 1]))) - 20), FONT, 0.60,
                          (0, 0, 0), 2))
    sd, sw = record.get("edge_distance_mm"), record.get("stitch_width_mm")
    n_d, n_w = int(rows["n_dist"]), int(rows["n_width"])
    if sd is not None and sw is not None:
        info = f"Edge Dist: {sd:.2f}mm | Avg Width: {sw:.2f}mm (n_d={n_d}, n_w={n_w})"
    elif sd is not None:
        info = f"Edge Distance: {sd:.2f}mm (n={n_d})"
    elif sw is not None:
        info = f"Avg Width: {sw:.2f}mm (n={n_w})"
    else:
        info = f"Insufficient stitches (dist={n_d}, width={n_w}, need {int(min_stitches)})"
    items.append((info, (10, 30), FONT, 0.7, (0, 0, 255), 2))
    items.append((f"Stitches: {int(rows['n_stitch'])} | Fabric: {int(rows['n_fabric'])}", (10, h - 10), FONT, 0.5, (0, 0, 0), 1))
    return items


def put_text(img, items):
    """cv2.putText for every item of text_items(), in place.  Raises ImportError where OpenCV is not installed."""
    import cv2
    for text, org, face, scale, colour, thickness in items:
        cv2.putText(img, text, org, getattr(cv2, face), scale, colour, thickness)
    return img


# ---- text as 1-bit stamps: what vti_stamp paints ------------------------------------------------------------------------------
_CANVASES = {}          # (h, w) -> the zero uint8 canvas of that frame size (the 4 latest sizes)


def cv2_rasterise(canvas, item):
    """The default rasteriser of text_stamps: the item drawn with cv2.putText, default line type, in 255.  ImportError without OpenCV."""
    import cv2
    text, org, face, scale, _, thickness = item
    cv2.putText(canvas, text, org, getattr(cv2, face), scale, 255, thickness)


def text_stamps(items, h, w, rasterise=None):
    """The items of text_items / checker_text_items (and any further ones of the same form) for one picture of h x w, each as a
    stamp (x, y, bits, colour): bits bool [bh, bw] with its top-left corner at picture pixel (x, y), colour the item's BGR triple.
    `rasterise(canvas, item)` draws the item in any non-zero value onto a zero uint8 [h, w] canvas -- the size of the picture, so that
    it clips exactly as it would on the picture; the stamp is the bounding box of what it drew, and an item that drew nothing gives no
    stamp.  Default: cv2_rasterise (ImportError where OpenCV is not installed, as put_text).  The pixel set of putText with the
    default line type does not depend on the picture under it, so stamp(picture, text_stamps(items, h, w)) is put_text(picture,
    items).  One canvas is kept per frame size and cleared only where an item drew."""
    if rasterise is None:
        import cv2  # noqa: F401  (the ImportError comes before anything is drawn)
        rasterise = cv2_rasterise
    h, w = int(h), int(w)
    canvas = _CANVASES.pop((h, w), None)
    if canvas is None:
        canvas = np.zeros((h, w), np.uint8)
        while len(_CANVASES) >= 4:
            del _CANVASES[next(iter(_CANVASES))]
    _CANVASES[(h, w)] = canvas
    stamps = []
    try:
        for item in items:
            rasterise(canvas, item)
            rows = np.flatnonzero(canvas.any(axis=1))
            if rows.size == 0:
                continue
            y0, y1 = int(rows[0]), int(rows[-1]) + 1
            cols = np.flatnonzero(canvas[y0:y1].any(axis=0))
            x0, x1 = int(cols[0]), int(cols[-1]) + 1
            box = canvas[y0:y1, x0:x1]
            stamps.append((x0, y0, box != 0, tuple(int(v) for v in item[4][:3])))
            box[...] = 0
    except BaseException:
        canvas[...] = 0         # a rasteriser that raised may have drawn: the kept canvas is zero again
        raise
    return stamps


def stamp(picture, stamps):
    """The specification of vti_stamp, in place: for every stamp (x, y, bits, colour) in list order, picture[y + r, x + c] = colour
    wherever bits[r, c] is set (a later stamp overwrites an earlier one).  picture: uint8 [h, w, 3]; a stamp lies inside it.
    -> picture."""
    for x, y, bits, colour in stamps:
        bits = np.asarray(bits, dtype=bool)
        bh, bw = bits.shape
        if x < 0 or y < 0 or y + bh > picture.shape[0] or x + bw > picture.shape[1]:
            raise ValueError(f"stamp: a {bh} x {bw} stamp at ({x}, {y}) is not inside the {picture.shape[0]} x {picture.shape[1]} picture")
        picture[y:y + bh, x:x + bw][bits] = colour
    return picture
