"""annotate.checker_display_list -- the host specification of vti_annotate_checker's picture (Utils/check_stitch_distance.py:293-545)
-- on small hand-made frames.  Every expected primitive list is written out by hand from the checker's text; the builder is never
asked what it should return.  No GPU and no library call; the device is compared with the same builder in
tests/test_gpu_annotate_checker.py."""
import numpy as np

from test_checker_ref import degenerate_calib
from test_oracle_geometry import load_calib
from vti_amd import annotate as A

H, W = 48, 64
CALIB = load_calib()
CYAN, MAGENTA, ORANGE, GREEN, OLIVE = (255, 255, 0), (255, 0, 255), (255, 128, 0), (0, 255, 0), (200, 200, 0)
KEPT, MASK, SELECTED, NEAR, DIST, WIDTH = 1, 2, 4, 8, 16, 32
ALL = KEPT | MASK | SELECTED | NEAR | DIST | WIDTH
NAN = float("nan")


def params(calib=CALIB, **kw):
    return dict(dict(stitch_id=0, fabric_id=1, drop_empty=False, K=calib[0], dist=calib[1], R=calib[2], t=calib[3]), **kw)


def rect_mask(y0, y1, x0, x1):
    """rows y0..y1, columns x0..x1, all inclusive"""
    m = np.zeros((H, W), np.uint8)
    m[y0:y1 + 1, x0:x1 + 1] = 1
    return m


def rows_of(status, per_instance):
    """per_instance: None (not a stitch: flags 0, rank -1) or (flags, rank, cx, cy, left, right, width, edge_y, dist)."""
    n = len(per_instance)
    flags, rank, f64 = np.zeros(n, np.int32), np.full(n, -1, np.int32), np.full((n, 7), np.nan)
    for i, r in enumerate(per_instance):
        if r is not None:
            flags[i], rank[i], f64[i] = r[0], r[1], r[2:]
    return dict(status=status, flags=flags, rank=rank, f64=f64)


def same(got, want):
    """Two primitive lists, entry by entry (point arrays by value)."""
    assert len(got) == len(want), (len(got), len(want), [p[0] for p in got])
    for k, (g, e) in enumerate(zip(got, want)):
        assert g[0] == e[0], (k, g, e)
        if g[0] == "polyline":
            assert np.asarray(g[1]).reshape(-1, 2).tolist() == [list(p) for p in e[1]], (k, np.asarray(g[1]).tolist(), e[1])
            assert (bool(g[2]), tuple(g[3]), g[4]) == (e[2], e[3], e[4]), (k, g[2:], e[2:])
        else:
            assert tuple(g[1:]) == tuple(e[1:]), (k, g, e)


# ---- the scene of the order test: one fabric, four stitches -------------------------------------------------------------------
FABRIC = rect_mask(12, 39, 5, 58)                   # a flat top edge on row 12
CLS = np.array([1, 0, 0, 0, 0])
BOXES = np.array([[4.7, 10.2, 59.9, 40.5], [10.9, 20.1, 14.2, 23.8], [30.0, 20.0, 34.0, 24.0], [40.2, 33.3, 44.4, 36.6],
                  [47.9, 28.0, 53.9, 33.9]], np.float32)
MASKS = [FABRIC, rect_mask(20, 23, 11, 14), rect_mask(20, 24, 30, 34), rect_mask(33, 36, 40, 44), rect_mask(28, 33, 48, 53)]
ROWS = [None,
        (ALL, 0, 12.5, 21.5, 11.0, 14.0, 1.0, 12.0, 2.0),                            # round(12.5) = 12, round(21.5) = 22: half to even
        (KEPT | MASK | SELECTED, 1, 32.0, 22.0, 30.0, 34.0, NAN, NAN, NAN),          # selected, not near: outside the final set
        (KEPT | MASK | NEAR, 2, 42.0, 34.5, 40.0, 44.0, NAN, NAN, NAN),              # near, not selected: outside it too
        (KEPT | MASK | SELECTED | NEAR | WIDTH, 3, 50.4, 30.6, 48.0, 53.0, 1.5, NAN, NAN)]      # no distance
BOX_PRIMS = [("rect", (4, 10), (59, 40), MAGENTA, 2), ("rect", (10, 20), (14, 23), CYAN, 1), ("rect", (30, 20), (34, 24), CYAN, 1),
             ("rect", (40, 33), (44, 36), CYAN, 1), ("rect", (47, 28), (53, 33), CYAN, 1)]
ENVELOPE = ("polyline", [(x, 12) for x in range(5, 59)], False, ORANGE, 2)
OUTLINE = ("polyline", [(5, 12), (5, 39), (58, 39), (58, 12)], True, ORANGE, 2)    # CHAIN_APPROX_SIMPLE: the four corners, down first
STITCH_1 = [("line", (12, 12), (12, 22), GREEN, 1), ("circle", (12, 12), 2, MAGENTA),
            ("circle", (11, 22), 3, OLIVE), ("circle", (14, 22), 3, OLIVE), ("line", (11, 22), (14, 22), OLIVE, 1),
            ("circle", (12, 22), 4, GREEN)]
STITCH_4 = [("circle", (48, 31), 3, OLIVE), ("circle", (53, 31), 3, OLIVE), ("line", (48, 31), (53, 31), OLIVE, 1),
            ("circle", (50, 31), 4, GREEN)]


def test_the_order_of_boxes_envelope_markers_and_outline():
    got, word = A.checker_display_list(H, W, CLS, BOXES, MASKS, rows_of(A.OK, ROWS), params(), with_status=True)
    same(got, BOX_PRIMS + [ENVELOPE] + STITCH_1 + STITCH_4 + [OUTLINE])
    assert word == 0


def test_both_early_stops():
    same(A.checker_display_list(H, W, CLS, BOXES, MASKS, rows_of(A.NO_FABRIC, ROWS), params()), BOX_PRIMS)
    same(A.checker_display_list(H, W, CLS, BOXES, MASKS, rows_of(A.NO_STITCHES, ROWS), params()), BOX_PRIMS + [ENVELOPE])
    assert A.checker_display_list(H, W, CLS, BOXES, MASKS, rows_of(A.BAD_CAMERA, ROWS), params()) == []     # a plain copy


def test_an_empty_mask_fabric_joins_the_union_with_its_filled_box():
    """(int 40, int 2) .. (int 70, int 6), corners inclusive, clipped to columns 40..63: in the envelope and in the outline.  A slot
    past the capacity (mask None) is the same empty mask."""
    cls, boxes = np.array([1]), np.array([[40.9, 2.3, 70.5, 6.9]], np.float32)
    want = [("rect", (40, 2), (70, 6), MAGENTA, 2), ("polyline", [(x, 2) for x in range(40, 64)], False, ORANGE, 2)]
    for mask in (np.zeros((H, W), np.uint8), None):
        got = A.checker_display_list(H, W, cls, boxes, [mask], rows_of(A.NO_STITCHES, [None]), params())
        same(got, want)
    # with a stitch, status OK: the outline is the box's
    cls, boxes = np.array([1, 0]), np.array([[40.9, 2.3, 70.5, 6.9], [50.0, 10.0, 52.0, 12.0]], np.float32)
    rows = rows_of(A.OK, [None, (KEPT | MASK | SELECTED, 0, 51.0, 11.0, 50.0, 52.0, NAN, NAN, NAN)])
    got = A.checker_display_list(H, W, cls, boxes, [np.zeros((H, W), np.uint8), rect_mask(10, 12, 50, 52)], rows, params())
    same(got, [want[0], ("rect", (50, 10), (52, 12), CYAN, 1), want[1], ("circle", (51, 11), 4, GREEN),
               ("polyline", [(40, 2), (40, 6), (63, 6), (63, 2)], True, ORANGE, 2)])
    # next to a real mask the box widens the union: one contour, the mask's rows 12..39 and the box's rows 30..45 right of it
    cls, boxes = np.array([1, 1]), np.array([[5.0, 12.0, 20.0, 39.0], [21.0, 30.0, 25.0, 45.0]], np.float32)
    got = A.checker_display_list(H, W, cls, boxes, [rect_mask(12, 39, 5, 20), np.zeros((H, W), np.uint8)],
                                 rows_of(A.NO_STITCHES, [None, None]), params())
    same(got[2:], [("polyline", [(x, 12) for x in range(5, 21)] + [(x, 30) for x in range(21, 26)], False, ORANGE, 2)])


def test_the_final_set_is_every_selected_stitch_when_none_is_near():
    rows = [None, (KEPT | MASK | SELECTED | WIDTH, 0, 12.5, 21.5, 11.0, 14.0, 1.0, NAN, NAN),
            (KEPT | MASK | SELECTED, 1, 32.0, 22.0, 30.0, 34.0, NAN, NAN, NAN),
            (KEPT | MASK | NEAR, 2, 42.0, 34.5, 40.0, 44.0, NAN, NAN, NAN),          # near but not selected: it does not count
            (KEPT | MASK, 3, 50.4, 30.6, 48.0, 53.0, NAN, NAN, NAN)]
    got = A.checker_display_list(H, W, CLS, BOXES, MASKS, rows_of(A.OK, rows), params())
    same(got, BOX_PRIMS + [ENVELOPE] + STITCH_1[2:] + [("circle", (32, 22), 4, GREEN)] + [OUTLINE])


def test_a_width_from_the_estimate_draws_the_centroid_and_no_width_markers():
    """test_checker_ref's calibration: n . ray = (u - K02) / fx, exactly 0 on column K02.  With K02 on the stitch's left end,
    world(left, cy) does not exist, so the checker takes the local-scale estimate (:500-507): VTI_STITCH_WIDTH without markers."""
    calib = degenerate_calib(11.0)
    assert not A.world_point_exists(11.0, 21.5, *calib) and A.world_point_exists(14.0, 21.5, *calib)
    assert A.world_point_exists(11.0 + 1e-6, 21.5, *calib) and not A.world_point_exists(11.0 + 1e-8, 21.5, *calib)      # |x| / 100 vs 1e-9
    got = A.checker_display_list(H, W, CLS, BOXES, MASKS, rows_of(A.OK, ROWS), params(calib))
    same(got, BOX_PRIMS + [ENVELOPE] + STITCH_1[:2] + STITCH_1[5:] + STITCH_4 + [OUTLINE])
    # K02 on the right end instead: the same
    got = A.checker_display_list(H, W, CLS, BOXES, MASKS, rows_of(A.OK, ROWS), params(degenerate_calib(14.0)))
    same(got, BOX_PRIMS + [ENVELOPE] + STITCH_1[:2] + STITCH_1[5:] + STITCH_4 + [OUTLINE])


def test_the_radius_four_circle_against_a_hand_listed_span_table():
    """cv::Circle's midpoint walk for r = 4: (dx, dy) = (4, 0), (3, 1), (3, 2) -- half widths 0, 2, 3, 3, 4, 3, 3, 2, 0."""
    half = {-4: 0, -3: 2, -2: 3, -1: 3, 0: 4, 1: 3, 2: 3, 3: 2, 4: 0}
    frame = np.zeros((H, W, 3), np.uint8)
    img = A.rasterise(frame, [("circle", (20, 10), 4, GREEN)])
    want = np.zeros((H, W), bool)
    for dy, hw in half.items():
        want[10 + dy, 20 - hw:20 + hw + 1] = True
    assert np.array_equal((img == GREEN).all(axis=-1), want) and (img[~want] == 0).all()
    # clipped by the frame's corner
    img = A.rasterise(frame, [("circle", (1, 46), 4, GREEN)])
    want = np.zeros((H, W), bool)
    for dy, hw in half.items():
        if 46 + dy < H:
            want[46 + dy, max(1 - hw, 0):1 + hw + 1] = True
    assert np.array_equal((img == GREEN).all(axis=-1), want)


def test_drop_empty_removes_the_box_of_an_instance_that_does_not_exist():
    cls = np.array([1, 0, 1, 0])
    boxes = np.array([[4.7, 10.2, 59.9, 40.5], [10.0, 20.0, 14.0, 23.0], [40.9, 2.3, 70.5, 6.9], [30.0, 20.0, 34.0, 24.0]], np.float32)
    masks = [FABRIC, np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8), None]
    rows = rows_of(A.NO_STITCHES, [None] * 4)
    # without drop_empty every instance has its box, and the empty fabric its filled rectangle (the envelope's columns 40..58 rise to row 2)
    got = A.checker_display_list(H, W, cls, boxes, masks, rows, params())
    same(got, [("rect", (4, 10), (59, 40), MAGENTA, 2), ("rect", (10, 20), (14, 23), CYAN, 1), ("rect", (40, 2), (70, 6), MAGENTA, 2),
               ("rect", (30, 20), (34, 24), CYAN, 1),
               ("polyline", [(x, 12) for x in range(5, 40)] + [(x, 2) for x in range(40, 64)], False, ORANGE, 2)])
    # with it: the empty stitch, the empty fabric and the instance past the capacity are gone, boxes and rectangle alike
    got = A.checker_display_list(H, W, cls, boxes, masks, rows, params(drop_empty=True))
    same(got, [("rect", (4, 10), (59, 40), MAGENTA, 2), ENVELOPE])


def test_the_picture_differs_from_process_frames():
    """The same instances and rows through display_list (process_frame's overlay, ROI off): the other envelope, other markers,
    another outline colour."""
    frame = np.full((H, W, 3), 7, np.uint8)
    rows = rows_of(A.OK, ROWS)
    ours = A.rasterise(frame, A.checker_display_list(H, W, CLS, BOXES, MASKS, rows, params()))
    theirs = A.rasterise(frame, A.display_list(H, W, CLS, BOXES, MASKS, rows, dict(roi_enabled=False)))
    assert not np.array_equal(ours, theirs)
    assert (ours[12, 20] == ORANGE).all() and (theirs[39, 20] == (0, 0, 255)).all() and (ours[39, 20] == ORANGE).all()
    assert (ours[22, 13] == GREEN).all() and (theirs[22, 13] == (200, 0, 0)).all()          # the centroids: r = 4 green, r = 3 blue
    assert (ours[22, 28] == 7).all() and (theirs[22, 28] == OLIVE).all()                   # stitch 2 is outside the checker's final set


def test_max_points_too_small_leaves_the_outline_out_and_sets_the_status_word():
    got, word = A.checker_display_list(H, W, CLS, BOXES, MASKS, rows_of(A.OK, ROWS), params(), max_points=3, with_status=True)
    same(got, BOX_PRIMS + [ENVELOPE] + STITCH_1 + STITCH_4)
    assert word == A.STATUS_OUTLINE
    got, word = A.checker_display_list(H, W, CLS, BOXES, MASKS, rows_of(A.OK, ROWS), params(), max_points=4, with_status=True)
    assert word == 0 and len(got) == len(BOX_PRIMS) + 12
