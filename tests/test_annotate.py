"""annotate.py, the host specification of vti_annotate, without a GPU: the raster rules on shapes whose OpenCV answer is known in
closed form, the display list's order and content on hand scenes, both early stops, the exact text strings, painter's order -- and
that the scenes tests/test_gpu_annotate.py compares the device on exercise every part of the overlay (a GPU test that compares two
plain copies would pass vacuously)."""
import numpy as np
import pytest

import annotate_util as U
import measure_ref as mr
from vti_amd import annotate as A

ONE = (1, 1, 1)


def _paint(h, w, prims):
    return A.rasterise(np.zeros((h, w, 3), np.uint8), prims)[:, :, 0]


def _set(img):
    return {(int(x), int(y)) for y, x in zip(*np.nonzero(img))}


# ---- raster rules ---------------------------------------------------------------------------------------------------------
def test_axis_aligned_thin_lines_are_their_pixel_runs():
    assert _set(_paint(10, 12, [("line", (2, 3), (9, 3), ONE, 1)])) == {(x, 3) for x in range(2, 10)}
    assert _set(_paint(10, 12, [("line", (9, 3), (2, 3), ONE, 1)])) == {(x, 3) for x in range(2, 10)}
    assert _set(_paint(10, 12, [("line", (4, 8), (4, 1), ONE, 1)])) == {(4, y) for y in range(1, 9)}


def test_diagonal_thin_lines_step_both_axes_every_pixel():
    assert _set(_paint(10, 12, [("line", (1, 2), (7, 8), ONE, 1)])) == {(1 + k, 2 + k) for k in range(7)}
    assert _set(_paint(10, 12, [("line", (7, 2), (1, 8), ONE, 1)])) == {(7 - k, 2 + k) for k in range(7)}


def test_a_zero_length_line_is_one_pixel_and_outside_the_frame_nothing():
    assert _set(_paint(6, 6, [("line", (3, 2), (3, 2), ONE, 1)])) == {(3, 2)}
    assert _set(_paint(6, 6, [("line", (7, 2), (7, 2), ONE, 1)])) == set()
    assert _set(_paint(6, 6, [("line", (-3, -1), (-1, -4), ONE, 1)])) == set()


def test_lines_are_clipped_at_the_borders():
    assert _set(_paint(8, 10, [("line", (-5, 4), (20, 4), ONE, 1)])) == {(x, 4) for x in range(10)}
    assert _set(_paint(8, 10, [("line", (6, -3), (6, 30), ONE, 1)])) == {(6, y) for y in range(8)}
    # a 45-degree line through the corner region: the clipped segment lies on the same diagonal
    assert _set(_paint(8, 10, [("line", (-3, -1), (12, 14), ONE, 1)])) == {(x, x + 2) for x in range(0, 6)}
    # a rectangle that touches x = W (a box clipped to the frame by scale_boxes): its right edge is outside, the rest is drawn
    got = _set(_paint(8, 10, [("rect", (4, 2), (10, 6), ONE, 1)]))
    assert got == {(x, 2) for x in range(4, 10)} | {(x, 6) for x in range(4, 10)} | {(4, y) for y in range(2, 7)}


def test_a_thin_rectangle_is_its_four_borders():
    got = _set(_paint(12, 12, [("rect", (2, 3), (8, 9), ONE, 1)]))
    assert got == ({(x, 3) for x in range(2, 9)} | {(x, 9) for x in range(2, 9)} | {(2, y) for y in range(3, 10)} |
                   {(8, y) for y in range(3, 10)})


def test_filled_circles_are_the_midpoint_spans():
    assert _set(_paint(9, 9, [("circle", (4, 4), 0, ONE)])) == {(4, 4)}
    assert _set(_paint(9, 9, [("circle", (4, 4), 1, ONE)])) == {(4, 4), (3, 4), (5, 4), (4, 3), (4, 5)}
    half = {0: 3, 1: 2, 2: 2, 3: 0}            # radius 3: half width per |dy|
    assert _set(_paint(9, 9, [("circle", (4, 4), 3, ONE)])) == {(4 + dx, 4 + dy) for dy in range(-3, 4)
                                                                for dx in range(-half[abs(dy)], half[abs(dy)] + 1)}
    assert A.circle_spans(2) == [(0, 2), (2, 0), (1, 1), (1, 1)]
    # clipped to the frame
    assert _set(_paint(9, 9, [("circle", (0, 8), 1, ONE)])) == {(0, 8), (1, 8), (0, 7)}
    assert _set(_paint(9, 9, [("circle", (-4, 3), 3, ONE)])) == set()


def test_a_thick_horizontal_line_is_three_rows_with_round_ends():
    got = _paint(9, 14, [("line", (2, 4), (10, 4), ONE, 2)])
    rows = {y: sorted(np.nonzero(got[y])[0].tolist()) for y in range(9) if got[y].any()}
    assert rows == {3: list(range(2, 11)), 4: list(range(1, 12)), 5: list(range(2, 11))}
    # thickness 2, zero length: the two end caps (radius 1) only
    assert _set(_paint(9, 9, [("line", (4, 4), (4, 4), ONE, 2)])) == {(4, 4), (3, 4), (5, 4), (4, 3), (4, 5)}
    # an open polyline of one point draws nothing (PolyLine's loop is empty); a closed one draws its cap
    assert _set(_paint(9, 9, [("polyline", np.array([[4, 4]]), False, ONE, 2)])) == set()
    assert _set(_paint(9, 9, [("polyline", np.array([[4, 4]]), True, ONE, 2)])) == {(4, 4), (3, 4), (5, 4), (4, 3), (4, 5)}


def test_thick_lines_are_symmetric_under_the_frames_symmetries():
    """A thick vertical line is the transpose of the horizontal one; reversing the end points changes nothing."""
    hor = _paint(15, 15, [("line", (3, 7), (11, 7), ONE, 2)])
    ver = _paint(15, 15, [("line", (7, 3), (7, 11), ONE, 2)])
    assert np.array_equal(hor.T, ver)
    assert np.array_equal(hor, _paint(15, 15, [("line", (11, 7), (3, 7), ONE, 2)]))


def test_a_later_primitive_overwrites_an_earlier_one():
    a, b = (10, 20, 30), (200, 100, 50)
    img = A.rasterise(np.zeros((9, 9, 3), np.uint8), [("circle", (4, 4), 3, a), ("line", (0, 4), (8, 4), b, 1)])
    assert tuple(img[4, 4]) == b and tuple(img[3, 4]) == a and tuple(img[4, 0]) == b
    img = A.rasterise(np.zeros((9, 9, 3), np.uint8), [("line", (0, 4), (8, 4), b, 1), ("circle", (4, 4), 3, a)])
    assert tuple(img[4, 4]) == a and tuple(img[4, 0]) == b
    src = np.full((5, 5, 3), 7, np.uint8)
    out = A.rasterise(src, [])
    assert np.array_equal(out, src) and out is not src


def test_clip_line_matches_the_exact_intersections_on_easy_cases():
    assert A.clip_line(10, 8, -5, 4, 20, 4) == (True, 0, 4, 9, 4)
    assert A.clip_line(10, 8, 3, -4, 3, 20) == (True, 3, 0, 3, 7)
    assert A.clip_line(10, 8, -3, -1, 12, 14)[:1] == (True,)
    assert A.clip_line(10, 8, 10, 2, 10, 6)[0] is False and A.clip_line(10, 8, -1, -1, -5, 3)[0] is False


# ---- the display list ---------------------------------------------------------------------------------------------------
def _frame(scene, h=960, w=1280, mh=736, mw=960, native=False, name="kmeans", **extra):
    _, ref, _, _ = U.host_batch([scene], h, w, mh, mw, native)
    cls, boxes, ms = ref[0]
    settings = dict(U.settings_for(name, h, w), **extra)
    rows, rec = U.ref_rows(h, w, cls, boxes, ms, settings)
    return cls, boxes, ms, rows, rec, settings


def _kinds(prims):
    return [(p[0], p[3] if p[0] != "polyline" else p[3], p[4] if p[0] in ("rect", "line", "polyline") else p[2]) for p in prims]


def test_display_list_order_and_content_on_a_two_row_scene():
    cls, boxes, ms, rows, rec, settings = _frame(U.scenes()[0])
    prims = A.display_list(960, 1280, cls, boxes, ms, rows, settings)
    assert rec["status"] == mr.OK and rec["n_stitch"] == 20
    k = _kinds(prims)
    assert k[0] == ("rect", A.ROI_COLOUR, 2) and prims[0][1:3] == ((10, 300), (1270, 760))
    # boxes in detection order: the fabric first (this scene lists it first), then the 20 stitches, at the truncated coordinates
    assert k[1] == ("rect", A.FABRIC_BOX_COLOUR, 2) and k[2:22] == [("rect", A.STITCH_BOX_COLOUR, 1)] * 20
    assert prims[2][1:3] == (tuple(int(v) for v in boxes[1][:2]), tuple(int(v) for v in boxes[1][2:]))
    assert k[22] == ("polyline", A.ENVELOPE_COLOUR, 2) and prims[22][2] is False
    env = prims[22][1]
    assert len(env) <= 1280 and (np.diff(env[:, 0]) > 0).all()
    # per stitch of stitch_meta, in rank order: two width circles, the line between them, the centre
    order = [i for _, i in sorted((rows["rank"][i], i) for i in range(len(cls)) if rows["flags"][i] & A.KEPT)]
    at = 23
    for i in order:
        cx, cy, left, right = rows["f64"][i, :4]
        a, b = (round(left), round(cy)), (round(right), round(cy))
        assert prims[at:at + 4] == [("circle", a, 3, A.WIDTH_COLOUR), ("circle", b, 3, A.WIDTH_COLOUR), ("line", a, b, A.WIDTH_COLOUR, 1),
                                    ("circle", (round(cx), round(cy)), 3, A.CENTRE_COLOUR)]
        at += 4
    with_dist = [i for i in order if rows["flags"][i] & A.DIST]
    assert len(with_dist) == rec["n_dist"] and 0 < len(with_dist) < len(order)
    for i in with_dist:
        cx, cy, edge = rows["f64"][i, 0], rows["f64"][i, 1], rows["f64"][i, 5]
        e = (min(max(round(cx), 0), 1279), round(edge))
        assert prims[at:at + 2] == [("line", e, (round(cx), round(cy)), A.DIST_COLOUR, 1), ("circle", e, 2, A.EDGE_POINT_COLOUR)]
        at += 2
    rest = prims[at:]
    assert rest and all(p[0] == "polyline" and p[2] is True and p[3] == A.OUTLINE_COLOUR and p[4] == 2 for p in rest)


def test_round_is_half_to_even_where_the_edge_is_a_half():
    cls, boxes, ms, rows, rec, settings = _frame(U.scenes()[0])
    rows = dict(rows, f64=rows["f64"].copy())
    i = int(np.flatnonzero(rows["flags"] & A.DIST)[0])
    rows["f64"][i, 5] = 650.5
    rows["f64"][i, 0] = 301.5
    prims = A.display_list(960, 1280, cls, boxes, ms, rows, settings)
    assert ("circle", (302, 650), 2, A.EDGE_POINT_COLOUR) in prims


def test_no_fabric_stops_after_the_boxes_and_no_stitches_after_the_envelope():
    cls, boxes, ms, rows, rec, settings = _frame(U.scenes()[3])
    assert rec["status"] == mr.NO_FABRIC
    prims = A.display_list(960, 1280, cls, boxes, ms, rows, settings)
    assert [p[0] for p in prims] == ["rect"] * 11 and prims[0][3] == A.ROI_COLOUR
    assert all(p[3] == A.STITCH_BOX_COLOUR for p in prims[1:])
    cls, boxes, ms, rows, rec, settings = _frame(U.scenes()[4])
    assert rec["status"] == mr.NO_STITCHES
    prims = A.display_list(960, 1280, cls, boxes, ms, rows, settings)
    assert [p[0] for p in prims] == ["rect", "rect", "rect", "polyline"]
    assert prims[-1][2] is False and prims[-1][3] == A.ENVELOPE_COLOUR
    assert A.display_list(960, 1280, cls, boxes, ms, dict(rows, status=A.BAD_CAMERA), settings) == []


def test_roi_and_drop_empty_decide_the_boxes():
    scene = U.scenes()[2]           # stitches above the ROI, a fabric below it, a stitch left of it
    cls, boxes, ms, rows, rec, settings = _frame(scene)
    prims = A.display_list(960, 1280, cls, boxes, ms, rows, settings)
    n_boxes = sum(p[0] == "rect" for p in prims) - 1
    assert n_boxes == rec["n_stitch"] + 1 == 7
    cls, boxes, ms, rows, rec, settings = _frame(scene, roi_enabled=False)
    prims = A.display_list(960, 1280, cls, boxes, ms, rows, settings)
    assert prims[0][3] != A.ROI_COLOUR and sum(p[0] == "rect" for p in prims) == len(cls) == 14
    # drop_empty: the four stitches with empty masks of the `empty` scene have no box
    scene = U.scenes()[5]
    for drop, n in ((False, 13), (True, 9)):
        cls, boxes, ms, rows, rec, settings = _frame(scene, drop_empty=drop)
        prims = A.display_list(960, 1280, cls, boxes, ms, rows, settings)
        assert sum(p[0] == "rect" for p in prims) - 1 == n, drop


def test_the_union_form_gives_the_same_list_as_the_masks():
    cls, boxes, ms, rows, rec, settings = _frame(U.scenes()[10])
    a = A.display_list(960, 1280, cls, boxes, ms, rows, settings)
    union = np.zeros((960, 1280), np.uint8)
    for c, m in zip(cls, ms):
        if c == 1:
            union |= A.frame_bitmap(m, 960, 1280)
    b = A.display_list(960, 1280, cls, boxes, union, rows, settings)
    assert len(a) == len(b)
    for p, q in zip(a, b):
        assert p[0] == q[0] and (np.array_equal(p[1], q[1]) if p[0] == "polyline" else p == q)


def test_the_envelope_is_subsampled_as_the_reference_does():
    h, w = 40, 2500
    union = np.zeros((h, w), np.uint8)
    union[5:20, 100:2400] = 1
    rows = dict(status=A.NO_STITCHES, flags=np.zeros(0, np.int32), rank=np.zeros(0, np.int32), f64=np.zeros((0, 7)))
    prims = A.display_list(h, w, np.zeros(0), np.zeros((0, 4)), union, rows, dict(roi_enabled=False))
    assert len(prims) == 1 and prims[0][0] == "polyline"
    pts = prims[0][1]                      # 2300 valid columns: step = 2300 // 1000 = 2
    assert len(pts) == 1150 and pts[0].tolist() == [100, 19] and pts[1].tolist() == [102, 19]


# ---- text -----------------------------------------------------------------------------------------------------------------
def test_text_items_carry_the_references_strings():
    F, red, black = "FONT_HERSHEY_SIMPLEX", (0, 0, 255), (0, 0, 0)
    none = dict(flags=np.zeros(0, np.int32), rank=np.zeros(0, np.int32), f64=np.zeros((0, 7)), n_stitch=0, n_fabric=0, n_dist=0, n_width=0)
    assert A.text_items({}, dict(none, status=A.NO_FABRIC), 960) == [("Fabric not detected", (10, 55), F, 0.7, red, 2)]
    assert A.text_items({}, dict(none, status=A.NO_STITCHES), 960) == [("No stitches detected", (10, 55), F, 0.7, red, 2)]
    assert A.text_items({}, dict(none, status=A.BAD_CAMERA), 960) == []
    rows = dict(none, status=A.OK, n_stitch=7, n_fabric=2, n_dist=4, n_width=6)
    both = A.text_items(dict(edge_distance_mm=12.3456, stitch_width_mm=3.14159), rows, 960)
    assert both == [("Edge Dist: 12.35mm | Avg Width: 3.14mm (n_d=4, n_w=6)", (10, 30), F, 0.7, red, 2),
                    ("Stitches: 7 | Fabric: 2", (10, 950), F, 0.5, black, 1)]
    assert A.text_items(dict(edge_distance_mm=12.3456, stitch_width_mm=None), rows, 960)[0][0] == "Edge Distance: 12.35mm (n=4)"
    assert A.text_items(dict(edge_distance_mm=None, stitch_width_mm=3.14159), rows, 960)[0][0] == "Avg Width: 3.14mm (n=6)"
    assert A.text_items(dict(edge_distance_mm=None, stitch_width_mm=None), rows, 480, min_stitches=5) == [
        ("Insufficient stitches (dist=4, width=6, need 5)", (10, 30), F, 0.7, red, 2), ("Stitches: 7 | Fabric: 2", (10, 470), F, 0.5, black, 1)]


def test_width_labels_show_the_last_width_computed_so_far():
    """measurement.py:365-368 prints all_widths[-1]: a stitch without a width of its own repeats the previous one's, and stitches
    before the first width have no label."""
    f64 = np.full((4, 7), np.nan)
    f64[:, 0] = [100.5, 200.4, 300.6, 400.0]
    f64[:, 1] = [50.5, 51.5, 52.4, 53.0]
    f64[:, 4] = [np.nan, 2.349, np.nan, 7.0]
    rows = dict(status=A.OK, n_stitch=4, n_fabric=1, n_dist=0, n_width=2, rank=np.array([2, 0, 3, 1]), f64=f64,
                flags=np.array([A.KEPT, A.KEPT | A.WIDTH, A.KEPT, A.KEPT | A.WIDTH]))
    items = A.text_items(dict(edge_distance_mm=None, stitch_width_mm=None), rows, 960)
    labels = [it for it in items if it[3] == 0.60]
    # rank order: instance 1 (2.3), 3 (7.0), 0 (repeats 7.0), 2 (repeats 7.0); round() is half to even: 100.5 -> 100, 50.5 -> 50
    assert labels == [("2.3", (202, 32), "FONT_HERSHEY_SIMPLEX", 0.60, (0, 0, 0), 2), ("7.0", (402, 33), "FONT_HERSHEY_SIMPLEX", 0.60, (0, 0, 0), 2),
                      ("7.0", (102, 30), "FONT_HERSHEY_SIMPLEX", 0.60, (0, 0, 0), 2), ("7.0", (303, 32), "FONT_HERSHEY_SIMPLEX", 0.60, (0, 0, 0), 2)]
    rows["flags"] = np.array([A.KEPT, A.KEPT, A.KEPT, A.KEPT | A.WIDTH])
    labels = [it[0] for it in A.text_items({}, rows, 960) if it[3] == 0.60]
    assert labels == ["7.0", "7.0", "7.0"]      # rank 0 (instance 1) comes before the first width: no label


def test_put_text_needs_opencv():
    try:
        import cv2  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError):
            A.put_text(np.zeros((8, 8, 3), np.uint8), [("x", (1, 1), "FONT_HERSHEY_SIMPLEX", 0.5, (0, 0, 0), 1)])


# ---- the scenes of the GPU test exercise the whole overlay --------------------------------------------------------------------
@pytest.mark.parametrize("mode,h,w,mh,mw", U.MODES, ids=["letterbox", "native", "native_odd"])
def test_the_gpu_scenes_are_not_vacuous(mode, h, w, mh, mw):
    native = mode == "native"
    _, ref, offsets, cap = U.host_batch(U.scenes(), h, w, mh, mw, native, dead=3)
    seen, statuses, diagonal = set(), [], False
    for b, (cls, boxes, ms) in enumerate(ref):
        settings = U.settings_for("kmeans", h, w, b % 4)
        rows, rec = U.ref_rows(h, w, cls, boxes, ms, settings)
        prims, word = A.display_list(h, w, cls, boxes, ms, rows, settings, max_points=U.MAX_POINTS, with_status=True)
        assert word == 0, b                     # no scene of the parity test hits the outline bound
        statuses.append(rec["status"])
        img = A.rasterise(np.zeros((h, w, 3), np.uint8), prims)
        painted = img.reshape(-1, 3)[img.reshape(-1, 3).any(axis=1)]
        seen |= {tuple(int(v) for v in c) for c in np.unique(painted, axis=0)}
        for p in prims:
            if p[0] == "polyline" and p[2]:
                d = np.abs(np.diff(np.vstack([p[1], p[1][:1]]), axis=0))
                diagonal |= bool(((d[:, 0] > 0) & (d[:, 1] > 0)).any())
    assert seen == set(A.COLOURS), seen ^ set(A.COLOURS)
    assert statuses[3] == mr.NO_FABRIC and statuses[4] == mr.NO_STITCHES and statuses.count(mr.OK) >= 8
    assert diagonal


@pytest.mark.parametrize("mode,h,w,mh,mw", U.MODES[:2], ids=["letterbox", "native"])
def test_the_jagged_scene_alone_exceeds_the_small_outline_bound(mode, h, w, mh, mw):
    native = mode == "native"
    _, ref, _, _ = U.host_batch(U.jagged_scenes(), h, w, mh, mw, native)
    words = []
    for cls, boxes, ms in ref:
        settings = U.settings_for("kmeans", h, w)
        rows, rec = U.ref_rows(h, w, cls, boxes, ms, settings)
        assert rec["status"] == mr.OK
        prims, word = A.display_list(h, w, cls, boxes, ms, rows, settings, max_points=U.SMALL_MAX_POINTS, with_status=True)
        words.append(word)
        assert any(p[0] == "polyline" and p[2] for p in prims) == (word == 0)
        assert any(p[0] == "polyline" and not p[2] for p in prims)          # everything else stands
    assert words == [0, A.STATUS_OUTLINE, 0]
