"""CPU checks of the stitch-distance checker's restatement (tests/checker_ref.py) on hand scenes with known answers, and of the
host side of StitchDistanceChecker (smoothing, info text, checker_text_items).  No GPU and no library call."""
import types
from collections import deque

import numpy as np
import pytest

import checker_ref as cr
import measure_ref as mr
from test_oracle_geometry import load_calib

CALIB = load_calib()
H, W = 40, 30


class Frame:
    """One frame's instances in detection order: class, frame-px box, frame-size 0/1 mask."""

    def __init__(self, h=H, w=W):
        self.h, self.w = h, w
        self.cls, self.boxes, self.masks = [], [], []

    def add(self, cls, box, mask=None):
        self.cls.append(cls)
        self.boxes.append(box)
        self.masks.append(np.zeros((self.h, self.w), np.uint8) if mask is None else mask.astype(np.uint8))
        return len(self.cls) - 1

    def rect(self, cls, y0, y1, x0, x1):
        """An instance whose mask is the rectangle rows [y0, y1), columns [x0, x1), and whose box is that rectangle."""
        m = np.zeros((self.h, self.w), np.uint8)
        m[y0:y1, x0:x1] = 1
        return self.add(cls, (x0, y0, x1, y1), m)

    def fabric(self, tops, bottoms, cls=1):
        """A fabric instance whose column x is set from row tops[x] to bottoms[x], both inclusive (tops[x] < 0: empty column)."""
        m = np.zeros((self.h, self.w), np.uint8)
        for x, (ya, yb) in enumerate(zip(tops, bottoms)):
            if ya >= 0:
                m[ya:yb + 1, x] = 1
        return self.add(cls, (0, 0, self.w, self.h), m)

    def args(self):
        return self.h, self.w, np.array(self.cls), np.array(self.boxes, np.float32).reshape(-1, 4), self.masks

    def check(self, calib=CALIB, **kw):
        return cr.measure_frame(*self.args(), calib, **kw)

    def process(self, **kw):
        return mr.measure_frame(*self.args(), CALIB, roi_enabled=False, **kw)


def _two_rows(f):
    """Three stitches 4-5 px below the fabric's top edge, three next to its bottom edge."""
    top = [f.rect(0, y, y + 2, x, x + 2) for x, y in ((3, 14), (12, 14), (21, 15))]      # cy 14.5, 14.5, 15.5
    f.fabric([10 + (x >= 15) for x in range(W)], [34] * W)                               # top edge 10 | 11, bottom edge 34
    bottom = [f.rect(0, y, y + 2, x, x + 2) for x, y in ((4, 29), (13, 30), (22, 29))]   # cy 29.5, 30.5, 29.5
    return top, bottom


def test_statuses_and_fabric_count():
    f = Frame()
    assert f.check()[0]["status"] == cr.NO_FABRIC
    f.rect(0, 10, 12, 5, 8)
    rec, st = f.check()
    assert (rec["status"], rec["n_stitch"], rec["n_fabric"]) == (cr.NO_FABRIC, 1, 0)
    assert st[0]["flags"] == cr.KEPT | cr.MASK and np.isnan(st[0]["width"])
    f.add(1, (40.0, 0.0, 50.0, 20.0))                 # an empty-mask fabric whose box lies outside the frame: counted, union empty
    rec, _ = f.check()
    assert (rec["status"], rec["n_fabric"]) == (cr.NO_FABRIC, 1)
    g = Frame()
    g.fabric([10] * W, [20] * W)
    rec, _ = g.check()
    assert (rec["status"], rec["n_stitch"], rec["n_fabric"], rec["avg_dist"]) == (cr.NO_STITCHES, 0, 1, None)


def test_the_upper_envelope_is_used_and_the_record_differs_from_process_frame():
    f = Frame()
    top, bottom = _two_rows(f)
    env, n_fab = cr.fabric_envelope(*f.args())
    assert env.tolist() == [10] * 15 + [11] * 15 and n_fab == 1
    rec, st = f.check()
    assert (rec["status"], rec["n_stitch"], rec["n_fabric"], rec["n_selected"], rec["n_dist"], rec["n_width"]) == (0, 6, 1, 3, 3, 3)
    by = {s["i"]: s for s in st}
    assert [s["i"] for s in st if s["flags"] & cr.SELECTED] == top          # the mean envelope row is 10.5: the upper row is nearer
    assert [by[i]["edge_y"] for i in top] == [10.0, 10.0, 11.0]             # cx 3.5 -> 4: cols 1..7; 12.5 -> 12: 9..15 (six 10s, one 11); 21.5 -> 22
    assert all(by[i]["flags"] == cr.KEPT | cr.MASK | cr.SELECTED | cr.NEAR | cr.DIST | cr.WIDTH for i in top)
    # the lower row is near too (0 < 29.5 - 10 < 150) but not selected: nothing but the centroid is computed for it
    assert all(by[i]["flags"] == cr.KEPT | cr.MASK | cr.NEAR and np.isnan(by[i]["width"]) and np.isnan(by[i]["edge_y"]) for i in bottom)
    assert rec["avg_dist"] is not None and rec["avg_width"] is not None
    # process_frame on the same scene measures to the bottom edge, from the bottom row, and gives every stitch a width
    prec, pst = f.process()
    pby = {s["i"]: s for s in pst}
    assert [s["i"] for s in pst if s["flags"] & mr.DIST] == bottom and all(pby[i]["edge_y"] == 34.0 for i in bottom)
    assert prec["n_width"] == 6 and rec["n_width"] == 3
    assert abs(prec["avg_dist"] - rec["avg_dist"]) > 1e-3


def test_a_stitch_on_or_above_the_edge_is_dropped_from_the_final_set():
    f = Frame()
    f.fabric([10] * W, [34] * W)
    below = f.rect(0, 14, 16, 3, 5)                   # cy 14.5: 4.5 px below the edge
    above = f.rect(0, 7, 9, 12, 14)                   # cy 7.5: above it, cy - env_y = -2.5
    on = f.rect(0, 10, 11, 20, 22)                    # cy 10.0: on it, cy - env_y = 0, and 0 < 0 is false
    rec, st = f.check(skip_cluster=True)
    by = {s["i"]: s for s in st}
    assert rec["n_selected"] == 3 and rec["n_dist"] == 1 and rec["n_width"] == 1
    assert by[below]["flags"] & cr.NEAR and by[below]["flags"] & cr.DIST and by[below]["edge_y"] == 10.0
    for i in (above, on):
        assert by[i]["flags"] == cr.KEPT | cr.MASK | cr.SELECTED and np.isnan(by[i]["edge_y"]) and np.isnan(by[i]["width"])
    # process_frame's unsigned test keeps all three
    prec, pst = f.process(skip_cluster=True, two_row_threshold_px=1000)
    assert all(s["flags"] & mr.NEAR for s in pst)


def test_no_selected_stitch_passes_so_the_final_set_is_the_selected_set():
    f = Frame()
    f.fabric([20] * W, [34] * W)
    ids = [f.rect(0, y, y + 2, x, x + 2) for x, y in ((3, 5), (12, 6), (21, 5))]         # all above the edge
    rec, st = f.check(skip_cluster=True)
    assert not any(s["flags"] & cr.NEAR for s in st)
    assert [s["i"] for s in st if s["flags"] & cr.DIST] == ids and rec["n_dist"] == 3 and rec["n_width"] == 3
    assert all(s["edge_y"] == 20.0 for s in st) and rec["avg_dist"] is not None
    # the same through the distance bound: below the edge, but farther than max_px_distance
    g = Frame()
    g.fabric([2] * W, [34] * W)
    ids = [g.rect(0, y, y + 2, x, x + 2) for x, y in ((3, 25), (12, 26), (21, 25))]
    rec, st = g.check(skip_cluster=True, max_px_distance=5)
    assert not any(s["flags"] & cr.NEAR for s in st) and rec["n_dist"] == 3


def test_an_empty_mask_fabric_joins_the_union_with_its_box():
    f = Frame()
    f.fabric([10 if x < 20 else -1 for x in range(W)], [34] * W)
    f.add(1, (15.7, 5.2, 28.9, 20.5))                 # empty mask; int box (15, 5, 28, 20), both corners inclusive
    s = f.rect(0, 14, 16, 23, 25)                     # cx 23.5 -> 24: over the box only
    env, n_fab = cr.fabric_envelope(*f.args())
    assert env.tolist() == [10] * 15 + [5] * 14 + [-1] and n_fab == 2
    rec, st = f.check(min_stitches=1)
    assert (rec["status"], rec["n_fabric"], rec["n_dist"]) == (cr.OK, 2, 1) and st[0]["edge_y"] == 5.0
    # with drop_empty the instance does not exist: columns 20.. have no edge, so the stitch has no distance (but a width)
    env, n_fab = cr.fabric_envelope(*f.args(), drop_empty=True)
    assert env.tolist() == [10] * 20 + [-1] * 10 and n_fab == 1
    rec, st = f.check(min_stitches=1, drop_empty=True)
    assert (rec["status"], rec["n_fabric"], rec["n_selected"], rec["n_dist"], rec["n_width"]) == (cr.OK, 1, 1, 0, 1)
    assert st[0]["i"] == s and np.isnan(st[0]["edge_y"]) and not st[0]["flags"] & cr.NEAR and st[0]["flags"] & cr.WIDTH
    # process_frame ignores a fabric instance with an empty mask either way
    assert f.process()[0]["n_fabric"] == 1
    # a box in the other corner order, partly outside the frame: clipped, still inclusive
    assert cr.filled_rectangle(6, 5, 7, 4, 2, -3)[:, :].tolist() == [[0, 0, 1, 1, 1]] * 5 + [[0] * 5]
    assert cr.filled_rectangle(6, 5, 2, -9, 4, -1).sum() == 0


def test_skip_cluster_selects_every_stitch():
    f = Frame()
    top, bottom = _two_rows(f)
    rec, st = f.check(skip_cluster=True)
    assert rec["n_selected"] == 6 and rec["n_dist"] == 6 and rec["n_width"] == 6 and all(s["flags"] & cr.SELECTED for s in st)
    rec, st = f.check(skip_cluster=True, max_px_distance=10)      # the bottom row is 18.5+ px below the edge
    assert rec["n_selected"] == 6 and [s["i"] for s in st if s["flags"] & cr.DIST] == top


def test_the_checkers_kmeans_returns_its_last_assignment():
    """Two tight rows: the first update leaves the min / max seeds unchanged.  measurement.py's loop then returns its initial
    all-zero labels (every stitch selected); the checker's sets labels = new_labels first, so the rows are split."""
    vals = np.array([9.5, 9.5, 29.5, 29.5])
    assert cr.kmeans_1d_two_clusters(vals)[0].tolist() == [0, 0, 1, 1]
    from oracle import geometry as og
    assert og.kmeans_1d_two_clusters(vals)[0].tolist() == [0, 0, 0, 0]
    assert cr.kmeans_1d_two_clusters(vals, 0)[0].tolist() == [0, 0, 0, 0]              # no pass at all: the initial zeros
    assert cr.kmeans_1d_two_clusters(np.array([4.0, 4.0, 4.0]))[0].tolist() == [0, 0, 0]
    f = Frame()
    ids = [f.rect(0, y, y + 2, x, x + 2) for x, y in ((3, 14), (12, 14), (4, 29), (13, 29))]
    f.fabric([10] * W, [34] * W)
    rec, st = f.check()
    assert rec["n_selected"] == 2 and [s["i"] for s in st if s["flags"] & cr.SELECTED] == ids[:2]
    assert f.process()[0]["n_selected"] == 4
    # a tie between the two cluster means picks label 1 (strict <): rows at 14.5 and 29.5, mean envelope row 22
    g = Frame()
    ids = [g.rect(0, y, y + 2, x, x + 2) for x, y in ((3, 14), (12, 14), (4, 29), (13, 29))]
    g.fabric([22] * W, [34] * W)
    rec, st = g.check()
    assert [s["i"] for s in st if s["flags"] & cr.SELECTED] == ids[2:]


def degenerate_calib(k02, k12=20.0):
    """dist = 0 and a rotation whose third column is (1, 0, 0): the plane normal is the camera's x axis, so n . ray = (u - K02) / fx,
    exactly 0 at u = K02 (the undistort iteration is the identity for zero distortion) and the reference returns None there."""
    K = np.array([[100.0, 0.0, float(k02)], [0.0, 100.0, float(k12)], [0.0, 0.0, 1.0]])
    R = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])
    return K, np.zeros(5), R, np.array([0.5, 0.0, 1.0])


def test_the_width_estimate_is_used_when_an_end_has_no_world_point():
    from oracle import geometry as og
    calib = degenerate_calib(12)
    n_c, d_c = og.compute_camera_plane(calib[2], calib[3])
    assert n_c.tolist() == [1.0, 0.0, 0.0]
    assert og.pixel_to_world_using_camera_plane(12.0, 20.0, *calib, n_c, d_c) is None
    assert og.pixel_to_world_using_camera_plane(13.5, 20.0, *calib, n_c, d_c) is not None
    f = Frame()
    f.fabric([10] * W, [34] * W)
    a = f.rect(0, 19, 22, 12, 16)                     # cols 12..15: left = 12 = K02, cx 13.5, cy 20.0, px_width 3
    b = f.rect(0, 19, 22, 20, 24)                     # both ends have a world point
    rec, st = f.check(calib=calib, skip_cluster=True, min_stitches=1)
    by = {s["i"]: s for s in st}
    assert (by[a]["left"], by[a]["right"], by[a]["cx"], by[a]["cy"], by[a]["px_width"]) == (12.0, 15.0, 13.5, 20.0, 3.0)
    # cy = K12, so the rays are (x, 0, 1) with x = (u - 12) / 100 and X_cam = (0.5, 0, 0.5 / x): |world(23.5) - world(13.5)| =
    # 0.5 / 0.015 - 0.5 / 0.115 m, and the width is 3 / 10 of that
    exp = 0.3 * (0.5 / 0.015 - 0.5 / 0.115) * 1000.0
    assert by[a].get("estimated") and by[a]["flags"] & cr.WIDTH and abs(by[a]["width"] - exp) <= 1e-9 * exp
    assert abs(exp - 8695.652173913044) < 1e-6
    assert not by[b].get("estimated") and abs(by[b]["width"] - (0.5 / 0.08 - 0.5 / 0.11) * 1000.0) <= 1e-9 * 2000
    assert rec["n_width"] == 2 and rec["n_dist"] == 2
    # the centroid on the singular column: neither a distance, nor a width of either kind
    g = Frame()
    g.fabric([10] * W, [34] * W)
    c = g.rect(0, 19, 22, 10, 15)                     # cols 10..14: cx 12.0 = K02; both ends fine, so the width is the plain one
    d = g.add(0, (12.0, 18.0, 12.9, 22.0))            # empty mask: box (12, 18, 12, 22): left = right = cx = 12, all singular
    rec, st = g.check(calib=calib, skip_cluster=True, min_stitches=1)
    by = {s["i"]: s for s in st}
    assert by[c]["flags"] & cr.WIDTH and not by[c]["flags"] & cr.DIST and by[c]["edge_y"] == 10.0 and np.isnan(by[c]["dist"])
    assert not by[d]["flags"] & (cr.WIDTH | cr.DIST) and np.isnan(by[d]["width"]) and by[d]["edge_y"] == 10.0
    assert (rec["n_selected"], rec["n_dist"], rec["n_width"]) == (2, 0, 1)


def test_the_info_text_forms():
    assert cr.info_text(12.345, 2.5, 7, 3) == "Edge Dist: 12.35mm | Avg Width: 2.50mm (n=7)"
    assert cr.info_text(12.345, None, 2, 3) == "Edge Distance: 12.35mm (n=2)"
    assert cr.info_text(None, 2.5, 4, 3) == "Avg Width: 2.50mm (n=4)"
    assert cr.info_text(None, None, 2, 3) == "Insufficient stitches (found 2, need 3)"
    sm = cr.Smoother(3)
    assert sm(dict(status=cr.NO_FABRIC))["info_text"] == "Fabric not detected"
    assert sm(dict(status=cr.NO_STITCHES))["error"] == "No stitches detected"
    r = sm(dict(status=cr.OK, avg_dist=None, avg_width=None, n_width=1))
    assert r["info_text"] == "Insufficient stitches (found 1, need 3)" and r["stitch_count"] == 1 and "error" not in r
    r = sm(dict(status=cr.OK, avg_dist=4.0, avg_width=None, n_width=5))
    assert r["info_text"] == "Edge Distance: 4.00mm (n=5)" and r["edge_distance_mm"] == 4.0 and r["stitch_width_mm"] is None
    r = sm(dict(status=cr.OK, avg_dist=8.0, avg_width=2.0, n_width=3))
    assert r["info_text"] == "Edge Dist: 6.00mm | Avg Width: 2.00mm (n=3)"           # the median of the deque (4, 8)


def test_stitch_distance_checker_smoothing_and_text_match_the_restatement():
    import vti_amd
    p = vti_amd.CheckerParams(*CALIB)
    assert (p.max_px_distance, p.min_stitches, p.envelope_neighborhood, p.skip_cluster, p.kmeans_iters, p.frame_buffer) == \
        (150, 3, 3, False, 10, 8)
    ck = vti_amd.StitchDistanceChecker(types.SimpleNamespace(drop_empty_masks=True), p, frame_buffer=3)
    assert ck.params.drop_empty and ck.params.frame_buffer == 3 and ck.frame_buf_dist.maxlen == 3
    sm = cr.Smoother(3, 3)
    rng = np.random.default_rng(4)
    for k in range(24):
        status = int(rng.choice([0, 0, 0, 1, 2]))
        d = None if rng.uniform() < 0.3 else float(rng.uniform(5, 15))
        w = None if rng.uniform() < 0.3 else float(rng.uniform(1, 3))
        n_w = int(rng.integers(0, 9))
        got = ck._record(np.array([np.nan if d is None else d, np.nan if w is None else w]),
                         np.array([status, 5, 1, 4, n_w + 1, n_w], np.int32))
        exp = sm(dict(status=status, avg_dist=d, avg_width=w, n_width=n_w))
        assert {k: v for k, v in got.items() if k != "timestamp"} == exp and "timestamp" in got
    assert list(ck.frame_buf_dist) == list(sm.d) and list(ck.frame_buf_width) == list(sm.w)


def test_checker_text_items():
    import vti_amd
    font = "FONT_HERSHEY_SIMPLEX"
    f64 = np.full((5, 7), np.nan)
    f64[:, 0] = [10.5, 20.4, 30.6, 40.0, 50.0]
    f64[:, 1] = [100.5, 101.5, 99.4, 98.0, 97.0]
    f64[:, 4] = [np.nan, 2.34, np.nan, 9.99, np.nan]
    K, S, N, Wd = 1, 4, 8, 32
    # rank order: slot 2 (final, no width yet: no label), slot 1 (final, width 2.34), slot 0 (final, no width: repeats 2.34),
    # slot 3 (selected but not near while others are: not final), slot 4 (not a stitch)
    rows = dict(status=0, n_stitch=4, n_fabric=2, f64=f64, rank=[2, 1, 0, 3, -1],
                flags=[K | S | N, K | S | N | Wd, K | S | N, K | S | Wd, 0])
    rec = dict(info_text="Edge Distance: 4.00mm (n=1)")
    items = vti_amd.checker_text_items(rec, rows, 480)
    assert items == [("w:2.3mm", (26, 108), font, 0.45, (0, 255, 0), 1),          # round(20.4) + 6, round(101.5) = 102 (half to even) + 6
                     ("w:2.3mm", (16, 106), font, 0.45, (0, 255, 0), 1),          # round(10.5) = 10, round(100.5) = 100
                     ("Edge Distance: 4.00mm (n=1)", (10, 30), font, 0.7, (0, 0, 255), 2),
                     ("Stitches: 4 | Fabric: 2", (10, 470), font, 0.5, (255, 255, 255), 1)]
    # nothing near: the final set is the selected set, so slot 3 is labelled too
    rows["flags"] = [K | S, K | S | Wd, K | S, K | S | Wd, 0]
    assert [i[0] for i in vti_amd.checker_text_items(rec, rows, 480)][:3] == ["w:2.3mm", "w:2.3mm", "w:10.0mm"]
    for status, text in ((1, "Fabric not detected"), (2, "No stitches detected")):
        assert vti_amd.checker_text_items(dict(info_text=text), dict(rows, status=status), 480) == \
            [(text, (10, 55), font, 0.7, (0, 0, 255), 2)]
