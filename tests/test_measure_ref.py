"""CPU checks of the measurement restatement (tests/measure_ref.py) on hand scenes with known answers, of StitchMeasurer's host
smoothing, and of vti_measure's argument checks (all made before any HIP call, so no GPU is needed)."""
import ctypes as C
import os
import types
from collections import deque

import numpy as np
import pytest

import measure_ref as mr
from test_oracle_geometry import load_calib

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CALIB = load_calib()
NOROI = dict(roi_enabled=False)


class Frame:
    """One frame's instances in detection order: class, frame-px box, frame-size 0/1 mask (native form)."""

    def __init__(self, h, w):
        self.h, self.w = h, w
        self.cls, self.boxes, self.masks = [], [], []

    def add(self, cls, box, mask=None):
        m = np.zeros((self.h, self.w), np.uint8) if mask is None else mask.astype(np.uint8)
        self.cls.append(cls)
        self.boxes.append(box)
        self.masks.append(m)
        return len(self.cls) - 1

    def rect(self, cls, y0, y1, x0, x1):
        """An instance whose mask is the rectangle rows [y0, y1), columns [x0, x1), and whose box is that rectangle."""
        m = np.zeros((self.h, self.w), np.uint8)
        m[y0:y1, x0:x1] = 1
        return self.add(cls, (x0, y0, x1, y1), m)

    def fabric_bottoms(self, bottoms, cls=1):
        """A fabric instance whose column x is set from row 0 down to bottoms[x] (< 0: empty column)."""
        m = np.zeros((self.h, self.w), np.uint8)
        for x, yb in enumerate(bottoms):
            if yb >= 0:
                m[:yb + 1, x] = 1
        return self.add(cls, (0, 0, self.w, self.h), m)

    def measure(self, **kw):
        return mr.measure_frame(self.h, self.w, np.array(self.cls), np.array(self.boxes, np.float32).reshape(-1, 4), self.masks,
                                CALIB, **kw)


def test_statuses():
    f = Frame(40, 30)
    assert f.measure(**NOROI)[0]["status"] == mr.NO_FABRIC                 # nothing at all
    f.rect(0, 10, 12, 5, 8)
    rec, st = f.measure(**NOROI)
    assert (rec["status"], rec["n_stitch"], rec["n_fabric"]) == (mr.NO_FABRIC, 1, 0)
    assert st[0]["flags"] == mr.KEPT | mr.MASK and np.isnan(st[0]["width"])
    f.add(1, (0, 0, 30, 20))                                                 # a fabric instance with an empty mask: still none
    assert f.measure(**NOROI)[0]["status"] == mr.NO_FABRIC
    g = Frame(40, 30)
    g.fabric_bottoms([20] * 30)
    rec, st = g.measure(**NOROI)
    assert (rec["status"], rec["n_stitch"], rec["n_fabric"], rec["avg_dist"]) == (mr.NO_STITCHES, 0, 1, None)


def _two_rows():
    f = Frame(40, 30)
    far = [f.rect(0, y, y + 2, x, x + 2) for x, y in ((3, 9), (12, 9), (21, 10))]        # cy 9.5, 9.5, 10.5
    f.fabric_bottoms([34] * 30)
    near = [f.rect(0, y, y + 2, x, x + 2) for x, y in ((4, 29), (13, 30), (22, 29))]     # cy 29.5, 30.5, 29.5: next to the edge
    return f, far, near


def test_kmeans_that_stops_on_its_seeds_selects_everything():
    """Two rows of exactly two values: the first update leaves the min / max seeds unchanged, so kmeans_1d_two_clusters returns
    its initial all-zero labels; cluster 1 is empty (mean 1e9) and every stitch is selected."""
    f = Frame(40, 30)
    for x, y in ((3, 9), (12, 9), (4, 29), (13, 29)):
        f.rect(0, y, y + 2, x, x + 2)
    f.fabric_bottoms([34] * 30)
    rec, st = f.measure(**NOROI)
    assert rec["n_selected"] == 4 and all(s["flags"] & mr.SELECTED for s in st)


def test_two_rows_kmeans_selects_the_row_next_to_the_edge():
    f, far, near = _two_rows()
    rec, st = f.measure(**NOROI)
    assert rec["status"] == mr.OK and rec["n_stitch"] == 6 and rec["n_fabric"] == 1
    sel = [s["i"] for s in st if s["flags"] & mr.SELECTED]
    fin = [s["i"] for s in st if s["flags"] & mr.DIST]
    assert sel == near and fin == near and rec["n_selected"] == 3 and rec["n_dist"] == 3 and rec["n_width"] == 6
    assert all(s["edge_y"] == 34.0 for s in st if s["i"] in near) and all(np.isnan(s["edge_y"]) for s in st if s["i"] in far)
    assert rec["avg_dist"] is not None and 0 < rec["avg_dist"] < 50 and rec["avg_width"] is not None
    # the median split: a spread of 21 px is one row under the default threshold, two rows under 5 px
    rec, st = f.measure(skip_cluster=True, **NOROI)
    assert rec["n_selected"] == 6
    rec, st = f.measure(skip_cluster=True, two_row_threshold_px=5, **NOROI)
    assert [s["i"] for s in st if s["flags"] & mr.SELECTED] == near
    # min_stitches gates the averages, not the counts
    rec, _ = f.measure(min_stitches=4, **NOROI)
    assert rec["avg_dist"] is None and rec["n_dist"] == 3 and rec["avg_width"] is not None


def test_nothing_near_the_edge_falls_back_to_the_selected_row():
    f, far, near = _two_rows()
    rec, st = f.measure(max_px_distance=2, **NOROI)                          # |cy - 34| > 2 for every stitch
    assert not any(s["flags"] & mr.NEAR for s in st)
    assert [s["i"] for s in st if s["flags"] & mr.DIST] == near and rec["n_dist"] == 3


def test_roi_filters_stitches_and_fabric():
    f, far, near = _two_rows()
    rec, st = f.measure(roi=(0, 20, 29, 39))           # box centres with y in [20, 39], bounds inclusive: the near row, the fabric (y 20)
    assert [s["i"] for s in st] == near and rec["n_fabric"] == 1 and rec["status"] == mr.OK
    rec, st = f.measure(roi=(0, 21, 29, 39))           # the fabric's centre is out: no fabric, whatever the stitches
    assert [s["i"] for s in st] == near and rec["n_fabric"] == 0 and rec["status"] == mr.NO_FABRIC
    rec, st = f.measure(roi=(0, 21, 29, 21))           # degenerate after clamping: the ROI is inactive
    assert rec["n_stitch"] == 6 and rec["status"] == mr.OK


def test_round_half_to_even_of_cx():
    f = Frame(40, 30)
    f.fabric_bottoms([10 + x for x in range(30)])
    a = f.rect(0, 20, 22, 2, 4)                                              # cx = 2.5 -> 2
    b = f.rect(0, 20, 22, 5, 7)                                              # cx = 5.5 -> 6
    rec, st = f.measure(envelope_neighborhood=0, **NOROI)
    by = {s["i"]: s for s in st}
    assert by[a]["cx"] == 2.5 and by[b]["cx"] == 5.5
    assert by[a]["edge_y"] == 12.0 and by[b]["edge_y"] == 16.0


@pytest.mark.parametrize("pair,cy_row,near", [((20, 21), 40, False), ((21, 22), 41, True)])
def test_even_count_median_rounds_half_to_even(pair, cy_row, near):
    """Two envelope values around the centre: the median is k + 0.5 and python's round() takes the even neighbour."""
    f = Frame(48, 30)
    bottoms = [-1] * 30
    bottoms[3], bottoms[5] = pair
    f.fabric_bottoms(bottoms)
    i = f.rect(0, cy_row, cy_row + 1, 4, 5)                                   # cx = 4.0, cy = cy_row
    rec, st = f.measure(envelope_neighborhood=1, max_px_distance=19.5, **NOROI)
    s = st[0]
    assert s["i"] == i and bool(s["flags"] & mr.NEAR) == near
    assert s["edge_y"] == (pair[0] + pair[1]) / 2                             # the edge itself is not rounded
    assert s["flags"] & mr.DIST                                               # near or by the fall-back


def test_neighbourhood_clips_at_the_frame_columns():
    f = Frame(40, 30)
    bottoms = [10] * 30
    bottoms[0], bottoms[29] = 30, 31
    f.fabric_bottoms(bottoms)
    f.rect(0, 20, 22, 0, 1)                                                   # cx = 0: xs = 0,0,0,0,1,2,3
    f.rect(0, 20, 22, 29, 30)                                                 # cx = 29: xs = 26,27,28,29,29,29,29
    rec, st = f.measure(**NOROI)
    assert [s["edge_y"] for s in st] == [30.0, 31.0]


def test_empty_stitch_masks_use_the_box_and_drop_empty_removes_them():
    f, far, near = _two_rows()
    e = f.add(0, (10, 26, 15, 33))                                            # empty mask: box centre (12.5, 29.5), width 5
    rec, st = f.measure(**NOROI)
    s = [s for s in st if s["i"] == e][0]
    assert (s["cx"], s["cy"], s["left"], s["right"]) == (12.5, 29.5, 10.0, 15.0) and not s["flags"] & mr.MASK
    assert rec["n_stitch"] == 7
    rec, st = f.measure(drop_empty=True, **NOROI)
    assert rec["n_stitch"] == 6 and e not in [s["i"] for s in st]


def test_stitch_measurer_smoothing_matches_a_deque():
    import vti_amd
    p = vti_amd.MeasureParams.from_files(os.path.join(G, "camera_calibration.json"), os.path.join(G, "extrinsics.json"))
    assert np.allclose(p.R, CALIB[2], atol=1e-15) and np.array_equal(p.K, CALIB[0]) and np.array_equal(p.t, CALIB[3])
    sm = vti_amd.StitchMeasurer(types.SimpleNamespace(drop_empty_masks=False), p, frame_buffer=3)
    rng = np.random.default_rng(4)
    dq_d, dq_w = deque(maxlen=3), deque(maxlen=3)
    for k in range(20):
        status = int(rng.choice([0, 0, 0, 1, 2]))
        d = np.nan if rng.uniform() < 0.3 else rng.uniform(5, 15)
        w = np.nan if rng.uniform() < 0.3 else rng.uniform(1, 3)
        n_d = int(rng.integers(0, 9))
        rec = sm._record(np.array([d, w]), np.array([status, 5, 1, 4, n_d, 5], np.int32))
        if status:
            assert rec["error"] == ("Fabric not detected" if status == 1 else "No stitches detected")
            assert rec["edge_distance_mm"] is None and rec["stitch_width_mm"] is None and rec["stitch_count"] == 0
            continue
        exp_d = exp_w = None
        if not np.isnan(d):
            dq_d.append(d)
            exp_d = float(np.median(dq_d))
        if not np.isnan(w):
            dq_w.append(w)
            exp_w = float(np.median(dq_w))
        assert (rec["edge_distance_mm"], rec["stitch_width_mm"], rec["stitch_count"]) == (exp_d, exp_w, n_d) and "error" not in rec


def test_measure_argument_checks_without_a_gpu(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    eng = vti_amd.Engine("n", 2, H=64, W=64, max_batch=2)
    p = vti_amd.MeasureParams(*CALIB)
    B, max_det, cap, H0, W0 = 2, 10, 20, 48, 64
    need = eng.measure_scratch_bytes(B, cap, W0)
    assert need >= cap * 44 + B * W0 * 4 and need % 256 == 0
    assert L.vti_measure_scratch_bytes(eng._ctx, -1, cap, W0) == 0 and L.vti_measure_scratch_bytes(None, B, cap, W0) == 0
    one, ws = C.c_void_p(4096), C.c_void_p(1 << 20)           # never dereferenced: every check comes before any HIP call

    def call(params=p, ctx=eng._ctx, masks=one, native=0, dets=one, B=B, max_det=max_det, cap=cap, scratch=ws, nbytes=need):
        cp = params.to_c() if params is not None else None
        return L.vti_measure(ctx, C.byref(cp) if cp is not None else None, masks, native, dets, one, one, one, B, max_det, cap, H0,
                             W0, scratch, nbytes, one, one, None, None, None)

    import dataclasses as dc
    assert call(params=None) == -1
    assert call(ctx=None) == -1
    assert call(params=dc.replace(p, envelope_neighborhood=-1)) == -1
    assert b"envelope_neighborhood" in L.vti_last_error(eng._ctx)
    assert call(params=dc.replace(p, envelope_neighborhood=65)) == -1
    assert call(params=dc.replace(p, fabric_id=0)) == -1
    assert call(params=dc.replace(p, min_stitches=0)) == -1
    assert call(params=dc.replace(p, kmeans_iters=-1)) == -1
    assert call(params=dc.replace(p, max_px_distance=float("nan"))) == -1
    assert call(nbytes=need - 1) == -1
    assert b"scratch" in L.vti_last_error(eng._ctx)
    assert call(scratch=C.c_void_p(4096 + 64)) == -1
    assert call(scratch=None) == -1
    assert call(native=2) == -1
    assert call(masks=C.c_void_p(4096 + 8)) == -1               # letterbox bits: 16-byte loads
    assert call(masks=C.c_void_p(4096 + 4), native=1) == -1     # native rows: 8-byte loads
    assert call(masks=None) == -1
    assert call(dets=None) == -1
    assert call(B=-1) == -1 and call(max_det=0) == -1 and call(cap=-1) == -1
    assert call(max_det=vti_amd._lib.VTI_MEASURE_MAX_DET + 1) == -6
    assert call(B=0, cap=0, masks=None, nbytes=0, scratch=None) == 0     # nothing to do: no launch
