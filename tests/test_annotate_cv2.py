"""annotate.py's raster rules against OpenCV itself, where OpenCV is installed (skipped elsewhere).  An extra: the specification
of vti_annotate is annotate.py, pinned by the closed-form cases of test_annotate.py; this file is how a machine with cv2 finds out
whether the restatement and OpenCV's drawing.cpp still agree."""
import numpy as np
import pytest

cv2 = pytest.importorskip("cv2")

import annotate_util as U                       # noqa: E402
from vti_amd import annotate as A               # noqa: E402


def _cv(img, p):
    if p[0] == "line":
        cv2.line(img, tuple(p[1]), tuple(p[2]), p[3], p[4])
    elif p[0] == "rect":
        cv2.rectangle(img, tuple(p[1]), tuple(p[2]), p[3], p[4])
    elif p[0] == "circle":
        cv2.circle(img, tuple(p[1]), p[2], p[3], -1)
    else:
        cv2.polylines(img, [np.asarray(p[1], np.int32)], bool(p[2]), p[3], p[4])


def test_every_primitive_kind_matches_opencv():
    rng = np.random.default_rng(0)
    h, w = 60, 80
    for it in range(400):
        pt = lambda: (int(rng.integers(-15, w + 15)), int(rng.integers(-15, h + 15)))
        colour = tuple(int(v) for v in rng.integers(1, 256, 3))
        kind = it % 4
        if kind == 0:
            p = ("line", pt(), pt(), colour, int(rng.integers(1, 3)))
        elif kind == 1:
            p = ("rect", pt(), pt(), colour, int(rng.integers(1, 3)))
        elif kind == 2:
            p = ("circle", pt(), int(rng.integers(0, 5)), colour)
        else:
            p = ("polyline", np.array([pt() for _ in range(int(rng.integers(1, 6)))], np.int32), bool(it & 4), colour, 2)
        ref = np.zeros((h, w, 3), np.uint8)
        _cv(ref, p)
        assert np.array_equal(A.rasterise(np.zeros((h, w, 3), np.uint8), [p]), ref), p


def test_one_whole_overlay_matches_opencv():
    h, w = 960, 1280
    _, ref, _, _ = U.host_batch([U.scenes()[0]], h, w, 736, 960, False)
    cls, boxes, ms = ref[0]
    settings = U.settings_for("kmeans", h, w)
    rows, _ = U.ref_rows(h, w, cls, boxes, ms, settings)
    prims = A.display_list(h, w, cls, boxes, ms, rows, settings)
    frame = np.random.default_rng(1).integers(0, 256, (h, w, 3), dtype=np.uint8)
    want = frame.copy()
    for p in prims:
        _cv(want, p)
    assert np.array_equal(A.rasterise(frame, prims), want)
