"""overlay.py against OpenCV itself, where OpenCV is installed (the whole file is skipped elsewhere).  An extra: the specification of
vti_overlay is overlay.py, pinned by the closed-form cases of test_overlay.py; this file is how a machine with cv2 finds out whether
the restatement still agrees with the cv2 calls the viewer makes (Utils/check_model.py:215-255): findContours / drawContours,
rectangle (outlined and filled), addWeighted."""
import numpy as np
import pytest

cv2 = pytest.importorskip("cv2")

from vti_amd import overlay as O               # noqa: E402


def _scene(h, w, seed):
    """Blobs without islands inside holes (the RETR_EXTERNAL deviation of polygons.py is not this file's subject)."""
    rng = np.random.default_rng(seed)
    cls, boxes, masks, plates = [], [], [], []
    for i in range(7):
        x1, y1 = int(rng.integers(-5, w - 20)), int(rng.integers(-5, h - 20))
        x2, y2 = x1 + int(rng.integers(8, 60)), y1 + int(rng.integers(8, 50))
        m = np.zeros((h, w), np.uint8)
        if i != 3:                                                          # instance 3 has an empty mask
            yy, xx = np.mgrid[0:h, 0:w]
            cx, cy, rx, ry = (x1 + x2) / 2, (y1 + y2) / 2, (x2 - x1) / 2, (y2 - y1) / 2
            m[((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 <= 1.0] = 1
            m[max(y1, 0):max(y1, 0) + 3, max(x1, 0):max(x1, 0) + 2] = 1     # and a second component
        cls.append(int(rng.integers(0, 9)))
        boxes.append((x1 + 0.4, y1 + 0.6, x2 + 0.2, y2 + 0.9))
        masks.append(m)
        plates.append((x1, max(20, y1 - 8) - 22, x1 + int(rng.integers(30, 90)), max(20, y1 - 8) + 4))
    return np.array(cls), np.array(boxes, np.float32), masks, plates


def _viewer(frame, cls, boxes, masks, plates):
    """The viewer's cv2 calls, without the text: -> (annotated before the blend, overlay)."""
    annotated, overlay = frame.copy(), frame.copy()
    for c, box, m, plate in zip(cls, boxes, masks, plates):
        col = O.colour(c)
        x1, y1, x2, y2 = (int(v) for v in box)
        if np.count_nonzero(m):
            overlay[m > 0] = col
            found, _ = cv2.findContours(m, cv2.RETR_EXTERNAL, cv2.CHAIN_APPROX_SIMPLE)
            cv2.drawContours(annotated, found, -1, col, 2)
        cv2.rectangle(annotated, (x1, y1), (x2, y2), col, 2)
        cv2.rectangle(annotated, plate[:2], plate[2:], col, -1)
    return annotated, overlay


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_picture_matches_the_viewers_cv2_calls(seed):
    h, w = 120, 160
    frame = np.random.default_rng(10 + seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    cls, boxes, masks, plates = _scene(h, w, seed)
    annotated, overlay = _viewer(frame, cls, boxes, masks, plates)
    draw = O.render(frame, cls, boxes, masks, plates, mode=O.DRAW)
    assert np.array_equal(draw, annotated)                                   # pixel for pixel
    bitmaps = [O.instance_bitmap(m, h, w) for m in masks]
    assert np.array_equal(O.tint(frame, cls, bitmaps), overlay)
    want = cv2.addWeighted(overlay, 0.30, annotated, 0.70, 0.0)
    both = O.render(frame, cls, boxes, masks, plates, mode=O.BOTH)
    assert np.abs(both.astype(int) - want.astype(int)).max() <= 1            # a cv2 without FMA rounds a * alpha too
    agree = O.add_weighted(overlay, annotated) == O.add_weighted_unfused(overlay, annotated)
    assert np.array_equal(both[agree], want[agree])                          # exactly equal wherever the two forms agree


def test_get_text_size_plates_are_proper_rectangles():
    items = O.label_items(np.array([0, 1]), np.array([0.91, 0.5]), np.array([[10, 50, 60, 80], [5, 3, 40, 30]], np.float32), ["a", "b"])
    rects = O.plates(items)
    assert rects.shape == (2, 4) and (rects[:, 2] > rects[:, 0]).all() and (rects[:, 3] > rects[:, 1]).all()
    assert rects[0, 0] == 10 and rects[0, 3] == 46 and rects[1, 3] == 24     # (x1, ..., text_y + 4), text_y = max(20, y1 - 8)
