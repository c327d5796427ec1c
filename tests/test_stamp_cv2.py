"""annotate.text_stamps with its default rasteriser against cv2.putText applied directly, where OpenCV is installed (skipped
elsewhere).  An extra: the specification of vti_stamp is annotate.stamp, pinned by test_stamp.py with an injected rasteriser; this
file is how a machine with cv2 finds out that stamping the rasterised strings and writing them onto the picture give the same bytes."""
import numpy as np
import pytest

cv2 = pytest.importorskip("cv2")

from vti_amd import annotate as A               # noqa: E402


def _rows(n, w, h, rng):
    f64 = np.zeros((n, 7))
    f64[:, 0] = rng.uniform(-10, w + 10, n)     # centroids on both sides of every border: some labels are clipped
    f64[:, 1] = rng.uniform(-5, h + 25, n)
    f64[:, 4] = rng.uniform(1, 20, n)
    return dict(status=A.OK, n_stitch=n, n_fabric=1, n_dist=n, n_width=n, flags=np.full(n, A.KEPT | A.WIDTH), rank=np.arange(n), f64=f64)


def test_stamping_the_rasterised_text_is_put_text():
    h, w = 97, 131
    rng = np.random.default_rng(0)
    records = [dict(edge_distance_mm=3.251, stitch_width_mm=4.104), dict(edge_distance_mm=None, stitch_width_mm=4.1),
               dict(edge_distance_mm=None, stitch_width_mm=None)]
    clipped = 0
    for k, record in enumerate(records):
        items = A.text_items(record, _rows(6 + k, w, h, rng), h)
        pic = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        want = A.put_text(pic.copy(), items)
        stamps = A.text_stamps(items, h, w)
        assert np.array_equal(A.stamp(pic.copy(), stamps), want), k
        clipped += sum(x == 0 or y == 0 or x + b.shape[1] == w or y + b.shape[0] == h for x, y, b, _ in stamps)
    for status in (A.NO_FABRIC, A.NO_STITCHES):
        items = A.text_items({}, dict(status=status), h)
        pic = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        assert np.array_equal(A.stamp(pic.copy(), A.text_stamps(items, h, w)), A.put_text(pic.copy(), items))
    assert clipped >= 2                         # the info line runs past the right border, a label past another one
