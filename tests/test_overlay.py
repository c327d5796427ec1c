"""overlay.py, the host specification of vti_overlay (the model-check viewer's picture, Utils/check_model.py:155-256), pinned by
closed-form cases on the CPU: the blend's arithmetic for every (a, b) pair against exact rational arithmetic, the tint's order, what
an empty mask draws, the filled rectangle against FillConvexPoly, and the identity between the three modes.  The device is compared
with these functions in test_gpu_overlay.py."""
from fractions import Fraction

import numpy as np
import pytest

from vti_amd import annotate as A
from vti_amd import overlay as O


def _f32_fraction(v):
    """The float32 nearest to v as an exact integer over a power of two."""
    m, e = np.frexp(np.float32(v))                      # v = m * 2^e, 0.5 <= |m| < 1: m * 2^24 is an integer
    return Fraction(int(np.float32(m) * np.float32(1 << 24)), 1 << 24) * Fraction(2) ** int(e)


def _round_f32(q):
    """The exact rational q >= 0 rounded once to float32 (half to even), as a Fraction."""
    if q == 0:
        return q
    e = 0
    while q >= Fraction(2) ** (e + 1):
        e += 1
    while q < Fraction(2) ** e:
        e -= 1
    ulp = Fraction(2) ** (e - 23)
    n = q / ulp                                         # 2^23 <= n < 2^24
    lo = n.numerator // n.denominator
    rem = n - lo
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and lo % 2 == 1):
        lo += 1
    return lo * ulp


def _round_half_even(q):
    lo = q.numerator // q.denominator
    rem = q - lo
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and lo % 2 == 1):
        lo += 1
    return lo


def _exact_blend(alpha, beta):
    """[256, 256] (a, b) -> the fused form in integer / Fraction arithmetic, independent of numpy's float arithmetic."""
    al, be = _f32_fraction(alpha), _f32_fraction(beta)
    assert float(al) == float(np.float32(alpha)) and float(be) == float(np.float32(beta))
    prod = [_round_f32(b * be) for b in range(256)]
    out = np.zeros((256, 256), np.uint8)
    for a in range(256):
        for b in range(256):
            out[a, b] = min(255, max(0, _round_half_even(_round_f32(a * al + prod[b]))))
    return out


def _pairs():
    a, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    return a, b


def test_add_weighted_equals_exact_arithmetic_for_every_pair():
    a, b = _pairs()
    assert np.array_equal(O.add_weighted(a, b), _exact_blend(0.30, 0.70))
    assert np.array_equal(O.add_weighted(a, b, 0.5, 0.25), _exact_blend(0.5, 0.25))


def test_blending_a_picture_with_itself_is_the_identity():
    a = np.arange(256, dtype=np.uint8)
    assert np.array_equal(O.add_weighted(a, a), a)
    assert np.array_equal(O.add_weighted_unfused(a, a), a)


def test_the_fused_and_unfused_forms_differ_by_at_most_one():
    a, b = _pairs()
    f, u = O.add_weighted(a, b).astype(int), O.add_weighted_unfused(a, b).astype(int)
    print(f"fused vs unfused addWeighted(0.30, 0.70): {int((f != u).sum())} of 65536 pairs differ")
    assert np.abs(f - u).max() <= 1


def _frame(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _two_masks(h=24, w=32):
    m0, m1 = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
    m0[4:16, 3:20] = 1
    m1[10:22, 12:30] = 1
    return m0, m1


def test_the_last_instance_that_covers_a_pixel_tints_it():
    frame = _frame(24, 32)
    m0, m1 = _two_masks()
    c0, c1 = O.colour(0), O.colour(1)
    for order in ((0, 1), (1, 0)):
        ms, cls = [(m0, m1)[i] for i in order], [order[0], order[1]]
        t = O.tint(frame, cls, ms)
        last = O.colour(cls[1])
        both = (m0 > 0) & (m1 > 0)
        assert both.any() and (t[both] == last).all()
        assert (t[(m0 > 0) & ~both] == c0).all() and (t[(m1 > 0) & ~both] == c1).all()
        assert np.array_equal(t[(m0 == 0) & (m1 == 0)], frame[(m0 == 0) & (m1 == 0)])
    assert O.colour(7) == O.PALETTE[1] and len(O.PALETTE) == 6 and O.PALETTE[0] == (0, 255, 0) and O.PALETTE[5] == (255, 128, 0)


def test_an_empty_mask_draws_its_box_and_nothing_else():
    frame = _frame(40, 48, 1)
    cls, xyxy = np.array([2]), np.array([[5.7, 6.2, 30.9, 28.1]], np.float32)
    for mask in (np.zeros((40, 48), np.uint8), np.zeros((20, 24), np.uint8), None):
        assert O.instance_bitmap(mask, 40, 48) is None
        prims = O.display_list(40, 48, cls, xyxy, [O.instance_bitmap(mask, 40, 48)])
        assert prims == [("rect", (5, 6), (30, 28), O.colour(2), 2)]
        assert np.array_equal(O.tint(frame, cls, [None]), frame)
        pic = O.render(frame, cls, xyxy, [mask], mode=O.DRAW)
        assert np.array_equal(pic, A.rasterise(frame, prims)) and not np.array_equal(pic, frame)


def test_a_mask_gives_its_contours_before_its_box_and_the_plate_comes_last():
    m0, m1 = _two_masks()
    m0[20, 1] = 1                                                           # a second component
    prims = O.display_list(24, 32, [0, 1], np.array([[3, 4, 19, 15], [12, 10, 29, 21]], np.float32), [m0, m1],
                           plates=[None, (12, 2, 25, 9)])
    kinds = [(p[0], p[3] if p[0] != "fillrect" else p[3]) for p in prims]
    assert kinds == [("polyline", O.colour(0))] * 2 + [("rect", O.colour(0)), ("polyline", O.colour(1)), ("rect", O.colour(1)),
                                                       ("fillrect", O.colour(1))]
    assert all(p[2] is True and p[4] == 2 for p in prims if p[0] == "polyline")
    # the contour of a rectangle of set pixels: its four corners
    assert sorted(map(tuple, prims[3][1].tolist())) == [(12, 10), (12, 21), (29, 10), (29, 21)]
    # more vertices than max_points: none of the frame's contours, the status word, everything else stands
    few, word = O.display_list(24, 32, [0, 1], np.zeros((2, 4), np.float32), [m0, m1], max_points=8, with_status=True)
    assert word == O.OUTLINE_SKIPPED and [p[0] for p in few] == ["rect", "rect"]
    _, word = O.display_list(24, 32, [0, 1], np.zeros((2, 4), np.float32), [m0, m1], max_points=9, with_status=True)
    assert word == 0


def test_no_instances_return_the_copy_in_every_mode():
    frame = _frame(17, 23, 2)
    for mode in (O.DRAW, O.BLEND, O.BOTH):
        pic = O.render(frame, np.zeros(0), np.zeros((0, 4), np.float32), [], mode=mode)
        assert np.array_equal(pic, frame) and pic is not frame


RECTS = [(5, 4, 20, 12), (-6, 3, 8, 9), (30, 3, 47, 9), (10, -5, 20, 4), (10, 25, 20, 40), (-9, -9, 60, 50),      # inside, each edge, all
         (-20, 5, -3, 9), (50, 5, 70, 9), (5, -20, 9, -2), (5, 33, 9, 60),                                        # fully outside
         (7, 7, 7, 7), (0, 0, 0, 0), (39, 29, 39, 29),                                                            # one pixel
         (5, 6, 5, 20), (5, 6, 30, 6), (-3, 6, 60, 6)]                                                            # degenerate: a line


@pytest.mark.parametrize("rect", RECTS)
def test_a_filled_rectangle_equals_fill_convex_poly(rect):
    h, w = 30, 40
    xa, ya, xb, yb = rect
    want = np.zeros((h, w, 3), np.uint8)
    one = A.XY_ONE
    A._fill_convex(want, [(xa * one, ya * one), (xb * one, ya * one), (xb * one, yb * one), (xa * one, yb * one)], (1, 2, 3))
    got = np.zeros((h, w, 3), np.uint8)
    O.fill_rect(got, (xa, ya), (xb, yb), (1, 2, 3))
    assert np.array_equal(got, want)
    inside = [(x, y) for y in range(h) for x in range(w) if xa <= x <= xb and ya <= y <= yb]
    assert int((got[:, :, 0] == 1).sum()) == len(inside)
    assert np.array_equal(O.rasterise(np.zeros((h, w, 3), np.uint8), [("fillrect", (xa, ya), (xb, yb), (1, 2, 3))]), got)


def test_a_reversed_rectangle_draws_nothing():
    for rect in ((20, 4, 5, 12), (5, 12, 20, 4)):
        got = np.zeros((30, 40, 3), np.uint8)
        O.fill_rect(got, rect[:2], rect[2:], (9, 9, 9))
        assert not got.any()


def test_both_is_blend_applied_to_draw():
    frame = _frame(24, 32, 3)
    m0, m1 = _two_masks()
    small = np.zeros((12, 16), np.uint8)                                     # a letterbox-size mask: stretched by 2
    small[2:7, 3:9] = 1
    cls, xyxy = [0, 4, 1], np.array([[3, 4, 19, 15], [12, 10, 29, 21], [6, 4, 18, 14]], np.float32)
    masks, plates = [m0, m1, small], [(3, 0, 14, 3), None, (-2, 20, 9, 27)]
    draw = O.render(frame, cls, xyxy, masks, plates, mode=O.DRAW)
    both = O.render(frame, cls, xyxy, masks, plates, mode=O.BOTH)
    assert np.array_equal(both, O.render(frame, cls, xyxy, masks, plates, mode=O.BLEND, annotated=draw))
    assert not np.array_equal(both, draw) and not np.array_equal(draw, frame)
    # where nothing was drawn or tinted the blend leaves the frame's byte
    bitmaps = [O.instance_bitmap(m, 24, 32) for m in masks]
    assert np.array_equal(bitmaps[2], np.kron(small, np.ones((2, 2), np.uint8)))
    quiet = (draw == frame).all(axis=-1) & ~np.any([b > 0 for b in bitmaps], axis=0)
    assert quiet.any() and np.array_equal(both[quiet], frame[quiet])
    with pytest.raises(ValueError):
        O.render(frame, cls, xyxy, masks, mode=0)


def test_label_items_are_the_references_strings_and_origins():
    cls, conf = np.array([0, 1, 5]), np.array([0.876, 0.5, 0.999])
    xyxy = np.array([[10.9, 50.2, 60, 80], [300.5, 5.9, 320, 30], [-4.2, 28.0, 9, 40]], np.float32)
    items = O.label_items(cls, conf, xyxy, {0: "stitch", 1: "fabric"})
    assert [i[0] for i in items] == ["stitch 0.88", "fabric 0.50", "5 1.00"]
    assert [i[1] for i in items] == [(14, 40), (304, 18), (0, 18)]           # (x1 + 4, max(20, y1 - 8) - 2)
    assert all(i[2:] == ("FONT_HERSHEY_SIMPLEX", 0.55, (0, 0, 0), 2, "LINE_AA") for i in items)
    assert [i[0] for i in O.label_items(cls, conf, xyxy, ["a", "b"])] == ["a 0.88", "b 0.50", "5 1.00"]
    assert [i[0] for i in O.label_items(cls, conf, xyxy, None)] == ["0 0.88", "1 0.50", "5 1.00"]


def test_annotate_result_needs_the_engine_that_made_the_result():
    class Bare:
        boxes = None
    with pytest.raises(RuntimeError, match="Engine"):
        O.annotate_result(np.zeros((4, 4, 3), np.uint8), Bare())
