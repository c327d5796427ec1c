"""The range boundaries of masks_group_kernel's partition by weight, restated on the host (tools/post_balance.py mirrors
mask_weight_bound of post.hip statement for statement): the closed form from the prefix sums must cut the frame-major (frame, tile)
list exactly where the definition does -- item i goes to XCD k when its exclusive cumulative weight lies in [k W / 8, (k + 1) W / 8)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import post_balance as pb  # noqa: E402


@pytest.mark.parametrize("c", [0, 1, 32])
def test_closed_form_is_the_definition(c):
    rng = np.random.default_rng(c)
    cases = [(120, 0, 3, 0, 0, 1, 0, 64, 2), (5,), (0,), (0, 0, 0), (0, 0, 7), (7, 0, 0), (300,) * 64]
    cases += [tuple(rng.integers(0, 40, rng.integers(1, 70)) * rng.integers(0, 2, 1)) for _ in range(20)]
    cases += [tuple(rng.integers(0, 300, rng.integers(1, 70))) for _ in range(40)]
    for counts in cases:
        for tiles in (1, 20, 100):
            off = np.concatenate([[0], np.cumsum(counts)])
            weight = np.repeat(np.asarray(counts) + c, tiles)
            want = pb.bounds_weighted(weight, 8)
            got = [pb.bound_closed_form(off, tiles, c, k) for k in range(9)]
            assert got[0] == 0 and got[8] == len(weight) and all(a <= b for a, b in zip(got, got[1:]))
            if c > 0 or min(counts) > 0:
                assert got == want.tolist(), (counts, tiles)
            else:                       # weightless items may sit on either side of a boundary: the weighted ones may not
                cum = np.concatenate([[0], np.cumsum(weight)])
                assert [int(cum[g]) for g in got[:8]] == [int(cum[w]) for w in want[:8]], (counts, tiles)


def test_a_capacity_cuts_the_prefix_sums():
    off = np.minimum(np.concatenate([[0], np.cumsum((120, 0, 3, 0, 0, 1, 0, 64, 2))]), 100)
    got = [pb.bound_closed_form(off, 100, 32, k) for k in range(9)]
    weight = np.repeat(off[1:] - off[:-1] + 32, 100)
    assert got == pb.bounds_weighted(weight, 8).tolist()
