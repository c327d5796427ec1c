"""Pins tests/misc_ref.py on the CPU: the float64 references of the SPPF pools, the nearest 2x upsample and the decode against torch
and against the oracle's own decode, the pooled-output rule against an exhaustive search, and the DFL bound against fp32
emulations of both forms the kernels use, on every logit set the GPU tests (test_gpu_misc_ops.py) run."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import h2_ref
import misc_ref as M


@pytest.mark.parametrize("H,W", [(1, 1), (1, 9), (9, 1), (3, 4), (7, 11), (20, 20)])
def test_pool_ref_is_three_chained_max_pools(H, W):
    rng = np.random.default_rng(H * 100 + W)
    x = rng.standard_normal((2, H, W, 5))
    x[0] = -np.abs(x[0]) - 1.0                     # an all-negative frame: a pool padded with 0 would answer 0 at every edge
    t = torch.from_numpy(x).permute(0, 3, 1, 2)
    for got in M.pool_ref(x):
        t = F.max_pool2d(t, 5, 1, 2)
        assert np.array_equal(got, t.permute(0, 2, 3, 1).numpy())


def test_up_ref_is_nearest_interpolate():
    x = np.random.default_rng(0).standard_normal((2, 3, 5, 4)).astype(np.float32)
    ref = F.interpolate(torch.from_numpy(x).permute(0, 3, 1, 2), scale_factor=2, mode="nearest").permute(0, 2, 3, 1).numpy()
    assert np.array_equal(M.up_ref(x), ref)
    bits = np.random.default_rng(1).integers(0, 2 ** 32, (1, 2, 2, 4), dtype=np.uint32)        # any bit pattern: a copy
    assert np.array_equal(M.up_ref(bits)[0, 3, 2], bits[0, 1, 1])


def _brute_verdict(in_val, in_bits, out_val, out_bits):
    B, H, W, C = in_val.shape
    res = []
    for r, ov, ob in zip(M.POOL_RADII, out_val, out_bits):
        ok = np.zeros(in_val.shape, bool)
        for b, y, x, c in np.ndindex(B, H, W, C):
            win_v = in_val[b, max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1, c]
            win_b = in_bits[b, max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1, c]
            ok[b, y, x, c] = ov[b, y, x, c] == win_v.max() and ob[b, y, x, c] in win_b
        res.append(ok)
    return res


def test_pool_verdict_is_the_exhaustive_rule():
    """Small integers and both zeros, so that windows hold many equal values with different bits; the outputs under test are a
    correct pool, one that keeps the other zero, and corruptions of value and of bits -- each judged as the exhaustive search does."""
    rng = np.random.default_rng(3)
    val = rng.integers(-2, 2, (1, 6, 7, 3)).astype(np.float32)
    val[rng.random(val.shape) < 0.3] = -0.0
    bits = val.view(np.uint32)
    ref = [r.astype(np.float32) for r in M.pool_ref(val)]
    good = [r + np.float32(0.0) for r in ref]                                  # every zero as +0
    for out in (good, [np.where(r == 0, np.float32(-0.0), r) for r in ref],    # every zero as -0: wrong where the window has no -0
                [np.where(rng.random(r.shape) < 0.2, r + 1, r) for r in ref],  # wrong values
                [np.where(rng.random(r.shape) < 0.2, np.float32(1.0), r) for r in ref]):
        out = [np.ascontiguousarray(o, np.float32) for o in out]
        got = M.pool_verdict(val, bits, out, [o.view(np.uint32) for o in out])
        want = _brute_verdict(val.astype(np.float64), bits, out, [o.view(np.uint32) for o in out])
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
    # h2 pairs of equal value and different bits: (hi, lo) and (hi + one step, lo - one step); either is a correct answer
    hi = np.array([1024.0, 1025.0]); lo = np.array([0.5, -0.5])
    pair_bits = h2_ref.bits(hi, lo).view(np.uint32)
    assert h2_ref.dec(hi, lo)[0] == h2_ref.dec(hi, lo)[1] and pair_bits[0] != pair_bits[1]
    v = np.full((1, 1, 3, 1), -3.0); b = np.full((1, 1, 3, 1), h2_ref.bits(-48.0, 0.0).view(np.uint32))      # every window is the whole map
    v[0, 0, 0, 0], v[0, 0, 2, 0] = h2_ref.dec(hi, lo); b[0, 0, 0, 0], b[0, 0, 2, 0] = pair_bits
    ref = M.pool_ref(v)
    for keep in pair_bits:
        ob = [np.full(r.shape, keep) for r in ref]
        assert all(x.all() for x in M.pool_verdict(v, b, ref, ob))
    ob = [np.full(r.shape, h2_ref.bits(1026.0, -1.5).view(np.uint32)) for r in ref]          # the same value again, from no element
    assert h2_ref.dec(1026.0, -1.5) == v[0, 0, 0, 0] and not any(x.any() for x in M.pool_verdict(v, b, ref, ob))


def _oracle_decode(box, cls, mc, levels, strides):
    """The decode of oracle/model.py (OracleModel.head) on given head tensors: its convs replaced by a lookup."""
    from oracle.model import OracleModel
    o = object.__new__(OracleModel)
    o.spec = types.SimpleNamespace(reg_max=16, levels=[(None, h, w, s) for (h, w), s in zip(levels, strides)])
    B = box[0].shape[0]
    planted = {}
    for l, (h, w) in enumerate(levels):
        for tower, src in (("cv2", box), ("cv3", cls), ("cv4", mc)):
            planted[f"model.22.{tower}.{l}.2"] = torch.from_numpy(src[l]).reshape(B, h, w, -1).permute(0, 3, 1, 2).contiguous()
    o.conv = lambda x, name, res=None, out_fp32=False: planted.get(name, x)
    pred, _ = o.head([torch.zeros(B, 1, h, w) for h, w in levels])
    return pred.permute(0, 2, 1).double().numpy()


@pytest.mark.parametrize("levels", M.DECODE_LEVELS)
def test_decode_ref_against_the_oracles_decode(levels):
    """The oracle decodes in fp32 with torch's softmax: its boxes must lie within the fp32 bound of decode_ref, its scores within
    4 fp32 ulps (exactly 0 and 1 at -100 and +100), the coefficients equal -- the same statement the GPU tests make about the kernels."""
    nc, nm = 80, 32
    box, cls, mc, _ = M.decode_inputs(levels, 2, nc, nm, seed=1)
    pred, E, bound = M.decode_ref(box, cls, mc, levels, M.DECODE_STRIDES)
    assert pred.shape == (2, sum(h * w for h, w in levels), 4 + nc + nm)
    got = _oracle_decode(box, cls, mc, levels, M.DECODE_STRIDES)
    assert (np.abs(got[..., :4] - pred[..., :4]) <= bound).all()
    assert M.scores_ok(got[..., 4:4 + nc], pred[..., 4:4 + nc], np.concatenate(cls, 1)).all()
    assert np.array_equal(got[..., 4 + nc:], pred[..., 4 + nc:])
    # flat rows: every side is 7.5 bins, so a box is centred on its cell and 15 cells wide, levels concatenated in order
    flat = [np.zeros_like(b) for b in box]
    pred, _, _ = M.decode_ref(flat, cls, mc, levels, M.DECODE_STRIDES)
    a = levels[0][0] * levels[0][1]
    (h1, w1), s1 = levels[1], M.DECODE_STRIDES[1]
    assert pred[1, a + w1 + 2, :4].tolist() == [2.5 * s1, 1.5 * s1, 15.0 * s1, 15.0 * s1]


def test_dfl_ref_on_rows_with_known_answers():
    v = np.full((3, 16), -1000.0)
    v[0, 0] = v[1, 7] = v[2, 15] = 0.0
    d, E = M.dfl_ref(v)
    assert d.tolist() == [0.0, 7.0, 15.0]                       # one-hot: the tails underflow to exactly 0
    assert np.allclose(E, 30 * 2.0 ** -22 + 2.0 ** -15)
    d, E = M.dfl_ref(np.full((1, 16), 88.0))
    assert d[0] == 7.5 and abs(E[0] - (30 * 2.0 ** -22 + 2.0 ** -15)) < 1e-12


@pytest.mark.parametrize("name", M.BOX_SETS + tuple(f"normal {s}" for s in (0.5, 2, 5, 20)))
def test_fp32_softmax_expectation_sits_inside_the_bound(name):
    """Both fp32 forms, on the sets the GPU tests use (and the scales between them), stay within E -- measured: below 0.12 E."""
    v = M.box_rows(name, 20000, np.random.default_rng(11))
    d, E = M.dfl_ref(v)
    for form in (M.dfl_fp32_expf, M.dfl_fp32_exp2):
        ratio = (np.abs(form(v) - d) / E).max()
        print(f"{name:12s} {form.__name__}: max |d_fp32 - d| / E = {ratio:.3f}")
        assert ratio <= 1.0
    if name.startswith("one-hot"):
        assert (v.max(1) - np.sort(v, 1)[:, -2] > 50).all()      # peaked: the spread the issue asks for
    assert E.min() >= 2.0 ** -15 and E.max() < 3e-3


def test_decode_inputs_hold_every_set_at_every_level():
    for levels in M.DECODE_LEVELS:
        box, cls, mc, which = M.decode_inputs(levels, 2, 2, 32, seed=0)
        a0 = 0
        for l, (h, w) in enumerate(levels):
            assert set(which[:, a0:a0 + h * w].reshape(-1)) == set(range(len(M.BOX_SETS)))
            assert set(M.CLS_PLANTED) <= set(cls[l].reshape(-1).tolist())
            assert np.abs(cls[l]).max() <= 100 and (np.abs(cls[l])[np.abs(cls[l]) < 100] < 80).all()
            a0 += h * w
