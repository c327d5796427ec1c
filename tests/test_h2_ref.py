"""h2_ref.py (the h2 scheme in numpy float64) against the library's host-side encode / decode, and the host-side preconditions of
the bit-for-bit h2 cases of test_gpu_conv.py / test_gpu_conv1x1_wreg.py.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import h2_ref
import test_gpu_conv as tc
import test_gpu_conv1x1_wreg as tw

EDGES = [0.0, 2.0 ** -24 / 16, 8e-3, 4093.9, 4094.0, 4094.5, 4095.0, 1e5, float("inf")]


def _sweep():
    rng = np.random.default_rng(2024)
    mag = 2.0 ** rng.uniform(-30, 13, 40000)
    v = np.concatenate([mag * rng.choice([-1.0, 1.0], mag.size), EDGES, [-e for e in EDGES]])
    return v.astype(np.float32)


def test_h2_encode_decode_equal_the_scheme_bit_for_bit(lib_built):
    v = _sweep()
    hi, lo = h2_ref.enc_act(v)
    want = h2_ref.bits(hi, lo)
    got = lib_built.h2_encode(torch.from_numpy(v))
    assert got.dtype == torch.float32 and np.array_equal(got.view(torch.int32).numpy(), want)
    back = lib_built.h2_decode(got).numpy()
    assert np.array_equal(back.astype(np.float64), h2_ref.dec(hi, lo))
    assert np.isfinite(back).all() and np.abs(back).max() == 4094.0


def test_encode_saturates_and_keeps_the_range():
    """|v| <= 4094 saturating with lo = 0 at the limit; below it the pair keeps >= 21 bits while lo is a normal fp16 number."""
    for v, d in ((4094.0, 4094.0), (4095.0, 4094.0), (1e5, 4094.0), (np.inf, 4094.0), (-4094.5, -4094.0), (-np.inf, -4094.0)):
        hi, lo = h2_ref.enc_act(v)
        assert float(hi) == 16 * d and float(lo) == 0.0 and float(h2_ref.dec(hi, lo)) == d
    assert int(h2_ref.bits(*h2_ref.enc_act(-0.0))) == 0
    v = _sweep()
    v = v[(np.abs(v) >= 8e-3) & (np.abs(v) <= 4094)].astype(np.float64)
    assert (np.abs(h2_ref.q_act(v) - v) <= np.abs(v) * 2.0 ** -21).all()
    small = np.float64(2.0 ** -24 / 16)
    assert float(h2_ref.q_act(small)) == small and float(h2_ref.q_act(small / 4)) == 0.0      # the absolute floor


def test_enc_w_scale():
    for mx, sw in ((1.0, 2.0 ** 13), (1 + 2.0 ** -12, 2.0 ** 13), (0.999, 2.0 ** 14), (2.0 ** -20, 2.0 ** 33), (0.0, 1.0)):
        wh, wl, got = h2_ref.enc_w(np.array([mx, -mx / 3], np.float32))
        assert got == sw and (mx == 0 or 2.0 ** 13 <= np.abs(wh).max() <= 2.0 ** 14)


def _check_split(x, w, b, k, s, kind, res, want):
    assert np.array_equal(h2_ref.conv_scheme(x, w, b, k, s, kind, res=res, act=False), want)
    enc = h2_ref.conv_scheme(x, w, b, k, s, kind, res=res, act=False, encode=True)
    assert np.array_equal(h2_ref.dec(*[a.astype(np.float64) for a in _halves(enc)]), want)
    # a kernel that lost (or misplaced into a zero) its lo weight operand: differs in most outputs (K = 16: 88 %, K >= 48: 98 %)
    hi_only = h2_ref.conv_scheme(x, w, b, k, s, kind, res=res, act=False, encode=True, hi_only_w=True)
    assert (hi_only != enc).mean() > 0.8
    # ... and one that lost the activations' lo halves
    xh_only = h2_ref.dec(h2_ref.enc_act(x)[0], 0.0).astype(np.float32)
    assert (h2_ref.conv_scheme(xh_only, w, b, k, s, kind, res=res, act=False, encode=True) != enc).mean() > 0.8


def _halves(dwords):
    u = dwords.view(np.uint32)
    return (u & 0xFFFF).astype(np.uint16).view(np.float16), (u >> 16).astype(np.uint16).view(np.float16)


@pytest.mark.parametrize("case", tc.CASES, ids=lambda c: f"k{c[0]}s{c[1]}kind{c[2]}_{c[3]}to{c[4]}_{c[5]}x{c[6]}")
def test_split_construction_is_exact_conv_cases(case):
    k, s, kind = case[:3]
    _, x, w, b, res, want = tc.split_exact_case(case)       # asserts split-exactness and exact h2 outputs
    _check_split(x, w, b, k, s, kind, res, want)


@pytest.mark.parametrize("c1,c2,H,W,ex", sorted({(c[0], c[1], c[2], c[3], tuple(sorted(c[-1].items()))) for c in tw.CASES + tw.PK_CASES}))
def test_split_construction_is_exact_1x1_cases(c1, c2, H, W, ex):
    _, x, w, b, res, want = tw.split_exact_case(c1, c2, H, W, dict(ex), 12345 + c1)
    _check_split(x, w, b, 1, 1, 1, res, want)


def test_exactness_counts_what_it_says():
    x = np.array([[[[2 + 3 * 2.0 ** -13, -1.0]]]], np.float32)            # xh = 32, -16; xl = 3 * 2^-9, 0
    w = np.array([[[[1 + 2.0 ** -12]], [[-1.0]]]], np.float32)            # wh = 8192, -8192; wl = 2, 0
    g, n = h2_ref.exactness(x, w, 1, 1, 1)
    assert g == 16.0 and n == (8192 * (32 + 3 * 2.0 ** -9) + 2 * 32 + 8192 * 16) / 16


@pytest.mark.parametrize("k,s,kind,c1,c2,H,W", [(3, 1, 0, 24, 20, 7, 9), (3, 2, 1, 20, 24, 9, 7), (1, 1, 1, 40, 24, 5, 6), (2, 2, 2, 24, 20, 4, 5)])
def test_conv_scheme_is_the_conv_of_the_decoded_operands_less_the_lo_lo_term(k, s, kind, c1, c2, H, W):
    rng = np.random.default_rng(k * 10 + s + kind)
    x = rng.standard_normal((2, H, W, c1)).astype(np.float32) * 2.0 ** rng.integers(-10, 4, (1, 1, 1, c1))
    wshape = (c1, c2, k, k) if kind == 2 else (c2, c1, k, k)
    w = (rng.standard_normal(wshape) * 2.0 ** rng.integers(-12, 1, (wshape[0], 1, 1, 1)) / np.sqrt(c1 * k * k)).astype(np.float32)
    b = rng.standard_normal(c2).astype(np.float32)
    got = h2_ref.conv_scheme(x, w, b, k, s, kind, act=False)
    xq = torch.from_numpy(h2_ref.q_act(x)).permute(0, 3, 1, 2)
    wq, bq = torch.from_numpy(h2_ref.q_w(w)), torch.from_numpy(b.astype(np.float64))
    ref = (F.conv_transpose2d(xq, wq, bq, stride=s) if kind == 2 else F.conv2d(xq, wq, bq, stride=s, padding=k // 2)).permute(0, 2, 3, 1).numpy()
    (xh, xl), (wh, wl, sw) = h2_ref.enc_act(x), h2_ref.enc_w(w)
    dropped = h2_ref.lin(np.abs(xl), np.abs(wl), k, s, kind) / (16 * sw)
    total = h2_ref.lin(np.abs(xh), np.abs(wh), k, s, kind) / (16 * sw) + np.abs(b)
    assert dropped.max() > 0
    assert (np.abs(got - ref) <= dropped + total * 2.0 ** -45).all()          # 2^-45: float64 rounding of the two evaluations
    # kind 0 adds the SiLU in float64, the residual is added as stored
    res = rng.standard_normal(got.shape).astype(np.float32)
    full = h2_ref.conv_scheme(x, w, b, k, s, kind, res=res, act=True)
    assert np.allclose(full, got / (1 + np.exp(-got)) + h2_ref.q_act(res), rtol=1e-15, atol=0)
