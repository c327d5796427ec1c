"""h2 (split-fp16 pair) single convs over the storage's dynamic range, one shape per kernel family, against the scheme itself.

The h2 storage is lossy by design at small scales (16 v = hi + lo in fp16: lo is subnormal below |v| ~ 8e-3 and the pair has an
absolute floor of 2^-28), so a kernel is NOT compared with the true product here but with h2_ref.conv_scheme: the same
sum wh (xh + xl) + wl xh on the same encoded operands, in float64.  The only further error of a correct kernel is its fp32
accumulation and the order of its sums; that is measured on the reference alone, per output channel, as
    e32 = max |float32 CPU conv - float64 conv|  on the decoded operands,
and every kind-1 case asserts, per output channel and relative to nothing but that,
    |got - conv_scheme| <= 3 e32 + one h2 unit in the last place at the channel's maximum
(3: the slack test_fp32_box_error_is_the_fp32_floor gives the same quantity; the unit covers the final encode).  Per channel,
because one power of two SW scales all weights of a conv: a channel 2^-12 below the conv's largest keeps 11 bits in wh and has a
subnormal wl, and a bound relative to the layer's maximum would not see it lose them.

The saturation cases hold the encode of every epilogue to +-4094 (h2_enc clamps: 4094 * 16 = 65504 is the largest fp16;
unclamped, hi = inf and lo = -inf, and every later use of the pair is NaN).

Measured (MI355X): RATIOS below -- the largest excess of |got - scheme| over that one unit is 1.23 e32 (persistent 3x3 at
x ~ N(0, 1)), 0.13 .. 0.98 e32 in the other families; the channels 2^-12 below their conv's largest and the activations at 2^-16
(subnormal hi AND lo halves) are no worse than the rest, and test_subnormal_lo_operands_are_kept_exactly settles why: the fp16
MFMA keeps subnormal operands.  With SiLU: 0.17 of 4e-6 max(1, |ref|) per channel and 0.37 of the derived bound (_silu_bound).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import h2_ref
from gpu_util import need_gpu

pytestmark = pytest.mark.gpu

# family: k, s, kind-2 (ConvTranspose)?, c1, c2, H, W, persistent?, environment, forced tile
FAMILIES = {
    "3x3_pk": (3, 1, False, 64, 64, 24, 20, True, {}, (0, 0)),
    "3x3_tile": (3, 1, False, 32, 32, 9, 11, False, {}, (0, 0)),
    "3x3_s2": (3, 2, False, 32, 64, 21, 19, False, {}, (0, 0)),
    "1x1_tile": (1, 1, False, 48, 256, 7, 9, False, {"VTI_NO_PK1": "1"}, (0, 0)),
    "1x1_pk": (1, 1, False, 64, 64, 8, 20, True, {}, (1, 80)),
    "deconv": (2, 2, True, 64, 64, 6, 5, False, {}, (0, 0)),
}
# Measured on an MI355X, per family over all its kind-1 cases: the largest (|got - scheme| - unit) / e32 over the channels, i.e.
# what the cap of 3 applies to, and the case that gave it (each case prints its own figure).  Below |v| ~ 1e-3 the unit alone
# covers the difference (the encode's rounding: |d| is half a unit there); no case came near the cap.
RATIOS = {
    "3x3_pk": (1.23, "activations 2^0"),
    "3x3_tile": (0.87, "activations 2^4"),
    "3x3_s2": (0.98, "conv times 2^10"),
    "1x1_tile": (0.44, "activations 2^4"),
    "1x1_pk": (0.43, "output channels 2^0 .. 2^-12"),
    "deconv": (0.13, "activations 2^-4"),
}
B = 2
CAP = 3.0


def _shapes(fam):
    k, s, tr, c1, c2, H, W = FAMILIES[fam][:7]
    return k, s, tr, c1, c2, H, W, ((c1, c2, k, k) if tr else (c2, c1, k, k))


def _operands(fam, seed, gain=1.0):
    """x ~ N(0, 1) NHWC, w ~ N(0, gain^2 / K) in the conv's layout, b ~ 0.1 N(0, 1)."""
    k, s, tr, c1, c2, H, W, wshape = _shapes(fam)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, H, W, c1)).astype(np.float32)
    w = (rng.standard_normal(wshape) * gain / np.sqrt(c1 * (1 if tr else k * k))).astype(np.float32)
    b = (rng.standard_normal(c2) * 0.1).astype(np.float32)
    return rng, x, w, b


def _per_out(w, f, tr):
    return w * (f[None, :, None, None] if tr else f[:, None, None, None]).astype(np.float32)


def _per_in(w, f, tr):
    return w * (f[:, None, None, None] if tr else f[None, :, None, None]).astype(np.float32)


def _factors(rng, n, lo, hi=0):
    """2^u, u drawn per channel from lo..hi with both ends present."""
    u = rng.integers(lo, hi + 1, n)
    u[rng.permutation(n)[:2]] = (lo, hi)
    return 2.0 ** u


def _launch(fam, x, w, b, kind, monkeypatch, res=None):
    import vti_amd
    k, s, tr, c1, c2, H, W, pk, env, tile = FAMILIES[fam]
    for key in ("VTI_NO_PK", "VTI_NO_PK1", "VTI_PK_MAX_WGS"):
        monkeypatch.delenv(key, raising=False)
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    enc = lambda a: vti_amd.h2_encode(torch.from_numpy(np.ascontiguousarray(a))).cuda()
    out, _, cfg = vti_amd.debug_conv2d(enc(x), w, b, k, s, 2 if tr else kind, "h2", res=None if res is None else enc(res), tile=tile)
    torch.cuda.synchronize()
    assert bool(cfg["pk"]) == pk, (fam, cfg)
    return out.cpu()


def _e32(fam, x, w, b, res=None):
    """max |float32 CPU conv - float64 conv| per output channel, on the operands as the kernel holds them (decoded)."""
    k, s, tr = FAMILIES[fam][:3]
    xq = torch.from_numpy(h2_ref.q_act(x)).permute(0, 3, 1, 2)
    wq, bq = torch.from_numpy(h2_ref.q_w(w)), torch.from_numpy(np.asarray(b, np.float64))
    rq = None if res is None else torch.from_numpy(h2_ref.q_act(res)).permute(0, 3, 1, 2)

    def conv(t):
        y = F.conv_transpose2d(xq.to(t), wq.to(t), bq.to(t), stride=s) if tr else F.conv2d(xq.to(t), wq.to(t), bq.to(t), stride=s, padding=k // 2)
        return (y if rq is None else y + rq.to(t)).double()
    assert torch.equal(xq.float().double(), xq) and torch.equal(wq.float().double(), wq)        # the decoded operands are fp32 numbers
    return (conv(torch.float32) - conv(torch.float64)).abs().amax((0, 2, 3)).numpy()


def _check(fam, name, got_bits, x, w, b, kind, res=None, saturating=False):
    """The kind-1 bound, per output channel.  Returns the largest |got - scheme| / e32."""
    import vti_amd
    k, s, tr = FAMILIES[fam][:3]
    got = vti_amd.h2_decode(got_bits).double().numpy()
    assert np.isfinite(got).all(), f"{fam} {name}: {np.count_nonzero(~np.isfinite(got))} non-finite outputs"
    raw = h2_ref.conv_scheme(x, w, b, k, s, 2 if tr else kind, res=res, act=False)
    want = np.clip(raw, -h2_ref.H2_MAX, h2_ref.H2_MAX)
    assert saturating or np.array_equal(raw, want), f"{fam} {name}: the case leaves the range"
    d = np.abs(got - want).max((0, 1, 2))
    vmax = np.abs(want).max((0, 1, 2))
    e32 = _e32(fam, x, w, b, res)
    bound = CAP * e32 + h2_ref.unit(vmax)
    c = int(np.argmax(d / bound))
    units = h2_ref.unit(vmax)
    ratio = float((np.maximum(d - units, 0) / np.maximum(e32, 1e-300))[e32 > 0].max()) if (e32 > 0).any() else 0.0     # what the cap of 3 applies to
    print(f"h2range {fam:9s} {name:14s} max (d - unit)/e32 {ratio:6.3f}  worst channel {c}: |d| {d[c]:.3e} e32 {e32[c]:.3e} unit {h2_ref.unit(vmax[c]):.3e} max {vmax[c]:.3e}  d/bound {d[c] / bound[c]:.3f}")
    assert (d <= bound).all(), f"{fam} {name}: channel {c}: |got - scheme| {d[c]:.3e} > 3 * {e32[c]:.3e} + {h2_ref.unit(vmax[c]):.3e} (channel max {vmax[c]:.3e})"
    if saturating:
        past = np.abs(raw) > 4095
        assert past.mean() > 0.3 and (raw[past] > 0).any() and (raw[past] < 0).any() and (np.abs(raw) > 65504).any(), past.mean()
        assert np.array_equal(got[past], np.sign(raw[past]) * h2_ref.H2_MAX)
    return ratio


@pytest.mark.parametrize("e", [-16, -12, -8, -4, 0, 4, 7])
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_activation_scale(fam, e, monkeypatch):
    """x = N(0, 1) 2^e: from lo halves that are all subnormal or zero (e = -16) to the top of the range (e = 7: |x| up to ~600,
    outputs of standard deviation 256, sixteen of them below the limit)."""
    need_gpu()
    _, x, w, b = _operands(fam, 100 + e, gain=2.0)
    x = x * np.float32(2.0 ** e)
    b = b * np.float32(2.0 ** e)
    _check(fam, f"act 2^{e}", _launch(fam, x, w, b, 1, monkeypatch), x, w, b, 1)


@pytest.mark.parametrize("side", ["out", "in"])
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_channel_weight_scale(fam, side, monkeypatch):
    """Channels of one conv 2^0 .. 2^-12 apart (both ends present), as BN folding leaves them: one SW serves them all, so the
    small channels' lo halves are subnormal fp16 MFMA operands.  The bias follows its output channel."""
    need_gpu()
    k, s, tr, c1, c2 = _shapes(fam)[:5]
    rng, x, w, b = _operands(fam, 200 + (side == "in"))
    if side == "out":
        f = _factors(rng, c2, -12)
        w, b = _per_out(w, f, tr), b * f.astype(np.float32)
    else:
        w = _per_in(w, _factors(rng, c1, -12), tr)
    _check(fam, f"w per {side}", _launch(fam, x, w, b, 1, monkeypatch), x, w, b, 1)


@pytest.mark.parametrize("e", [-20, 10])
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_conv_weight_scale(fam, e, monkeypatch):
    """The whole conv times 2^-20 and 2^10 (bias alike): SW and alpha move, nothing else may."""
    need_gpu()
    _, x, w, b = _operands(fam, 300, gain=0.5)
    w, b = w * np.float32(2.0 ** e), b * np.float32(2.0 ** e)
    _check(fam, f"conv 2^{e}", _launch(fam, x, w, b, 1, monkeypatch), x, w, b, 1)


@pytest.mark.parametrize("fam", list(FAMILIES))
def test_zero_weights_give_the_bias(fam, monkeypatch):
    need_gpu()
    _, x, w, b = _operands(fam, 400)
    out = _launch(fam, x, np.zeros_like(w), b, 1, monkeypatch)
    want = torch.from_numpy(h2_ref.bits(*h2_ref.enc_act(b))).expand(out.shape)
    assert torch.equal(out.view(torch.int32), want)


@pytest.mark.parametrize("pk", [False, True], ids=["1x1_tile", "1x1_pk"])
def test_subnormal_lo_operands_are_kept_exactly(pk, monkeypatch):
    """Does the fp16 MFMA keep SUBNORMAL A / B operands?  (The ISA text states it for f32 operands and for C / D only.)  A
    split-exact case, fp32 output, in which EVERY nonzero lo half of both operands is a subnormal fp16 number:
      16 x = +-(2 + xf 2^-16)          -> xh = +-2, xl = +-xf 2^-16                (xf in 0..3; input channel 0 is all zero)
      w SW = +-(1 + wf 2^-16), SW 2^13 -> wh = +-1, wl = +-wf 2^-16                (wf in 0..3; input channel 0 holds +-1 = 8192 / SW,
                                                                                    which sets SW and meets only zeros)
    Every product is a multiple of 2^-16 and sum|terms| stays below 2^24 of them, so the fp32 result is exact in any order and
    must equal the scheme BIT FOR BIT; with the subnormal operands flushed to zero it differs in most outputs (asserted on the
    host).  Measured on the MI355X: equal -- the subnormal halves are kept."""
    need_gpu()
    import vti_amd
    c1 = c2 = 64
    H, W = 8, 20
    rng = np.random.default_rng(77)
    sgn = lambda shape: rng.choice([-1.0, 1.0], shape)
    x = sgn((B, H, W, c1)) * rng.integers(0, 2, (B, H, W, c1)) * (2.0 + rng.integers(0, 4, (B, H, W, c1)) * 2.0 ** -16) / 16
    w = sgn((c2, c1, 1, 1)) * rng.integers(0, 2, (c2, c1, 1, 1)) * (1.0 + rng.integers(0, 4, (c2, c1, 1, 1)) * 2.0 ** -16) / 8192
    x[..., 0], w[:, 0] = 0.0, sgn((c2, 1, 1))
    x, w, b = x.astype(np.float32), w.astype(np.float32), np.zeros(c2, np.float32)
    (xh, xl), (wh, wl, sw) = h2_ref.enc_act(x), h2_ref.enc_w(w)
    assert sw == 8192 and np.array_equal(h2_ref.dec(xh, xl), x.astype(np.float64)) and np.array_equal((wh + wl) / sw, w.astype(np.float64))
    for lo in (xl, wl):     # every nonzero lo half is subnormal, and there are many
        assert (np.abs(lo[lo != 0]) < 2.0 ** -14).all() and (lo != 0).mean() > 0.3
    g, n = h2_ref.exactness(x, w, 1, 1, 1)
    assert g == 2.0 ** -16 and n < h2_ref.SPLIT_EXACT, (g, n)
    want = h2_ref.conv_scheme(x, w, b, 1, 1, 1, act=False)
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
    flushed = h2_ref.scheme_acc(xh, np.zeros_like(xl), wh, np.zeros_like(wl), 1, 1, 1) / (16 * sw)
    assert (flushed != want).mean() > 0.9
    monkeypatch.delenv("VTI_NO_PK1", raising=False)
    if not pk:
        monkeypatch.setenv("VTI_NO_PK1", "1")
    xd = vti_amd.h2_encode(torch.from_numpy(x)).cuda()
    out, _, cfg = vti_amd.debug_conv2d(xd, w, b, 1, 1, 1, "h2", out_f32=True, tile=(1, 80) if pk else (0, 0))
    torch.cuda.synchronize()
    assert bool(cfg["pk"]) == pk, cfg
    got = out.cpu().double().numpy()
    assert np.array_equal(got, want), f"differing outputs: {(got != want).mean():.3f}; equal to the flushed evaluation: {(got == flushed).mean():.3f}"


def _silu_bound(pre, ref, e32, unit):
    """The fast SiLU of the kernels, x * rcp(1 + exp2(x * -log2 e)), on a pre-activation that is off by at most `e32_bound`:
    |silu'| <= 1.1, and relative to the result (6 + 1.5 |x|) 2^-24 -- the rounded product x * c and c itself move exp2's
    argument by 1.5 |y| 2^-24, i.e. the exponential by 1.5 |x| 2^-24 relatively; v_exp_f32 and v_rcp_f32 are 1 ulp (2^-23)
    each, the add and the last multiply half an ulp each."""
    return 1.1 * CAP * e32 + (6 + 1.5 * np.abs(pre).max((0, 1, 2))) * 2.0 ** -24 * np.abs(ref).max((0, 1, 2)) + unit


def _check_silu(fam, name, got_bits, x, w, b, tol, res=None, k_s=None):
    """Per output channel: the file's h2 bound with SiLU, tol * max(1, |ref|), with the channel's own maximum; and, so that a
    channel far below 1 is held to something, the bound derived in _silu_bound."""
    import vti_amd
    k, s = k_s or FAMILIES[fam][:2]
    got = vti_amd.h2_decode(got_bits).double().numpy()
    assert np.isfinite(got).all()
    pre = h2_ref.conv_scheme(x, w, b, k, s, 1, act=False)
    with np.errstate(over="ignore"):
        ref = np.clip(h2_ref.conv_scheme(x, w, b, k, s, 0, res=res), -h2_ref.H2_MAX, h2_ref.H2_MAX)
    d = np.abs(got - ref).max((0, 1, 2))
    vmax = np.abs(ref).max((0, 1, 2))
    xq = torch.from_numpy(h2_ref.q_act(x)).permute(0, 3, 1, 2)
    wq, bq = torch.from_numpy(h2_ref.q_w(w)), torch.from_numpy(np.asarray(b, np.float64))
    e32 = (F.conv2d(xq.float(), wq.float(), bq.float(), stride=s, padding=k // 2).double() - F.conv2d(xq, wq, bq, stride=s, padding=k // 2)).abs().amax((0, 2, 3)).numpy()
    derived = _silu_bound(pre, ref, e32, h2_ref.unit(vmax))
    c = int(np.argmax(d / derived))
    print(f"h2range {fam:9s} {name:14s} worst channel {c}: |d| {d[c]:.3e} max {vmax[c]:.3e}  d/(tol max(1,ref)) {(d / (tol * np.maximum(1, vmax))).max():.3f}  d/derived {d[c] / derived[c]:.3f}")
    assert (d <= tol * np.maximum(1.0, vmax)).all(), (fam, name, c, d[c], vmax[c])
    return d, derived, c, vmax


def test_silu_channel_weight_scale(monkeypatch):
    """Kind 0 (SiLU) with per-channel weight scales, on the persistent 3x3."""
    need_gpu()
    fam = "3x3_pk"
    rng, x, w, b = _operands(fam, 500)
    f = _factors(rng, w.shape[0], -12)
    w, b = _per_out(w, f, False), b * f.astype(np.float32)
    d, derived, c, vmax = _check_silu(fam, "silu w per out", _launch(fam, x, w, b, 0, monkeypatch), x, w, b, 4e-6)
    assert (d <= derived).all(), (c, d[c], derived[c], vmax[c])


def test_stem_channel_weight_scale():
    """test_stem_conv_u8's shape with the 16 output channels 2^0 .. 2^-8 apart; its bound (2e-6 max(1, |ref|)) per channel."""
    need_gpu()
    import vti_amd
    rng = np.random.default_rng(11)
    H, W, c2 = 46, 62, 16
    x8 = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    f = _factors(rng, c2, -8).astype(np.float32)
    w = (rng.standard_normal((c2, 3, 3, 3)) / np.sqrt(27)).astype(np.float32) * f[:, None, None, None]
    b = rng.standard_normal(c2).astype(np.float32) * 0.1 * f
    out, _, _ = vti_amd.debug_conv2d(torch.from_numpy(x8).cuda(), w, b, 3, 2, 0, "h2", c1=3)
    torch.cuda.synchronize()
    x = x8.astype(np.float32) / np.float32(255)
    d, derived, c, vmax = _check_silu("stem", "w per out", out.cpu(), x, w, b, 2e-6, k_s=(3, 2))
    assert (d <= derived).all(), (c, d[c], derived[c], vmax[c])


# ---- saturation: ordinary finite numbers whose results leave +-4094

def _straddling(fam, seed):
    """About half the outputs past the limit, both signs; every other output channel 16 times larger still (past 65504)."""
    rng, x, w, b = _operands(fam, seed, gain=6000.0 / 16)
    x = x * np.float32(16)
    f = np.where(np.arange(w.shape[0]) % 2, 16.0, 1.0)
    return rng, x, _per_out(w, f, False), b


@pytest.mark.parametrize("fam", ["1x1_pk", "3x3_pk"])
def test_outputs_past_the_limit_saturate(fam, monkeypatch):
    need_gpu()
    _, x, w, b = _straddling(fam, 600)
    _check(fam, "saturate", _launch(fam, x, w, b, 1, monkeypatch), x, w, b, 1, saturating=True)


@pytest.mark.parametrize("fam", ["3x3_pk", "3x3_tile"])
def test_residual_sum_past_the_limit_saturates(fam, monkeypatch):
    """conv outputs of standard deviation 1500 (in range) plus a stored residual of +-3000: the SUM leaves the range."""
    need_gpu()
    rng, x, w, b = _operands(fam, 700, gain=1500.0 / 16)
    x = x * np.float32(16)
    Ho, Wo = h2_ref.out_hw(x.shape[1], x.shape[2], 3, 1, 1)
    res = (rng.choice([-3000.0, 3000.0], (B, Ho, Wo, w.shape[0])) + rng.standard_normal((B, Ho, Wo, w.shape[0]))).astype(np.float32)
    import vti_amd
    out = _launch(fam, x, w, b, 1, monkeypatch, res=res)
    raw = h2_ref.conv_scheme(x, w, b, 3, 1, 1, res=res, act=False)
    conv = h2_ref.conv_scheme(x, w, b, 3, 1, 1, act=False)
    assert np.abs(conv).max() < 4094 * 2 and (np.abs(conv) < 4094).mean() > 0.95 and (np.abs(raw) > 4095).mean() > 0.2
    got = vti_amd.h2_decode(out).double().numpy()
    assert np.isfinite(got).all()
    want = np.clip(raw, -4094, 4094)
    d = np.abs(got - want).max((0, 1, 2))
    bound = CAP * _e32(fam, x, w, b, res) + h2_ref.unit(np.abs(want).max((0, 1, 2)))
    assert (d <= bound).all(), (d / bound).max()
    past = np.abs(raw) > 4095
    assert np.array_equal(got[past], np.sign(raw[past]) * 4094.0)


@pytest.mark.parametrize("fam", ["1x1_pk", "3x3_pk"])
def test_silu_outputs_past_the_limit_saturate(fam, monkeypatch):
    """Kind 0: SiLU(+-6000) is 6000 and -0; the positive half saturates, nothing is NaN."""
    need_gpu()
    import vti_amd
    _, x, w, b = _straddling(fam, 800)
    k, s = FAMILIES[fam][:2]
    out = _launch(fam, x, w, b, 0, monkeypatch)
    got = vti_amd.h2_decode(out).double().numpy()
    assert np.isfinite(got).all()
    with np.errstate(over="ignore"):
        raw = h2_ref.conv_scheme(x, w, b, k, s, 0)
    want = np.clip(raw, -4094, 4094)
    vmax = np.abs(want).max((0, 1, 2))
    # the file's h2 bound with SiLU at the (clipped) channel maximum, plus what the fp32 accumulation of pre-activations up to
    # 5e5 leaves on an output that is still in range (|silu'| <= 1.1)
    d, bound = np.abs(got - want).max((0, 1, 2)), 1.1 * CAP * _e32(fam, x, w, b) + 4e-6 * np.maximum(1.0, vmax)
    assert (d <= bound).all(), (d / bound).max()
    past = raw > 4095
    assert past.mean() > 0.2 and (got[past] == 4094.0).all()


def test_forward_with_a_saturating_conv(monkeypatch):
    """The n-scale forward (320x320, the smallest canvas whose default plan has every kernel family of the 640x640 plan) on the
    seeded blob with model.4.cv1's weights and bias times 2^12: its SiLU outputs pass 4094 on these frames.  Unclamped, the NaN
    pairs reach the scores and NMS drops them silently; clamped, pred and proto are finite, everything upstream is bit-identical
    to the unmodified blob's and the scaled conv's output is the oracle's, clipped, under the usual per-layer bound."""
    need_gpu()
    import vti_amd
    from gpu_util import LAYER_TOL, frames_u8, plan_env, plan_families
    from oracle.model import OracleModel
    H = W = 320
    name = "model.4.cv1"
    plan_env(monkeypatch, {})
    engs = [vti_amd.Engine("n", 80, H=H, W=W, max_batch=B, dtype="h2") for _ in range(2)]
    table = engs[0].conv_table()
    assert plan_families(table) >= plan_families(vti_amd.Engine("n", 80, H=640, W=640, max_batch=B, dtype="h2").conv_table())
    blob = vti_amd.random_weights(engs[0], seed=1, gain=1.7)
    meta, _, tensors = vti_amd.unpack_container(blob)
    tensors = dict(tensors)
    tensors[name] = tuple(a * np.float32(2.0 ** 12) for a in tensors[name])
    big = vti_amd.pack_container(meta["scale"], meta["nc"], meta["nm"], meta["reg_max"], table, tensors)
    fr = frames_u8(B, H, W, seed=3)
    om = OracleModel(big, H, W, mode="fp32")
    om.forward_u8(fr, swap_rb=True, record=True)
    want = om.taps[name]
    assert (want > 4095).float().mean() > 0.02 and torch.isfinite(want).all()      # chosen on the oracle: 5 % of its outputs leave the range
    engs[0].load_weights(blob, 0)
    engs[1].load_weights(big, 0)
    x = torch.from_numpy(fr).cuda()
    idx = [t["name"] for t in table].index(name)
    upstream = {}
    for e, eng in enumerate(engs):
        pred, proto = eng.forward(x, swap_rb=True)
        torch.cuda.synchronize()
        for i in range(idx):
            try:
                t = eng.debug_conv_output(i, B).cpu()
            except vti_amd.VtiError:
                continue        # a row that lives in its consumer's kernel (check_conv_rows names which may)
            upstream.setdefault(i, []).append(t)
    assert torch.isfinite(pred).all() and torch.isfinite(proto.float()).all(), (torch.isfinite(pred).float().mean(), torch.isfinite(proto.float()).float().mean())
    assert len(upstream) >= 3 and all(len(v) == 2 and torch.equal(*v) for v in upstream.values())
    got = engs[1].debug_conv_output(idx, B).cpu()
    want = want.clamp(-4094, 4094)
    assert torch.isfinite(got).all() and (got - want).abs().max() <= LAYER_TOL["h2"] * 4094
    assert (got[om.taps[name] > 4095] == 4094).all()


@pytest.mark.parametrize("fam", ["1x1_pk", "3x3_pk"])
def test_inputs_at_the_limit(fam, monkeypatch):
    """x = +-4094 (hi = +-65504, lo = 0) everywhere: finite, and the scheme's result."""
    need_gpu()
    rng, x, w, b = _operands(fam, 900, gain=0.02)
    x = rng.choice([-4094.0, 4094.0], x.shape).astype(np.float32)
    _check(fam, "x at limit", _launch(fam, x, w, b, 1, monkeypatch), x, w, b, 1)
