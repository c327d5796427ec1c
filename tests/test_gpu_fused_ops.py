"""The conv kernels the planner fuses, ONE op at a time on operands the test writes (vti_debug_set_conv_output, vti_debug_run_op),
per output channel against tests/fused_ref.py: stem_l1_kernel (stem + layer 1 + model.2.cv1), bneck_pk (the Bottleneck pair, and
the pair with the C2f's closing 1x1 as its tail), conv_stage2 on the head towers with its raw, sigmoid + best-pair and DFL +
dist2bbox epilogues into pred, convfold_kernel (ConvTranspose folded into proto.cv2, + cv3) and conv1_pk reading half of its
input as a nearest-2x upsample.  n scale, nc 80, canvas 224x352 (maps 56x88, 28x44, 14x22, 7x11: every tile is clipped).

Procedure of every case: the seeded blob with the op's own convs replaced; every input view of the op written for all B frames
and READ BACK (the reference starts from what the kernel holds); pred, proto and best filled with a byte pattern; the op run
once; its outputs read; compared per output channel.

The bound, per output channel (the construction of test_gpu_h2_range.py / test_gpu_h2_wide.py, no new constant).  With
R = max |fused_ref(acc=float32) - fused_ref(float64)| over the channel (both round every intermediate to storage, so a
half-unit flip of an intermediate is inside R) a kernel must satisfy
    |got - fused_ref(float64)| <= CAP R + S + one storage unit at the channel's maximum,     CAP = 3,
S = the SiLU term of test_gpu_h2_range._silu_bound, (6 + 1.5 max|pre|) 2^-24 max|silu(pre)|, of every SiLU stage.  The term of
the LAST stage is per output channel as it stands (and CAP R passes through that SiLU with |silu'| <= 1.1, as _silu_bound
has it).  The term of an EARLIER stage is per channel of an intermediate; it reaches output channel o through the next conv as
at most sum_c (sum_taps |w[o, c, tap]|) term[c] (the triangle inequality), times 1.1 for every SiLU it then passes.  That is all
`_chain` does, with one term more that the first run on an MI355X showed the issue's bound to lack (fp16 towers: |d| up to 8 R
where R held only the few roundings that flip between the float32 and the float64 evaluation): an intermediate is ROUNDED to
storage, and two values a, b that differ by the slack above round to q(a), q(b) with |q(a) - q(b)| <= |a - b| + one storage
unit (each rounding moves its value by at most half a unit).  The kernel's fast SiLU puts its intermediates a few 2^-24 away
from the reference's, which flips far more roundings than the float32 accumulation alone does.  So every rounded intermediate
adds one storage unit at its channel's maximum to its own slack, and that is carried on like the SiLU term.  It is a worst
case (every intermediate flips against the sign of its weight): in fp16 it dominates the towers' and the pairs' bounds.
Further terms, each from the kernel's arithmetic:
  * scores: |sigmoid'| <= 1/4 on the logit's bound, plus the fast sigmoid's own (6 + 1.5 max|logit|) 2^-24 max(score) -- the same
    exp2 / rcp pair as the fast SiLU -- plus one fp32 unit.  The (max, first class) pair must be EXACTLY the pair of the row the
    kernel stored (what nms derives from the stored row), and is not compared with the reference's.
  * DFL boxes: misc_ref's bound of an fp32 decode, on top of the logits' bound delta_k carried through the expectation to first
    order: |d(d)| <= sum_k p_k |k - d| delta_k per side (d(sum k p_k)/dv_k = p_k (k - d)), then (l + r) / 2 and l + r times the stride.
  * the fold (convfold_kernel).  fused_ref.proto_fold is the three convs; the kernel composes ConvTranspose and 3x3 on the host
    (pack_conv_fold: in double, rounded to the storage type ONCE) and never forms U.  So the reference rounds U to storage and
    the kernel does not: cv2's pre-activation moves by at most  A[m'] = sum_{m,tap} |wv[m',m,tap]| hu(max|U_m|)  (hu: half a storage
    unit); and the reference holds q(wu), q(wv) where the kernel holds rnd(Weff(wu, wv)): with S[m',c] = sum_{m,tap} |wv[m',m,tap]|
    max_rq |wu[c,m,r,q]| >= the sum over the four window taps of |Weff|,
        W[m'] = sum_c max|P_c| (rel S[m',c] + sum_{m,tap} (|dwv| max|wu| + |wv| max|dwu| + |dwv| max|dwu|)),
    rel = 2^-11 (fp16), 2^-22 (h2), 2^-24 (fp32: the composed weights are rounded to float32), dw = q(w) - w.  A + W is added to
    cv2's pre-activation slack and carried on like a SiLU term.  In fp16 it dominates the fold's bound (the rounding of U).
Nobody had measured these kernels in isolation; RATIOS below holds, per family, the largest (|d| - unit) / R that a run on an
MI355X printed (each case prints its own line, `fusedops ...`), i.e. what CAP applies to before S.

Which plan rows are exercised (224x352, default switches unless stated; "--" = the dtype's plan does not produce the family):
  family        convs                                                    h2            fp16          fp32
  stem          model.0 + model.1 + model.2.cv1                          8x40          8x40          8x40
  pair_tail     model.2.m.0.cv1 + .cv2 + model.2.cv2                     8x20 / 16x20  8x20 / 16x20  --  (the fp32 plan keeps model.2.cv2 apart)
  pair          model.2.m.0 (fp32), model.4.m.0, model.15.m.0 (fp16)     --            8x20 / 16x20  8x20 / 16x20  (h2: model.4's pairs are not fused)
  tower_box     model.22.cv2.L.1 + .2 -> DFL boxes in pred (fp32: raw)   16x20 pk, 7x11  14x22, 7x11   14x22 raw   (DFL is not fused in fp32)
  tower_cls     model.22.cv3.L.1 + .2 -> scores + best in pred           14x22, 7x11   same          same
  tower_mc      model.22.cv4.L.1 + .2 -> raw in pred                     14x22, 7x11   same          same
  fold          proto.upsample + proto.cv2 + proto.cv3                   8x20          4x20 pk       4x20
  upcat         model.12.cv1, model.15.cv1 (VTI_PK1_ALL=1)               2x80 pk       2x80 pk       2x80 pk
(16x20: the max_batch = 64 engine, on which B = 3 is run.)

Sensitivity (once, on scratch builds of value-only mutations; none is committed): see SENSITIVITY below.
"""
import functools

import numpy as np
import pytest
import torch

import fused_ref
import h2_ref
from gpu_util import need_gpu, plan_env
from test_gpu_h2_range import CAP, _factors, _silu_bound

pytestmark = pytest.mark.gpu

NC, HW, MAXB = 80, (224, 352), 3
PATTERN = 0xFF       # every byte 0xFF: a NaN in fp16 and in float32, which no written output may be (a finite pattern can equal a real fp16 output)
LEVELS = {0: (28, 44, 8), 1: (14, 22, 16), 2: (7, 11, 32)}
A0 = {0: 0, 1: 28 * 44, 2: 28 * 44 + 14 * 22}
NA = 28 * 44 + 14 * 22 + 7 * 11
NO = 4 + NC + 32
DTYPES = ["h2", "fp16", "fp32"]

# Largest (|d| - unit) / R per (family, dtype) over all its cases on an MI355X, and the case that gave it.  Where it is above CAP the
# case is carried by a derived term, not by CAP R: fp16 towers by the rounding flips of the intermediate (R holds few), the fp16
# fold by the rounding of U that the kernel does not do (a constant input makes R tiny there), the h2 scores of channels 2^-12
# down by the fast sigmoid's own error (two fp32 units against an R of 1e-9), the fp32 1x1 over K = 384 by the SiLU term.  0.00:
# the difference never left the storage unit.  The largest |d| / bound of the whole file was 0.65 (upcat fp32 natural).
RATIOS = {
    ("stem", "h2"): (0.90, "natural"), ("stem", "fp16"): (0.00, "natural"), ("stem", "fp32"): (1.19, "natural"),
    ("pair_tail", "h2"): (0.67, "act 2^-12"), ("pair_tail", "fp16"): (0.00, "natural"),
    ("pair", "fp16"): (0.00, "natural"), ("pair", "fp32"): (1.20, "natural"),
    ("tower_box", "h2"): (0.00, "natural"), ("tower_box", "fp16"): (2.75, "natural"), ("tower_box", "fp32"): (2.67, "natural"),
    ("tower_cls", "h2"): (79.94, "factors 1"), ("tower_cls", "fp16"): (8.07, "natural"), ("tower_cls", "fp32"): (3.56, "natural"),
    ("tower_mc", "h2"): (1.98, "act 2^-12"), ("tower_mc", "fp16"): (7.94, "factors in1"), ("tower_mc", "fp32"): (2.00, "natural"),
    ("fold", "h2"): (2.08, "factors 1"), ("fold", "fp16"): (8710.81, "bias classes"), ("fold", "fp32"): (1.49, "natural"),
    ("upcat", "h2"): (2.37, "natural"), ("upcat", "fp16"): (0.00, "natural"), ("upcat", "fp32"): (5.99, "natural"),
}
# The five value-only mutations of the issue, each built once on a scratch copy and run against this file: which test caught it
# and by what factor over the bound (|d| / bound of the worst channel).
SENSITIVITY = {
    "1 interior bias class on the fold's right border": ("test_fold_bias_classes (all three dtypes), and the fold's natural, activation-scale, factor and saturating cases", 38915, "fold fp32 bias classes; h2 11493"),
    "2 h2 stage 2 fed the hi half of the intermediate": ("test_tower_natural / _activation_scale / _channel_factors / _on_the_wide_batch_engine (h2, all three epilogues), test_fold_* (h2)", 99, "tower_mc L0 h2 factors 0"),
    "3 tail without its Wb . y2 step": ("test_pair_natural / _activation_scale / _channel_factors / _shortcut / _saturating_intermediate (model.2, h2 and fp16)", 60161, "pair_tail h2 factors 1"),
    "4 shortcut added ahead of the second SiLU": ("test_pair_shortcut, _natural, _activation_scale, _channel_factors, _zero_weights, _saturating_intermediate (every dtype with a shortcut)", 2172393, "pair model.2 fp32 shortcut 2^6"),
    "5 alpha2 replaced by alpha in the pair's second epilogue": ("test_pair_activation_scale (h2: the two convs' weight scales differ), _channel_factors, _natural, _saturating_intermediate", 75343, "pair_tail h2 act 2^-4; 9.8e6 at 2^-12"),
}


# ---- engines, weights --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _engine(dtype, max_batch, pk1):
    import vti_amd
    return vti_amd.Engine("n", NC, H=HW[0], W=HW[1], max_batch=max_batch, dtype=dtype)


def engine(monkeypatch, dtype, max_batch=MAXB, pk1=False):
    """Cached per (dtype, switches); the switches are read when the engine is created."""
    plan_env(monkeypatch, {"VTI_PK1_ALL": "1"} if pk1 else {})
    return _engine(dtype, max_batch, pk1)


@functools.lru_cache(maxsize=None)
def base():
    import vti_amd
    plan = vti_amd.Engine("n", NC, H=HW[0], W=HW[1], max_batch=1)
    meta, table, tensors = vti_amd.unpack_container(vti_amd.random_weights(plan, seed=1, gain=1.7))
    return meta, plan.conv_table(), tensors


def load(eng, ws):
    import vti_amd
    meta, table, tensors = base()
    t = dict(tensors)
    t.update(ws)
    eng.load_weights(vti_amd.pack_container(meta["scale"], meta["nc"], meta["nm"], meta["reg_max"], table, t), 0)


def he(rng, shape, gain=1.7, deconv=False):
    fan = shape[0] if deconv else shape[1] * shape[2] * shape[3]
    return (rng.standard_normal(shape) * gain / np.sqrt(fan)).astype(np.float32)


def bias(rng, n, s=0.1):
    return (rng.standard_normal(n) * s).astype(np.float32)


# ---- bounds ------------------------------------------------------------------------------------------------------------------
def _cl(t):
    return t.permute(0, 2, 3, 1).numpy()


def _cmax(t):
    return t.abs().amax((0, 2, 3)).numpy()


def unit(kind, vmax):
    """One unit in the last place of the storage `kind` at magnitude vmax (array)."""
    vmax = np.asarray(vmax, np.float64)
    if kind == "h2":
        return h2_ref.unit(vmax)
    bits, emin = (10, -14) if kind == "fp16" else (23, -126)
    return 2.0 ** (np.floor(np.log2(np.maximum(vmax, 2.0 ** emin))) - bits)


def silu_term(pre):
    """The SiLU term of _silu_bound alone, per channel."""
    return _silu_bound(_cl(pre), _cl(fused_ref.silu(pre)), 0.0, 0.0)


def _l1(w):
    return np.abs(np.asarray(w, np.float64)).sum((2, 3))


def _chain(stages, dtype, extra=None):
    """stages: [(w OIHW as held or None for the first, pre, act)] in execution order -> the slack of the LAST stage's
    pre-activation that the earlier stages' SiLU terms and roundings (and `extra`: {stage index: slack added to that stage's
    pre-activation}) leave, per output channel.  Every stage but the last is rounded to the storage `dtype`."""
    slack = None
    for i, (w, pre, act) in enumerate(stages):
        pre_slack = np.zeros(pre.shape[1]) if slack is None or w is None else _l1(w) @ slack
        if extra and i in extra:
            pre_slack = pre_slack + extra[i]
        if i == len(stages) - 1:
            return pre_slack
        post = fused_ref.silu(pre) if act else pre
        slack = (1.1 * pre_slack + silu_term(pre) if act else pre_slack) + unit(dtype, _cmax(post))


def check(tag, got, ref64, ref32, pre, act, kind, pre_slack=None, saturating=False, quiet=False):
    """got / ref [B,C,h,w]; pre: the last stage's pre-activation (float64 reference); act: whether a SiLU follows it; kind: the
    output's storage.  -> (ratio, worst d / bound)."""
    got = got.double()
    assert torch.isfinite(ref64).all() and torch.isfinite(ref32).all(), tag
    assert torch.isfinite(got).all(), f"{tag}: {int((~torch.isfinite(got)).sum())} non-finite outputs"
    assert saturating or ref64.abs().max() <= 4094, tag
    R = _cmax(ref32 - ref64)
    vmax = _cmax(ref64)
    u = unit(kind, vmax)
    bound = _silu_bound(_cl(pre), _cl(ref64), R, u) if act else CAP * R + u
    if pre_slack is not None:
        bound = bound + (1.1 if act else 1.0) * pre_slack
    d = _cmax(got - ref64)
    c = int(np.argmax(d / bound))
    ratio = float((np.maximum(d - u, 0)[R > 0] / R[R > 0]).max()) if (R > 0).any() else 0.0
    if not quiet:
        print(f"fusedops {tag:44s} (d-unit)/R {ratio:7.3f}  worst channel {c}: |d| {d[c]:.3e} R {R[c]:.3e} unit {u[c]:.3e} max {vmax[c]:.3e} d/bound {d[c] / bound[c]:.3f}")
    assert (d <= bound).all(), f"{tag}: channel {c}: |got - ref| {d[c]:.3e} > bound {bound[c]:.3e} (R {R[c]:.3e}, unit {u[c]:.3e}, channel max {vmax[c]:.3e})"
    return ratio, float(d[c] / bound[c])


# ---- one op --------------------------------------------------------------------------------------------------------------------
class Op:
    """The op that computes conv `name` on an engine whose weights are loaded: write inputs, run, read."""

    def __init__(self, eng, name):
        self.eng, self.table = eng, eng.conv_table()
        self.names = [t["name"] for t in self.table]
        self.i = self.names.index(name)

    def idx(self, name):
        return self.names.index(name)

    def set(self, name, x):
        """x float32 [B,C,h,w] -> conv `name`'s output view; -> what the view then holds (float64, on the host)."""
        self.eng.debug_set_conv_output(self.idx(name), torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda())
        return self.get(name, x.shape[0])

    def get(self, name, B):
        out = self.eng.debug_conv_output(self.idx(name), B)
        torch.cuda.synchronize()
        return out.cpu().double()

    def run(self, B, x=None, swap=False):
        dev = self.eng.device
        fill = lambda *s: torch.full(s, PATTERN, dtype=torch.uint8, device=dev)
        self.pred = fill(B, NA, NO * 4).view(torch.float32)
        self.best = fill(B, NA, 2 * 4).view(torch.float32)
        self.proto = fill(B, HW[0] // 4, HW[1] // 4, 32 * (2 if self.eng.dtype == "fp16" else 4)).view(self.eng.torch_dtype)
        convs = self.eng.debug_run_op(self.i, B, x=x, swap_rb=swap, pred=self.pred, proto=self.proto, best=self.best)
        torch.cuda.synchronize()
        return [self.names[c] for c in convs]

    def rows(self, *names):
        return [self.table[self.idx(n)] for n in names]


def pattern_left(t):
    """bool, per element: still the byte pattern."""
    return (t.contiguous().view(torch.uint8) == PATTERN).view(*t.shape, -1).all(-1).cpu()


def hooks(dtype):
    return fused_ref.hooks(dtype)


def both(fn, *args, **kw):
    """-> ((out64, aux64), (out32, aux32))"""
    return fn(*args, acc=torch.float64, **kw), fn(*args, acc=torch.float32, **kw)


def record(fam, dtype, case, ratio):
    print(f"fusedops-ratio {fam} {dtype} {case} {ratio:.3f}")


# ---- stem ----------------------------------------------------------------------------------------------------------------------
STEM = ("model.0", "model.1", "model.2.cv1")


def stem_case(monkeypatch, dtype, B, ws, frames, case, swap=True):
    eng = engine(monkeypatch, dtype)
    load(eng, ws)
    op = Op(eng, "model.1")
    t0, t1, t2 = op.rows(*STEM)
    assert t1["fused"] and t2["fused"] and t1["tile"] == (8, 40) and not t0["persistent"]
    assert op.run(B, x=torch.from_numpy(frames).cuda(), swap=swap) == list(STEM)
    got = op.get("model.2.cv1", B)
    q_act, q_w = hooks(dtype)
    kw = {}
    if dtype == "h2":       # bytes as exact integers, the 1 / 255 inside the stem's weights (pack_stem_toeplitz)
        kw = dict(q_in=lambda x: x.double() / 255,
                  q_w0=lambda w: q_w((np.asarray(w, np.float64) / 255.0).astype(np.float32)) * 255.0)
    (o64, a64), (o32, _) = both(fused_ref.stem_l1, frames, swap, *ws[STEM[0]], *ws[STEM[1]], *ws[STEM[2]], q_act, q_w, **kw)
    w1, w2 = q_w(ws[STEM[1]][0]).numpy(), q_w(ws[STEM[2]][0]).numpy()
    p0, p1, p2 = a64["pre"]
    slack = _chain([(None, p0, True), (w1, p1, True), (w2, p2, True)], dtype)
    r, _ = check(f"stem {dtype} {case} B={B}", got, o64, o32, p2, True, dtype, slack)
    record("stem", dtype, case, r)
    assert pattern_left(op.pred).all() and pattern_left(op.best).all() and pattern_left(op.proto).all()


def stem_weights(rng, gain=1.7):
    return {STEM[0]: (he(rng, (16, 3, 3, 3), gain), bias(rng, 16)), STEM[1]: (he(rng, (32, 16, 3, 3), gain), bias(rng, 32)),
            STEM[2]: (he(rng, (32, 32, 1, 1), gain), bias(rng, 32))}


def frames_of(rng, B):
    return rng.integers(0, 256, (B, HW[0], HW[1], 3), dtype=np.uint8)


@pytest.mark.parametrize("B", [3, 1])
@pytest.mark.parametrize("dtype", DTYPES)
def test_stem_natural(dtype, B, monkeypatch):
    need_gpu()
    rng = np.random.default_rng(10)
    stem_case(monkeypatch, dtype, B, stem_weights(rng), frames_of(rng, B), "natural", swap=B == 3)


@pytest.mark.parametrize("which", [0, 1, 2, "in1"])
@pytest.mark.parametrize("dtype", ["h2", "fp16"])
def test_stem_channel_factors(dtype, which, monkeypatch):
    """Output channels of one conv of the op 2^0 .. 2^-12 (h2) / 2^-6 (fp16) apart, or layer 1's input channels; the biases of
    the stages before the last stay unscaled (mids far below their channel's weights' scale)."""
    need_gpu()
    rng = np.random.default_rng(11)
    ws = stem_weights(rng)
    ws = factors(rng, ws, STEM, which, dtype)
    stem_case(monkeypatch, dtype, 3, ws, frames_of(rng, 3), f"factors {which}")


def factors(rng, ws, names, which, dtype):
    lo = -12 if dtype == "h2" else -6
    ws = dict(ws)
    if which == "in1":
        w, b = ws[names[1]]
        ws[names[1]] = (w * _factors(rng, w.shape[1], lo).astype(np.float32)[None, :, None, None], b)
    else:
        w, b = ws[names[which]]
        f = _factors(rng, w.shape[0], lo).astype(np.float32)
        ws[names[which]] = (w * f[:, None, None, None], b * f if which == len(names) - 1 else b)
    return ws


@pytest.mark.parametrize("dtype", DTYPES)
def test_stem_zero_weights(dtype, monkeypatch):
    """All weights zero: the output is the bias chain alone (the Toeplitz pack of zeros, alpha of an all-zero conv)."""
    need_gpu()
    rng = np.random.default_rng(12)
    ws = {n: (np.zeros_like(w), bias(rng, b.size, 1.0)) for n, (w, b) in stem_weights(rng).items()}
    stem_case(monkeypatch, dtype, 3, ws, frames_of(rng, 3), "zero weights")


# ---- the Bottleneck pair, with and without the tail --------------------------------------------------------------------------------
def pair_case(monkeypatch, dtype, B, block, ws, x, case, max_batch=MAXB, saturating=False):
    """block: "model.2" (tail in h2 / fp16, plain pair in fp32), "model.4" or "model.15" (fp16 pairs).  x: float32 [B, 2c, h, w],
    the block's cv1 output (y0 | y1)."""
    eng = engine(monkeypatch, dtype, max_batch)
    load(eng, ws)
    n1, n2, nt, nin = f"{block}.m.0.cv1", f"{block}.m.0.cv2", f"{block}.cv2", f"{block}.cv1"
    tail = block == "model.2" and dtype != "fp32"
    op = Op(eng, n2)
    t1, t2, tt = op.rows(n1, n2, nt)
    tile = (16, 20) if max_batch == 64 else (8, 20)
    assert t1["persistent"] and t2["fused"] and t2["persistent"] and t1["tile"] == tile and (tt["fused"] and tt["tile"] == tile) == tail, (t1, t2, tt)
    held = op.set(nin, x)
    assert op.run(B) == [n1, n2] + ([nt] if tail else [])
    assert torch.equal(op.get(nin, B), held), "the op's input (y0 | y1 of the shared buffer) changed"
    got = op.get(nt if tail else n2, B)
    q_act, q_w = hooks(dtype)
    y0, y1 = held.chunk(2, 1)
    shortcut = block != "model.15"
    args = (y1, *ws[n1], *ws[n2], shortcut, q_act, q_w)
    kw = dict(tail=(y0, *ws[nt])) if tail else {}
    (o64, a64), (o32, _) = both(fused_ref.bneck, *args, **kw)
    p = a64["pre"]
    stages = [(None, p[0], True), (q_w(ws[n2][0]).numpy(), p[1], True)]
    if tail:
        c = y1.shape[1]
        wt = q_w(ws[nt][0]).numpy()[:, 2 * c:]          # only y2's columns carry slack: y0 and y1 are exact
        stages.append((wt, p[2], True))
    slack = _chain(stages, dtype)
    r, _ = check(f"{'pair_tail' if tail else 'pair'} {block} {dtype} {case} B={B} tile={tile}", got, o64, o32, p[-1], True, dtype, slack, saturating)
    record("pair_tail" if tail else "pair", dtype, case, r)
    assert pattern_left(op.pred).all() and pattern_left(op.best).all() and pattern_left(op.proto).all()
    return a64


PAIR_SHAPES = {"model.2": (16, 56, 88), "model.4": (32, 28, 44), "model.15": (32, 28, 44)}
PAIRS = [(d, "model.2") for d in DTYPES] + [("fp16", "model.4"), ("fp16", "model.15")]      # h2: model.4's / model.15's pairs are not fused


def pair_weights(rng, block, gain=1.7):
    c = PAIR_SHAPES[block][0]
    nt_in = {"model.2": 3 * c, "model.4": 4 * c, "model.15": 3 * c}[block]
    return {f"{block}.m.0.cv1": (he(rng, (c, c, 3, 3), gain), bias(rng, c)), f"{block}.m.0.cv2": (he(rng, (c, c, 3, 3), gain), bias(rng, c)),
            f"{block}.cv2": (he(rng, (2 * c, nt_in, 1, 1), gain), bias(rng, 2 * c))}


def pair_names(block):
    return (f"{block}.m.0.cv1", f"{block}.m.0.cv2", f"{block}.cv2")


def pair_input(rng, block, B):
    c, h, w = PAIR_SHAPES[block]
    return rng.standard_normal((B, 2 * c, h, w)).astype(np.float32)


@pytest.mark.parametrize("B,max_batch", [(3, MAXB), (1, MAXB), (3, 64)])
@pytest.mark.parametrize("dtype,block", PAIRS)
def test_pair_natural(dtype, block, B, max_batch, monkeypatch):
    """N(0, 1) inputs, He weights; max_batch = 64 plans the 16x20 tile.  model.15.m.0 is the pair without a shortcut."""
    need_gpu()
    rng = np.random.default_rng(20)
    pair_case(monkeypatch, dtype, B, block, pair_weights(rng, block), pair_input(rng, block, B), "natural", max_batch)


@pytest.mark.parametrize("e", [-12, -4, 4])
@pytest.mark.parametrize("dtype,block", [p for p in PAIRS if p[0] != "fp32"])
def test_pair_activation_scale(dtype, block, e, monkeypatch):
    """Inputs times 2^e, the first conv's weights times 2^-e: the intermediate keeps its size.  With the shortcut (and y0, y1 in the
    tail) the input's own scale reaches the output as it is."""
    need_gpu()
    rng = np.random.default_rng(21)
    ws = pair_weights(rng, block)
    n1 = pair_names(block)[0]
    ws[n1] = (ws[n1][0] * np.float32(2.0 ** -e), ws[n1][1])
    pair_case(monkeypatch, dtype, 3, block, ws, pair_input(rng, block, 3) * np.float32(2.0 ** e), f"act 2^{e}")


# model.4's op has no tail (the block's closing 1x1 is another op): no factors on a third conv there
@pytest.mark.parametrize("dtype,block,which", [(d, b, wh) for d, b in (("h2", "model.2"), ("fp16", "model.2"), ("fp16", "model.4"))
                                               for wh in (0, 1, 2, "in1") if wh != 2 or b == "model.2"])
def test_pair_channel_factors(dtype, block, which, monkeypatch):
    need_gpu()
    rng = np.random.default_rng(22)
    ws = factors(rng, pair_weights(rng, block), pair_names(block)[:3 if block == "model.2" else 2], which, dtype)
    pair_case(monkeypatch, dtype, 3, block, ws, pair_input(rng, block, 3), f"factors {which}")


@pytest.mark.parametrize("dtype,block", PAIRS)
def test_pair_zero_weights(dtype, block, monkeypatch):
    """Zero weights, biases of scale 1: the bias chain (and the shortcut; in the tail the three-part sum is its bias alone)."""
    need_gpu()
    rng = np.random.default_rng(23)
    ws = {n: (np.zeros_like(w), bias(rng, b.size, 1.0)) for n, (w, b) in pair_weights(rng, block).items()}
    pair_case(monkeypatch, dtype, 3, block, ws, pair_input(rng, block, 3), "zero weights")


@pytest.mark.parametrize("dtype,block", PAIRS)
def test_pair_shortcut(dtype, block, monkeypatch):
    """x of magnitude 2^6, different in every pixel and channel, against a conv result below 1 (the second conv's gain 2^-6): a
    shortcut taken from a neighbouring pixel or channel, or added ahead of the SiLU, cannot hide.  model.15.m.0 has none: there
    the same operands must NOT show x in the output."""
    need_gpu()
    rng = np.random.default_rng(24)
    ws = pair_weights(rng, block)
    n1, n2 = pair_names(block)[:2]
    ws[n1] = (ws[n1][0] * np.float32(2.0 ** -6), ws[n1][1])
    ws[n2] = (ws[n2][0] * np.float32(2.0 ** -6), ws[n2][1])
    x = pair_input(rng, block, 3)
    x = (np.sign(x) * (64 + 16 * np.abs(x))).astype(np.float32)
    pair_case(monkeypatch, dtype, 3, block, ws, x, "shortcut 2^6")


def test_pair_saturating_intermediate(monkeypatch):
    """h2: first-stage weights such that about a third of the first SiLU's outputs pass 4094 (its pre-activations have a standard
    deviation of 9500); the T image must hold them clamped to +-4094 -- finite outputs, equal to the reference whose q clamps."""
    need_gpu()
    rng = np.random.default_rng(25)
    block = "model.2"
    ws = pair_weights(rng, block)
    n1, n2 = pair_names(block)[:2]
    ws[n1] = (he(rng, ws[n1][0].shape, 9500.0), ws[n1][1])
    ws[n2] = (ws[n2][0] * np.float32(2.0 ** -12), ws[n2][1])
    a = pair_case(monkeypatch, "h2", 3, block, ws, pair_input(rng, block, 3), "saturating", saturating=True)
    past = fused_ref.silu(a["pre"][0]) > 4095
    assert 0.25 < past.double().mean() < 0.45 and (a["mid"][0][past] == h2_ref.H2_MAX).all()


# ---- head towers ---------------------------------------------------------------------------------------------------------------
TOWERS = {"box": ("cv2", 64, 64, 0), "cls": ("cv3", 80, NC, 4), "mc": ("cv4", 32, 32, 4 + NC)}


def tower_weights(rng, kind, lvl, gain=1.7, gain2=1.0):
    tw, c, c2, _ = TOWERS[kind]
    return {f"model.22.{tw}.{lvl}.1": (he(rng, (c, c, 3, 3), gain), bias(rng, c)),
            f"model.22.{tw}.{lvl}.2": (he(rng, (c2, c, 1, 1), gain2), bias(rng, c2, 1.0))}


def tower_case(monkeypatch, dtype, B, kind, lvl, ws, x, case, max_batch=MAXB, saturating=False):
    tw, c, c2, cb = TOWERS[kind]
    h, w, stride = LEVELS[lvl]
    eng = engine(monkeypatch, dtype, max_batch)
    load(eng, ws)
    n0, n1, n2 = (f"model.22.{tw}.{lvl}.{j}" for j in range(3))
    op = Op(eng, n2)
    t1, t2 = op.rows(n1, n2)
    pk = dtype == "h2" and kind == "box" and lvl < 2           # the h2 box towers of the wide maps run persistently, 16x20
    assert t2["fused"] and t1["tile"] == t2["tile"] == ((16, 20) if pk else (min(h, 14), min(w, 22))) and bool(t1["persistent"]) == pk, (t1, t2)
    held = op.set(n0, x)
    assert op.run(B) == [n1, n2]
    assert torch.equal(op.get(n0, B), held)
    q_act, q_w = hooks(dtype)
    mode = {"box": "raw" if dtype == "fp32" else "dfl", "cls": "sigmoid", "mc": "raw"}[kind]
    (o64, a64), (o32, a32) = both(fused_ref.tower, held, *ws[n1], *ws[n2], mode, q_act, q_w, stride=stride)
    p1, logits = a64["pre"]
    slack = _chain([(None, p1, True), (q_w(ws[n2][0]).numpy(), logits, False)], dtype)
    tag = f"tower_{kind} L{lvl} {dtype} {case} B={B}"
    pred = op.pred.cpu()
    a0 = A0[lvl]
    inside = torch.zeros((B, NA, NO), dtype=torch.bool)
    if kind == "box" and dtype == "fp32":       # DFL is not fused in fp32: the raw logits go to the level's box buffer, pred is not touched
        got = op.get(n2, B)
        r, _ = check(tag, got, o64, o32, logits, False, "fp32", slack, saturating)
    else:
        width = 4 if kind == "box" else c2
        inside[:, a0:a0 + h * w, cb:cb + width] = True
        got = pred[:, a0:a0 + h * w, cb:cb + width].permute(0, 2, 1).reshape(B, width, h, w)
        assert not pattern_left(pred)[inside].any(), f"{tag}: part of the op's block of pred was not written"
        if kind == "mc":
            r, _ = check(tag, got, o64, o32, logits, False, "fp32", slack, saturating)
        elif kind == "cls":
            lb = CAP * _cmax(a32["logits"] - logits) + slack           # the logits' bound
            smax = _cmax(o64)
            bound = lb / 4 + (6 + 1.5 * _cmax(logits)) * 2.0 ** -24 * smax + unit("fp32", smax)
            d = _cmax(got.double() - o64)
            R = _cmax(o32 - o64)
            r = float((np.maximum(d - unit("fp32", smax), 0)[R > 0] / R[R > 0]).max()) if (R > 0).any() else 0.0
            ch = int(np.argmax(d / bound))
            print(f"fusedops {tag:44s} (d-unit)/R {r:7.3f}  worst channel {ch}: |d| {d[ch]:.3e} R {R[ch]:.3e} d/bound {d[ch] / bound[ch]:.3f}")
            assert torch.isfinite(got).all() and (d <= bound).all(), (tag, ch, d[ch], bound[ch])
            # the (max, first class) pair: exactly the pair of the row the kernel stored
            best = op.best.cpu()
            rows = pred[:, a0:a0 + h * w, cb:cb + c2]
            mx = rows.max(-1)[0]
            first = (rows == mx[..., None]).int().argmax(-1)
            assert torch.equal(best[:, a0:a0 + h * w, 0], mx) and torch.equal(best[:, a0:a0 + h * w, 1], first.float()), tag
            binside = torch.zeros((B, NA, 2), dtype=torch.bool)
            binside[:, a0:a0 + h * w] = True
            assert pattern_left(best)[~binside].all(), f"{tag}: best written outside the level's anchors"
        else:
            lb = CAP * _cmax(a32["logits"] - logits) + slack + unit("fp32", _cmax(logits))        # per logit channel (16 side + bin)
            lg = logits.permute(0, 2, 3, 1).reshape(B, h * w, 4, 16)
            pr = torch.softmax(lg, -1)
            dd = (pr * torch.arange(16.0, dtype=torch.float64)).sum(-1, keepdim=True)
            ds = (pr * (torch.arange(16.0, dtype=torch.float64) - dd).abs() * torch.from_numpy(lb).reshape(4, 16)).sum(-1)     # [B, hw, 4] bins
            ex, ey = ds[..., 0] + ds[..., 2], ds[..., 1] + ds[..., 3]
            bound = a64["dfl_bound"] + torch.stack((ex / 2, ey / 2, ex, ey), -1) * stride
            gb = pred[:, a0:a0 + h * w, :4].double()
            assert torch.isfinite(gb).all(), tag
            d = (gb - o64).abs()
            worst = (d / bound).max().item()
            R = (o32 - o64).abs().max().item()
            r = max(d.max().item() - 4 * 2.0 ** -17 * stride, 0) / R if R > 0 else 0.0
            print(f"fusedops {tag:44s} max|d| {d.max().item():.3e} px  R {R:.3e}  d/bound {worst:.3f}")
            assert (d <= bound).all(), (tag, worst)
    record(f"tower_{kind}", dtype, case, r)
    assert pattern_left(pred)[~inside].all(), f"{tag}: pred written outside [a0, a0 + h w) x the op's channel block"
    if kind != "cls":
        assert pattern_left(op.best).all(), tag
    assert pattern_left(op.proto).all(), tag
    return a64


def tower_input(rng, kind, lvl, B):
    h, w, _ = LEVELS[lvl]
    return rng.standard_normal((B, TOWERS[kind][1], h, w)).astype(np.float32)


@pytest.mark.parametrize("B,lvl", [(3, 0), (1, 0), (3, 2), (3, 1)])
@pytest.mark.parametrize("kind", list(TOWERS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_tower_natural(dtype, kind, B, lvl, monkeypatch):
    need_gpu()
    rng = np.random.default_rng(30 + lvl)
    tower_case(monkeypatch, dtype, B, kind, lvl, tower_weights(rng, kind, lvl), tower_input(rng, kind, lvl, B), "natural")


@pytest.mark.parametrize("kind", ["box", "mc"])
def test_tower_on_the_wide_batch_engine(kind, monkeypatch):
    """max_batch = 64, B = 3: the plan of the 16x20 tower tiles (h2)."""
    need_gpu()
    rng = np.random.default_rng(31)
    tower_case(monkeypatch, "h2", 3, kind, 0, tower_weights(rng, kind, 0), tower_input(rng, kind, 0, 3), "natural mb64", max_batch=64)


@pytest.mark.parametrize("e", [-12, -4, 4])
@pytest.mark.parametrize("kind", list(TOWERS))
@pytest.mark.parametrize("dtype", ["h2", "fp16"])
def test_tower_activation_scale(dtype, kind, e, monkeypatch):
    need_gpu()
    rng = np.random.default_rng(32)
    ws = tower_weights(rng, kind, 0)
    n1 = f"model.22.{TOWERS[kind][0]}.0.1"
    ws[n1] = (ws[n1][0] * np.float32(2.0 ** -e), ws[n1][1])
    tower_case(monkeypatch, dtype, 3, kind, 0, ws, tower_input(rng, kind, 0, 3) * np.float32(2.0 ** e), f"act 2^{e}")


@pytest.mark.parametrize("which", [0, 1, "in1"])
@pytest.mark.parametrize("kind", list(TOWERS))
@pytest.mark.parametrize("dtype", ["h2", "fp16"])
def test_tower_channel_factors(dtype, kind, which, monkeypatch):
    need_gpu()
    rng = np.random.default_rng(33)
    tw = TOWERS[kind][0]
    ws = factors(rng, tower_weights(rng, kind, 0), (f"model.22.{tw}.0.1", f"model.22.{tw}.0.2"), which, dtype)
    tower_case(monkeypatch, dtype, 3, kind, 0, ws, tower_input(rng, kind, 0, 3), f"factors {which}")


@pytest.mark.parametrize("kind", list(TOWERS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_tower_zero_weights(dtype, kind, monkeypatch):
    """Zero weights: the epilogues on the bias chain alone (raw: b2; scores: sigmoid(b2) and its best pair; boxes: the DFL of b2)."""
    need_gpu()
    rng = np.random.default_rng(34)
    ws = {n: (np.zeros_like(w), bias(rng, b.size, 1.0)) for n, (w, b) in tower_weights(rng, kind, 0).items()}
    tower_case(monkeypatch, dtype, 3, kind, 0, ws, tower_input(rng, kind, 0, 3), "zero weights")


@pytest.mark.parametrize("kind", list(TOWERS))
def test_tower_saturating_intermediate(kind, monkeypatch):
    need_gpu()
    rng = np.random.default_rng(35)
    ws = tower_weights(rng, kind, 0, gain=9500.0, gain2=2.0 ** -10)
    a = tower_case(monkeypatch, "h2", 3, kind, 0, ws, tower_input(rng, kind, 0, 3), "saturating", saturating=True)
    past = fused_ref.silu(a["pre"][0]) > 4095
    assert 0.25 < past.double().mean() < 0.45 and (a["mid"][0][past] == h2_ref.H2_MAX).all()


# ---- the fold ------------------------------------------------------------------------------------------------------------------
FOLD = ("model.22.proto.upsample", "model.22.proto.cv2", "model.22.proto.cv3")
REL = {"fp16": 2.0 ** -11, "h2": 2.0 ** -22, "fp32": 2.0 ** -24}


def fold_weights(rng, gain=1.7, gu=1.0, bu=0.1):
    return {FOLD[0]: (he(rng, (64, 64, 2, 2), gu, deconv=True), bias(rng, 64, bu)), FOLD[1]: (he(rng, (64, 64, 3, 3), gain), bias(rng, 64)),
            FOLD[2]: (he(rng, (32, 64, 1, 1), gain), bias(rng, 32))}


def fold_slack(dtype, ws, P, U):
    """A + W of the module docstring, per channel of cv2's pre-activation."""
    q_act, q_w = hooks(dtype)
    wu, wv = np.asarray(ws[FOLD[0]][0], np.float64), np.asarray(ws[FOLD[1]][0], np.float64)
    dwu, dwv = np.abs(q_w(ws[FOLD[0]][0]).numpy() - wu), np.abs(q_w(ws[FOLD[1]][0]).numpy() - wv)
    hu = unit(dtype, _cmax(U)) / 2                                    # [m]
    A = np.abs(q_w(ws[FOLD[1]][0]).numpy()).sum((2, 3)) @ hu
    mu, mdu = np.abs(wu).max((2, 3)), dwu.max((2, 3))                  # [c, m]
    av, adv = np.abs(wv).sum((2, 3)), dwv.sum((2, 3))                  # [m', m]
    S = av @ mu.T                                                      # [m', c]
    W = (REL[dtype] * S + adv @ mu.T + av @ mdu.T + adv @ mdu.T) @ _cmax(P)
    return A + W


def fold_case(monkeypatch, dtype, B, ws, x, case, saturating=False, regions=False):
    eng = engine(monkeypatch, dtype)
    load(eng, ws)
    op = Op(eng, FOLD[2])
    tu, tv, t3 = op.rows(*FOLD)
    assert t3["fused"] and not tu["fused"] and tu["tile"] == tv["tile"] == t3["tile"] == ((8, 20) if dtype == "h2" else (4, 20)), (tu, tv, t3)
    assert bool(tv["persistent"]) == (dtype == "fp16")
    held = op.set("model.22.proto.cv1", x)
    assert op.run(B) == list(FOLD)
    assert torch.equal(op.get("model.22.proto.cv1", B), held), "proto.cv1's output changed"
    assert not pattern_left(op.proto).any(), "part of proto was not written"
    got = op.get(FOLD[2], B)
    assert torch.equal(got, op.proto.cpu().permute(0, 3, 1, 2).double())
    q_act, q_w = hooks(dtype)
    (o64, a64), (o32, _) = both(fused_ref.proto_fold, held, *ws[FOLD[0]], *ws[FOLD[1]], *ws[FOLD[2]], q_act, q_w)
    u, p2, p3 = a64["pre"]
    slack = _chain([(None, p2, True), (q_w(ws[FOLD[2]][0]).numpy(), p3, True)], dtype, extra={0: fold_slack(dtype, ws, held, u)})
    kind = "fp32" if dtype == "h2" else dtype          # the h2 engine's proto is float32
    tag = f"fold {dtype} {case} B={B}"
    r, _ = check(tag, got, o64, o32, p3, True, kind, slack, saturating)
    record("fold", dtype, case, r)
    if regions:       # the nine border classes of the folded bias, each on its own pixels
        H, W = got.shape[2:]
        ys = {"top": slice(0, 1), "mid": slice(1, H - 1), "bottom": slice(H - 1, H)}
        xs = {"left": slice(0, 1), "mid": slice(1, W - 1), "right": slice(W - 1, W)}
        for ny, sy in ys.items():
            for nx, sx in xs.items():
                check(f"{tag} {ny}/{nx}", got[:, :, sy, sx], o64[:, :, sy, sx], o32[:, :, sy, sx], p3[:, :, sy, sx], True, kind, slack, quiet=True)
    assert pattern_left(op.pred).all() and pattern_left(op.best).all()
    return a64


def fold_input(rng, B):
    return rng.standard_normal((B, 64, 28, 44)).astype(np.float32)       # proto.cv1's output: the P3 map; proto is 56x88


@pytest.mark.parametrize("B", [3, 1])
@pytest.mark.parametrize("dtype", DTYPES)
def test_fold_natural(dtype, B, monkeypatch):
    need_gpu()
    rng = np.random.default_rng(40)
    fold_case(monkeypatch, dtype, B, fold_weights(rng), fold_input(rng, B), "natural")


@pytest.mark.parametrize("e", [-12, -4, 4])
@pytest.mark.parametrize("dtype", ["h2", "fp16"])
def test_fold_activation_scale(dtype, e, monkeypatch):
    need_gpu()
    rng = np.random.default_rng(41)
    ws = fold_weights(rng)
    ws[FOLD[0]] = (ws[FOLD[0]][0] * np.float32(2.0 ** -e), ws[FOLD[0]][1])
    fold_case(monkeypatch, dtype, 3, ws, fold_input(rng, 3) * np.float32(2.0 ** e), f"act 2^{e}")


@pytest.mark.parametrize("which", [0, 1, 2, "in1"])
@pytest.mark.parametrize("dtype", ["h2", "fp16"])
def test_fold_channel_factors(dtype, which, monkeypatch):
    need_gpu()
    rng = np.random.default_rng(42)
    ws = fold_weights(rng)
    if which == 0:          # the ConvTranspose is IOHW: its output channels are axis 1
        w, b = ws[FOLD[0]]
        ws[FOLD[0]] = (w * _factors(rng, 64, -12 if dtype == "h2" else -6).astype(np.float32)[None, :, None, None], b)
    else:
        ws = factors(rng, ws, FOLD, which, dtype)
    fold_case(monkeypatch, dtype, 3, ws, fold_input(rng, 3), f"factors {which}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_fold_zero_weights(dtype, monkeypatch):
    need_gpu()
    rng = np.random.default_rng(43)
    ws = {n: (np.zeros_like(w), bias(rng, b.size, 1.0)) for n, (w, b) in fold_weights(rng).items()}
    fold_case(monkeypatch, dtype, 3, ws, fold_input(rng, 3), "zero weights", regions=True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fold_bias_classes(dtype, monkeypatch):
    """A ConvTranspose bias of magnitude 4, a 3x3 gain of 1/4 of He's and a constant input: the folded bias carries the result and
    differs between the nine border classes (a 3x3 tap outside U loses wv . bu); corners, edges and interior are held to the
    bound separately, on the clipped right and bottom tiles too (the 28x44 low-resolution map against its 8x20 / 4x20 tiles)."""
    need_gpu()
    rng = np.random.default_rng(44)
    ws = fold_weights(rng, gain=1.7 / 4, gu=0.25)
    ws[FOLD[0]] = (ws[FOLD[0]][0], (rng.choice([-1.0, 1.0], 64) * rng.uniform(3, 5, 64)).astype(np.float32))
    x = np.broadcast_to(rng.standard_normal((1, 64, 1, 1)).astype(np.float32), (3, 64, 28, 44))
    a = fold_case(monkeypatch, dtype, 3, ws, x, "bias classes", regions=True)
    p2 = a["pre"][1]
    # the classes really differ, by far more than any bound here: interior against the first row, the last column, a corner
    for other in (p2[:, :, 0, 5], p2[:, :, 5, -1], p2[:, :, -1, -1]):
        assert (p2[:, :, 5, 5] - other).abs().max() > 0.5


def test_fold_saturating_intermediate(monkeypatch):
    """h2: cv2's SiLU outputs pass 4094 on about a third of the pixels; cv3 must see them clamped."""
    need_gpu()
    rng = np.random.default_rng(45)
    ws = fold_weights(rng, gain=1.7)
    ws[FOLD[1]] = (he(rng, (64, 64, 3, 3), 9500.0), ws[FOLD[1]][1])
    ws[FOLD[2]] = (ws[FOLD[2]][0] * np.float32(2.0 ** -10), ws[FOLD[2]][1])
    a = fold_case(monkeypatch, "h2", 3, ws, fold_input(rng, 3), "saturating", saturating=True)
    past = fused_ref.silu(a["pre"][1]) > 4095
    assert 0.25 < past.double().mean() < 0.45 and (a["mid"][1][past] == h2_ref.H2_MAX).all()


# ---- conv1_pk reading half of its input as a nearest-2x upsample (VTI_PK1_ALL=1) -------------------------------------------------------
UPCAT = {"model.12.cv1": ("model.9.cv2", 256, "model.6.cv2", 128, 128, 14, 22), "model.15.cv1": ("model.12.cv2", 128, "model.4.cv2", 64, 64, 28, 44)}


def upcat_case(monkeypatch, dtype, B, name, ws, xa, xb, case):
    na, ca, nb, cbb, c2, h, w = UPCAT[name]
    eng = engine(monkeypatch, dtype, MAXB, pk1=True)
    load(eng, ws)
    op = Op(eng, name)
    (t,) = op.rows(name)
    assert t["persistent"] and not t["fused"] and t["k"] == 1 and t["tile"] == (2, 80) and t["c1"] == ca + cbb, t
    ha, hb = op.set(na, xa), op.set(nb, xb)
    assert op.run(B) == [name]
    assert torch.equal(op.get(na, B), ha) and torch.equal(op.get(nb, B), hb), "an input of the op changed"
    got = op.get(name, B)
    q_act, q_w = hooks(dtype)
    (o64, a64), (o32, _) = both(fused_ref.up_concat_1x1, ha, hb, *ws[name], q_act, q_w)
    r, _ = check(f"upcat {name} {dtype} {case} B={B}", got, o64, o32, a64["pre"][0], True, dtype)
    record("upcat", dtype, case, r)
    assert pattern_left(op.pred).all() and pattern_left(op.best).all() and pattern_left(op.proto).all()


def upcat_operands(rng, name, B, gain=1.7):
    na, ca, nb, cbb, c2, h, w = UPCAT[name]
    ws = {name: (he(rng, (c2, ca + cbb, 1, 1), gain), bias(rng, c2))}
    return ws, rng.standard_normal((B, ca, h // 2, w // 2)).astype(np.float32), rng.standard_normal((B, cbb, h, w)).astype(np.float32)


@pytest.mark.parametrize("B", [3, 1])
@pytest.mark.parametrize("name", list(UPCAT))
@pytest.mark.parametrize("dtype", DTYPES)
def test_upcat_natural(dtype, name, B, monkeypatch):
    """The two operands are independent draws: a pixel of the upsampled half taken from the wrong source pixel shows at once."""
    need_gpu()
    rng = np.random.default_rng(50)
    ws, xa, xb = upcat_operands(rng, name, B)
    upcat_case(monkeypatch, dtype, B, name, ws, xa, xb, "natural")


@pytest.mark.parametrize("e", [-12, -4, 4])
@pytest.mark.parametrize("dtype", ["h2", "fp16"])
def test_upcat_activation_scale(dtype, e, monkeypatch):
    need_gpu()
    rng = np.random.default_rng(51)
    name = "model.12.cv1"
    ws, xa, xb = upcat_operands(rng, name, 3)
    ws[name] = (ws[name][0] * np.float32(2.0 ** -e), ws[name][1])
    upcat_case(monkeypatch, dtype, 3, name, ws, xa * np.float32(2.0 ** e), xb * np.float32(2.0 ** e), f"act 2^{e}")


@pytest.mark.parametrize("side", ["out", "in"])
@pytest.mark.parametrize("dtype", ["h2", "fp16"])
def test_upcat_channel_factors(dtype, side, monkeypatch):
    need_gpu()
    rng = np.random.default_rng(52)
    name = "model.15.cv1"
    ws, xa, xb = upcat_operands(rng, name, 3)
    w, b = ws[name]
    f = _factors(rng, w.shape[0 if side == "out" else 1], -12 if dtype == "h2" else -6).astype(np.float32)
    ws[name] = (w * f[:, None, None, None], b * f) if side == "out" else (w * f[None, :, None, None], b)
    upcat_case(monkeypatch, dtype, 3, name, ws, xa, xb, f"factors {side}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_upcat_zero_weights(dtype, monkeypatch):
    need_gpu()
    rng = np.random.default_rng(53)
    name = "model.12.cv1"
    ws, xa, xb = upcat_operands(rng, name, 3)
    ws[name] = (np.zeros_like(ws[name][0]), bias(rng, 128, 1.0))
    upcat_case(monkeypatch, dtype, 3, name, ws, xa, xb, "zero weights")


# ---- the two entry points themselves ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_set_conv_output_is_the_inverse_and_stays_in_its_slice(dtype, monkeypatch):
    """What is written is read back as the storage's own encode of it (fp16 rounding, the saturating h2 pair of h2_ref, float32
    unchanged); a view that shares its buffer with others (model.4.cv1 and model.4.m.0.cv2 in the C2f's concat buffer) leaves
    them as they were; B frames are written and no more; the refusals behind the state checks are the reader's."""
    need_gpu()
    import vti_amd
    eng = engine(monkeypatch, dtype)
    load(eng, {})
    op = Op(eng, "model.4.cv1")
    rng = np.random.default_rng(60)
    x = (rng.standard_normal((3, 64, 28, 44)) * 2.0 ** rng.integers(-14, 13, (3, 64, 28, 44))).astype(np.float32)
    x[0, 0, 0, :4] = (5000.0, -5000.0, 4094.0, 0.0)
    a = op.set("model.4.m.0.cv2", rng.standard_normal((3, 32, 28, 44)).astype(np.float32))
    held = op.set("model.4.cv1", x)
    q_act, _ = hooks(dtype)
    want = q_act(torch.from_numpy(x).double())
    assert torch.equal(held, want), (held - want).abs().max()
    if dtype == "h2":
        assert held[0, 0, 0, :4].tolist() == [4094.0, -4094.0, 4094.0, 0.0]
    assert torch.equal(op.get("model.4.m.0.cv2", 3), a), "a neighbouring slice of the buffer changed"
    b2 = op.set("model.4.cv1", x[:1] * 0 + 1)            # B = 1 writes frame 0 only
    assert torch.equal(op.get("model.4.cv1", 3)[1:], held[1:]) and (b2 == 1).all()
    L = vti_amd.lib()
    one = torch.zeros(16, device=eng.device)
    for fn in (L.vti_debug_conv_output, L.vti_debug_set_conv_output):
        assert fn(eng._ctx, 999, 1, one.data_ptr(), None) == -1 and fn(eng._ctx, -1, 1, one.data_ptr(), None) == -1
        assert fn(eng._ctx, 3, 1, None, None) == -1 and fn(eng._ctx, 3, MAXB + 1, one.data_ptr(), None) == -1
        assert fn(eng._ctx, op.idx("model.22.cv3.0.1"), 1, one.data_ptr(), None) == -6            # lives in its consumer's kernel
