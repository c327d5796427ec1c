"""The non-GEMM kernels of the forward pass (csrc/misc.hip: SPPF max-pools, nearest 2x upsample, DFL + dist2bbox + sigmoid decode),
stated once in numpy float64, with the case lists the GPU tests (test_gpu_misc_ops.py) and their CPU pin (test_misc_ref.py) share.
Takes nothing from the library and nothing from oracle/: test_misc_ref.py holds it to torch where torch has the operation, and
decode_ref to the oracle's decode.

The rule for a pooled output, the same for fp16, fp32 and h2 -- an element passes if
  (a) its decoded value equals pool_ref's (== on floats; an h2 pair decodes to hi + lo, exact in fp32 and fp64), and
  (b) its bits are the bits of some element of its window.
The rule is exact and leaves the tie-break open: +0 / -0, and h2 pairs of equal value (hi one step apart, lo of opposite signs),
have equal values and different bits, and which of them a kernel keeps is not part of the contract.

The DFL bound.  For one anchor side with logits v_0..v_15, p = softmax(v) and d = sum k p_k in float64,
    E = 30 * sum_k p_k eps_k + 2^-15,      eps_k = 2^-22 (1 + |v_k - max v|)       [bins]
bounds what an fp32 softmax expectation may differ from d by: eps_k is the relative error of exp(v_k - max v) computed as
exp2((v_k - max v) * log2 e) in fp32 with a 1-ulp exp2 (the product's rounding error, 2^-24 |v_k - max v| log2 e relative to its
value, turns into that much relative error of the result), 30 = 2 * 15 carries it into numerator and denominator of
sum k e_k / sum e_k (k <= 15), and 2^-15 is twice the rounding of two 16-term fp32 sums of values <= 15.  A box then carries
    cx, cy: stride (E_a + E_b) / 2 + 4 ulp,        w, h: stride (E_a + E_b) + 4 ulp        (a, b = l, r or t, b)
with fp32 ulps at the reference's magnitude.  E is about 4.5e-5 bins on flat rows.  Measured on the CPU (test_misc_ref.py, fp32
emulations of the expf form of decode_kernel / box_decode_kernel and of the exp2 butterfly form of the fused conv epilogue, on
every logit set below and normals of scale 0.5 to 40, 20000 rows each): the largest |d_fp32 - d| / E is 0.10 for either form
(normals of scale 5 to 10); one-hot and all-equal rows come out exact."""
import numpy as np

# ---- pools -----------------------------------------------------------------------------------------------------------------------
POOL_RADII = (2, 4, 6)          # three chained MaxPool2d(5, 1, 2) == windows of 5, 9, 13 clipped to the map


def _slide_max(a, r, fill):
    """max over the (2r+1)^2 window clipped to the map of a [B,H,W,C] array (separable); `fill` is below every element."""
    B, H, W, C = a.shape
    p = np.full((B, H, W + 2 * r, C), fill, a.dtype)
    p[:, :, r:r + W] = a
    m = p[:, :, 0:W]
    for d in range(1, 2 * r + 1):
        m = np.maximum(m, p[:, :, d:d + W])
    p = np.full((B, H + 2 * r, W, C), fill, a.dtype)
    p[:, r:r + H] = m
    m = p[:, 0:H]
    for d in range(1, 2 * r + 1):
        m = np.maximum(m, p[:, d:d + H])
    return m


def pool_ref(x):
    """x [B,H,W,C] -> the three pooled maps (5x5, 9x9, 13x13 windows clipped to the map), float64."""
    x = np.asarray(x, np.float64)
    return [_slide_max(x, r, -np.inf) for r in POOL_RADII]


def _vkey(val):
    """float64 values that fp32 holds exactly -> uint64 keys in the values' order, with -0 == +0."""
    f = np.asarray(val, np.float64).astype(np.float32) + np.float32(0.0)
    assert np.array_equal(f.astype(np.float64), np.asarray(val, np.float64) + 0.0)
    u = f.view(np.uint32).astype(np.uint64)
    return np.where(u >> np.uint64(31) != 0, ~u & np.uint64(0xFFFFFFFF), u | np.uint64(0x80000000))


def _member_slow(in_bits, out_bits, r, idx):
    """For the flat indices idx of out_bits: are the bits those of some element of the clipped (2r+1)^2 window?"""
    B, H, W, C = in_bits.shape
    b, y, x, c = np.unravel_index(idx, in_bits.shape)
    want = out_bits.reshape(-1)[idx]
    ok = np.zeros(idx.shape, bool)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            yy, xx = y + dy, x + dx
            inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            ok |= inside & (in_bits[b, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1), c] == want)
    return ok


def pool_verdict(in_val, in_bits, out_val, out_bits):
    """The rule above.  in_val [B,H,W,C] decoded input values and in_bits their stored bits (unsigned, any width up to 32);
    out_val / out_bits: three [B,H,W,C] arrays each (one per window).  -> three bool arrays: (a) and (b) per element.
    (b) is decided from two window maxima over (value, bits) and (value, ~bits) keys -- the largest and the smallest bit pattern
    among the window's largest values -- and by an exhaustive search of the window for whatever matches neither."""
    in_val = np.asarray(in_val, np.float64)
    ib = np.asarray(in_bits).astype(np.uint64)
    vk = _vkey(in_val) << np.uint64(32)
    mask = np.uint64(0xFFFFFFFF)
    res = []
    for r, ref, ov, ob in zip(POOL_RADII, pool_ref(in_val), out_val, out_bits):
        ob = np.asarray(ob).astype(np.uint64)
        hi = _slide_max(vk | ib, r, np.uint64(0)) & mask
        lo = mask - (_slide_max(vk | (mask - ib), r, np.uint64(0)) & mask)
        member = (ob == hi) | (ob == lo)
        rest = np.flatnonzero(~member)
        if rest.size:
            member.reshape(-1)[rest] = _member_slow(ib, ob, r, rest)
        res.append((np.asarray(ov, np.float64) == ref) & member)
    return res


def up_ref(x):
    """nearest 2x of x [B,H,W,C] (any dtype: a copy)."""
    return np.repeat(np.repeat(np.asarray(x), 2, axis=1), 2, axis=2)


# ---- decode ----------------------------------------------------------------------------------------------------------------------
def ulp32(v):
    """One fp32 unit in the last place at the magnitude of v (float64 array)."""
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)


def dfl_ref(v):
    """v [..., 16] logits -> (d, E): the softmax expectation in float64 and the bound E of the module docstring, [...]."""
    v = np.asarray(v, np.float64)
    z = v - v.max(-1, keepdims=True)
    e = np.exp(z)
    p = e / e.sum(-1, keepdims=True)
    d = (p * np.arange(16.0)).sum(-1)
    E = 30.0 * (p * (2.0 ** -22 * (1.0 + np.abs(z)))).sum(-1) + 2.0 ** -15
    return d, E


def decode_ref(box, cls, mc, levels, strides):
    """box[l] [B, H_l W_l, 64] (side-major: channel = 16 side + bin, sides l, t, r, b), cls[l] [B, H_l W_l, nc] logits, mc[l]
    [B, H_l W_l, nm]; levels: (H_l, W_l); anchors at cell centres (make_anchors, offset 0.5), levels concatenated.
    -> (pred [B, A, 4 + nc + nm] float64: cx, cy, w, h in pixels, sigmoid scores, coefficients;
        E [B, A, 4] per side in bins;  bound [B, A, 4]: what an fp32 decode may differ by in cx, cy, w, h)."""
    preds, Es, bounds = [], [], []
    for bx, cl, m, (H, W), st in zip(box, cls, mc, levels, strides):
        B = bx.shape[0]
        d, E = dfl_ref(np.asarray(bx, np.float64).reshape(B, H * W, 4, 16))
        la = np.arange(H * W)
        ax, ay = (la % W + 0.5)[None], (la // W + 0.5)[None]
        x1, y1, x2, y2 = ax - d[..., 0], ay - d[..., 1], ax + d[..., 2], ay + d[..., 3]
        xywh = np.stack(((x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1), -1) * st
        ex, ey = E[..., 0] + E[..., 2], E[..., 1] + E[..., 3]
        bounds.append(np.stack((ex / 2, ey / 2, ex, ey), -1) * st + 4 * ulp32(xywh))
        score = 1.0 / (1.0 + np.exp(-np.asarray(cl, np.float64)))
        preds.append(np.concatenate((xywh, score, np.asarray(m, np.float64)), -1))
        Es.append(E)
    return np.concatenate(preds, 1), np.concatenate(Es, 1), np.concatenate(bounds, 1)


def scores_ok(got, ref, logits):
    """Scores: within 4 fp32 ulps of the float64 sigmoid -- and exactly 0 or 1 at logits of -100 / +100, where the float64 answer
    (3.7e-44) lies below fp32's normal range and an fp32 sigmoid, 1 / (1 + exp(100)) = 1 / inf, answers 0.  The case lists keep
    every other logit inside +-80, clear of that range.  -> bool array."""
    got, ref, logits = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(logits, np.float64)
    return np.where(np.abs(logits) == 100.0, got == (logits > 0), np.abs(got - ref) <= 4 * ulp32(ref))


# fp32 emulations of the two forms the kernels use (numpy float32 arithmetic, exp / exp2 correctly rounded: within the 1 ulp the
# bound allows), for the CPU check that a correct fp32 softmax expectation sits well inside E
def dfl_fp32_expf(v):
    """decode_kernel / box_decode_kernel: e_k = expf(v_k - max), sequential sum, d = sum (e_k / sum) * k."""
    v = np.asarray(v, np.float32)
    e = np.exp((v - v.max(-1, keepdims=True)).astype(np.float64)).astype(np.float32)
    s = np.zeros(v.shape[:-1], np.float32)
    for k in range(16):
        s = s + e[..., k]
    d = np.zeros(v.shape[:-1], np.float32)
    for k in range(16):
        d = d + (e[..., k] / s) * np.float32(k)
    return d.astype(np.float64)


def dfl_fp32_exp2(v):
    """the fused conv epilogue: e_k = exp2((v_k - max) * log2e), four-bin partial sums, a butterfly over the four groups, w / s."""
    v = np.asarray(v, np.float32)
    t = (v - v.max(-1, keepdims=True)) * np.float32(1.4426950408889634)
    e = np.exp2(t.astype(np.float64)).astype(np.float32).reshape(v.shape[:-1] + (4, 4))
    k = np.arange(16, dtype=np.float32).reshape(4, 4)
    s = (e[..., 0] + e[..., 1]) + (e[..., 2] + e[..., 3])
    w = (e[..., 0] * k[:, 0] + e[..., 1] * k[:, 1]) + (e[..., 2] * k[:, 2] + e[..., 3] * k[:, 3])
    s = (s[..., 0] + s[..., 1]) + (s[..., 2] + s[..., 3])        # lanes l, l^16 then l^32
    w = (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])
    return (w / s).astype(np.float64)


# ---- the decode cases: shared by the GPU tests and their CPU pin --------------------------------------------------------------------
DECODE_LEVELS = [((7, 11), (4, 6), (2, 3)), ((9, 8), (5, 4), (3, 2))]      # 107 anchors: tiles of 64 + 13, 24 and 6, all clipped
DECODE_STRIDES = (8, 16, 32)
# (nc, nm): up to 159 + 32 the full decode takes 64 anchors per workgroup; 160 + 32: 63; 1025 + 32: 14 (tiles of 14 x 5 + 7, 14 + 10, 6)
DECODE_CLASSES = [(1, 32), (2, 32), (80, 32), (159, 32), (2, 64), (160, 32), (1025, 32)]
BOX_SETS = ("normal 1", "normal 10", "normal 40", "one-hot 0", "one-hot 7", "one-hot 15", "equal")
ONE_HOT_SPREAD = 60.0
CLS_PLANTED = (0.0, 20.0, -20.0, 100.0, -100.0)


def box_rows(name, n, rng):
    """n rows of 16 box logits of one set (float32)."""
    kind, _, arg = name.partition(" ")
    if kind == "normal":
        v = rng.standard_normal((n, 16)) * float(arg)
    elif kind == "one-hot":          # a peak of ONE_HOT_SPREAD over a low ripple, the whole row shifted: softmax must subtract the maximum
        v = rng.standard_normal((n, 16)) * 0.5 + rng.uniform(-40, 40, (n, 1))
        v[:, int(arg)] += ONE_HOT_SPREAD
    else:                            # all sixteen bins equal: d = 7.5 whatever the level
        v = np.repeat(rng.uniform(-90, 90, (n, 1)), 16, 1)
        for i, c in enumerate((0.0, 88.0, -88.0)[:n]):
            v[i] = c
    return v.astype(np.float32)


def decode_inputs(levels, B, nc, nm, seed):
    """-> (box, cls, mc, set_of_row): float32 inputs of one decode case.  Anchor side r (counted over batch, level, anchor and
    side) takes its logits from set r % 7, so every set meets every level, side and tile position.  Class logits: normals of
    scale 3 with CLS_PLANTED written over the first entries of every level; coefficients: normals of scale 2."""
    rng = np.random.default_rng(seed)
    box, cls, mc, which = [], [], [], []
    r0 = 0
    for H, W in levels:
        n = B * H * W * 4
        sets = (r0 + np.arange(n)) % len(BOX_SETS)
        r0 += n
        rows = np.zeros((n, 16), np.float32)
        for i, name in enumerate(BOX_SETS):
            rows[sets == i] = box_rows(name, int((sets == i).sum()), rng)
        box.append(rows.reshape(B, H * W, 64))
        which.append(sets.reshape(B, H * W, 4))
        c = (rng.standard_normal((B, H * W, nc)) * 3).astype(np.float32)
        flat = c.reshape(-1)
        flat[:len(CLS_PLANTED)] = CLS_PLANTED[:flat.size]
        flat[-len(CLS_PLANTED):] = CLS_PLANTED[:flat.size][::-1]
        cls.append(c)
        mc.append((rng.standard_normal((B, H * W, nm)) * 2).astype(np.float32))
    return box, cls, mc, np.concatenate(which, 1)
