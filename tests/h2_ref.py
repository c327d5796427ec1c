"""The h2 (split-fp16 pair) arithmetic of the conv family, stated once in numpy float64.  Takes nothing from the library: the
tests hold the kernels, vti_amd.h2_encode / h2_decode and the weight packers against THIS statement.

  activation  v (an fp32 value)  ->  clamp to +-4094, s = 16 v, hi = fp16(s), lo = fp16(s - hi); stored as (hi | lo << 16).
              4094 * 16 = 65504 is the largest fp16, so hi is always finite and lo = 0 at the limit.  lo is a normal fp16
              number down to |v| ~ 8e-3; below that the pair has an absolute floor of 2^-24 / 16.
  weight      one power of two SW per conv puts max|w| in [2^13, 2^14): wh = fp16(w SW), wl = fp16(w SW - wh).
  conv        acc = sum wh * (xh + xl) + wl * xh  over taps and channels (fp32 accumulators in the kernel; wl * xl is dropped
              by design: below 2^-22 of the sum), pre-activation = acc / (16 SW) + bias, then SiLU, then + residual, then
              the activation encode.
"""
import numpy as np

H2_SX = 16.0
H2_MAX = 4094.0         # 4094 * 16 = 65504, the largest finite fp16


def _f16(a):
    with np.errstate(over="ignore"):
        return np.asarray(a, np.float64).astype(np.float16).astype(np.float64)


def enc_act(v):
    """fp32 values -> (hi, lo) as float64 arrays holding fp16 values.  The + 0.0 is the device's fma(v, 16, +0): -0 encodes as +0."""
    v = np.asarray(v, np.float32).astype(np.float64)
    s = np.clip(v, -H2_MAX, H2_MAX) * H2_SX + 0.0
    hi = _f16(s)
    lo = _f16(s - hi)
    return hi, lo


def dec(hi, lo):
    return (np.asarray(hi, np.float64) + np.asarray(lo, np.float64)) / H2_SX


def bits(hi, lo):
    """the stored dword (hi | lo << 16) as int32."""
    h = np.asarray(hi, np.float64).astype(np.float16).view(np.uint16).astype(np.uint32)
    l = np.asarray(lo, np.float64).astype(np.float16).view(np.uint16).astype(np.uint32)
    return (h | (l << np.uint32(16))).view(np.int32)


def unit(vmax):
    """One unit in the last place of an h2 pair at magnitude vmax: hi has 11 bits, lo 11 more below hi's half unit, and fp16's
    subnormal spacing 2^-24 is the absolute floor (all of 16 v)."""
    s = H2_SX * np.minimum(np.abs(np.asarray(vmax, np.float64)), H2_MAX)
    e = np.floor(np.log2(np.maximum(s, 2.0 ** -24)))
    return np.maximum(2.0 ** (e - 21), 2.0 ** -24) / H2_SX


def q_act(v):
    """v as the h2 storage keeps it."""
    return dec(*enc_act(v))


def enc_w(w):
    """fp32 weights of ONE conv -> (wh, wl, SW): SW = 2^(14 - e) with max|w| = m 2^e, m in [0.5, 1); all zero: SW = 1."""
    w = np.asarray(w, np.float32).astype(np.float64)
    mx = float(np.abs(w).max()) if w.size else 0.0
    sw = 2.0 ** (14 - np.frexp(mx)[1]) if mx > 0 else 1.0
    wh = _f16(w * sw)
    wl = _f16(w * sw - wh)
    return wh, wl, sw


def q_w(w):
    wh, wl, sw = enc_w(w)
    return (wh + wl) / sw


def out_hw(H, W, k, s, kind):
    return (2 * H, 2 * W) if kind == 2 else ((H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1)


def lin(x, w, k, s, kind):
    """The linear part of an engine conv in float64: x NHWC [B,H,W,c1]; w OIHW [c2,c1,k,k] with padding k // 2 (kind 0 / 1),
    or IOHW [c1,c2,2,2] for the ConvTranspose2d(2, 2) (kind 2).  -> NHWC [B,Ho,Wo,c2]."""
    x = np.asarray(x, np.float64)
    w = np.asarray(w, np.float64)
    B, H, W, c1 = x.shape
    Ho, Wo = out_hw(H, W, k, s, kind)
    if kind == 2:
        c2 = w.shape[1]
        y = np.einsum("bhwi,iopq->bhpwqo", x, w)          # out[b, 2h+p, 2w+q, o]
        return np.ascontiguousarray(y.reshape(B, Ho, Wo, c2))
    c2 = w.shape[0]
    p = k // 2
    xp = np.zeros((B, H + 2 * p, W + 2 * p, c1))
    xp[:, p:p + H, p:p + W] = x
    y = np.zeros((B, Ho, Wo, c2))
    for dy in range(k):
        for dx in range(k):
            y += xp[:, dy:dy + (Ho - 1) * s + 1:s, dx:dx + (Wo - 1) * s + 1:s] @ w[:, :, dy, dx].T
    return y


def silu(y):
    return y / (1.0 + np.exp(-y))


def scheme_acc(xh, xl, wh, wl, k, s, kind):
    return lin(xh + xl, wh, k, s, kind) + lin(xh, wl, k, s, kind)


def conv_scheme(x, w, b, k, s, kind, res=None, act=None, encode=False, hi_only_w=False):
    """What a correct h2 kernel computes, up to its fp32 accumulation: x NHWC and res NHWC are fp32 values (encoded here as the
    kernel's inputs are), w / b the conv's fp32 weights and bias.  act defaults to kind == 0.  encode: return the int32 dwords of
    the stored output, else the float64 value before the final encode.  hi_only_w drops the wl operand (to show on the host that
    a comparison would notice a lost lo half)."""
    xh, xl = enc_act(x)
    wh, wl, sw = enc_w(w)
    if hi_only_w:
        wl = np.zeros_like(wl)
    y = scheme_acc(xh, xl, wh, wl, k, s, kind) / (H2_SX * sw) + np.asarray(b, np.float32).astype(np.float64)
    if kind == 0 if act is None else act:
        y = silu(y)
    if res is not None:
        y = y + dec(*enc_act(res))
    return bits(*enc_act(y)) if encode else y


def _val2(a):
    """smallest power-of-two exponent among the nonzero entries of a (each an fp16 value): a = odd * 2^e."""
    a = np.abs(np.asarray(a, np.float64))
    a = a[a != 0]
    if a.size == 0:
        return None
    m, e = np.frexp(a)                       # m in [0.5, 1) with at most 11 significant bits
    mi = (m * 2048).astype(np.int64)
    tz = np.zeros_like(mi)
    for _ in range(11):
        even = (mi & 1) == 0
        tz += even
        mi = np.where(even, mi >> 1, mi)
    return int((e - 11 + tz).min())


def exactness(x, w, k, s, kind):
    """-> (granule, max over outputs of sum|terms| / granule) for the operands of conv_scheme(x, w, ...).  granule: a power of
    two that divides every product wh * xh, wh * xl, wl * xh (from the operands' trailing zeros: a lower bound of the largest
    such).  Below 2^24 the case is split-exact: every partial sum, in any order, is a multiple of the granule below 2^24
    granules, hence exact in fp32."""
    xh, xl = enc_act(x)
    wh, wl, _ = enc_w(w)
    v = {n: _val2(a) for n, a in (("xh", xh), ("xl", xl), ("wh", wh), ("wl", wl))}
    es = [v[a] + v[b] for a, b in (("wh", "xh"), ("wh", "xl"), ("wl", "xh")) if v[a] is not None and v[b] is not None]
    if not es:
        return 1.0, 0.0
    g = 2.0 ** min(es)
    tot = lin(np.abs(xh) + np.abs(xl), np.abs(wh), k, s, kind) + lin(np.abs(xh), np.abs(wl), k, s, kind)
    return g, float(tot.max() / g)


SPLIT_EXACT = 2.0 ** 24


def split_operands(rng, xshape, wshape, x_int=2):
    """The worked split-exact construction: x = xi + sign(xi) xf 2^-13 (xi in [-x_int, x_int], xf in 0..3: hi = 16 xi, lo = xf 2^-9)
    and w = wi + sign(wi) wf 2^-12 (wi in {-1, 0, 1}, wf in {0, 1}: SW = 8192, wh = 8192 wi, wl = +-2).  Asymmetric between x and w."""
    xi = rng.integers(-x_int, x_int + 1, xshape).astype(np.float64)
    xf = rng.integers(0, 4, xshape).astype(np.float64)
    wi = rng.integers(-1, 2, wshape).astype(np.float64)
    wf = rng.integers(0, 2, wshape).astype(np.float64)
    x = (xi + np.sign(xi) * xf * 2.0 ** -13).astype(np.float32)
    w = (wi + np.sign(wi) * wf * 2.0 ** -12).astype(np.float32)
    return x, w


def split_case(seed, xshape_full, in_coff, c1, wshape, k, s, kind, res=False):
    """One bit-for-bit h2 case on the worked construction, with small integer bias (and residual): -> (x_full, x, w, b, res or
    None, float64 result), asserted split-exact on the host.  The activation integers shrink from [-2, 2] to [-1, 1] where a
    shape needs it; the assertion does not move."""
    B, H, W, _ = xshape_full
    c2 = wshape[1] if kind == 2 else wshape[0]
    for x_int in (2, 1):
        rng = np.random.default_rng(seed)
        x_full, w = split_operands(rng, xshape_full, wshape, x_int)
        x = x_full[..., in_coff:in_coff + c1]
        b = rng.integers(-3, 4, (c2,)).astype(np.float32)
        r = rng.integers(-4, 5, (B,) + out_hw(H, W, k, s, kind) + (c2,)).astype(np.float32) if res else None
        if exactness(x, w, k, s, kind)[1] < SPLIT_EXACT:
            break
    return x_full, x, w, b, r, assert_split_exact(x, w, b, k, s, kind, res=r)


def assert_split_exact(x, w, b, k, s, kind, res=None):
    """Host-side precondition of a bit-for-bit h2 case: the accumulation is split-exact, the lo operands are really there, and the
    pre-activation, the result and its stored pair are exact.  Returns the float64 result."""
    g, n = exactness(x, w, k, s, kind)
    assert n < SPLIT_EXACT, (g, n)
    xh, xl = enc_act(x)
    wh, wl, sw = enc_w(w)
    assert (xl != 0).mean() > 0.3 and (wl != 0).mean() > 0.2, ((xl != 0).mean(), (wl != 0).mean())
    pre = scheme_acc(xh, xl, wh, wl, k, s, kind) / (H2_SX * sw) + np.asarray(b, np.float64)
    y = conv_scheme(x, w, b, k, s, kind, res=res, act=False)
    for a in (pre, y):
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a)       # what the fp32 epilogue holds
    assert np.array_equal(q_act(y), y)                                          # exactly an h2 pair
    return y
