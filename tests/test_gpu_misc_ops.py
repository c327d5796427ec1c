"""The non-GEMM kernels of csrc/misc.hip one at a time, through vti_debug_sppf_pool / vti_debug_upsample2x / vti_debug_decode,
against the float64 statements of tests/misc_ref.py (pinned on the CPU by test_misc_ref.py), and the three places where DFL +
dist2bbox is computed (decode_kernel, box_decode_kernel, the fused box-tower epilogue) against each other on a trained-like head.

Inside vti_forward these kernels are seen only through the next conv or through pred, under bounds of 4e-5 to 6e-3 of a layer's
maximum on random nets: SiLU outputs whose windows nearly always hold a positive value, flat DFL rows, one pool path per canvas.
Here every output buffer is poisoned and carries a guard band, every channel outside the written slices must still hold the
poison, and the input slice must be unchanged.

Pools: the rule of misc_ref (value == the float64 maximum of the clipped window, bits those of an element of the window; the
tie-break stays open), on all three launch paths -- asserted from the launcher's own sppf_pool_path -- for fp16, fp32 and h2.
Decode: boxes within misc_ref's fp32 bound E (derived there; nothing in it is fitted to a kernel), scores within 4 fp32 ulps of
the float64 sigmoid and exactly 0 / 1 at -100 / +100, coefficients bit for bit, box_only leaving every other channel alone.

Largest |d box| / bound measured on an MI355X (the bound is dominated by its constant 2^-15 bins per side, which the kernels'
sixteen-term sums do not come near; the CPU emulations of misc_ref sit at 0.10 of E alone):
  decode_kernel      0.040  (levels (9,8)/(5,4)/(3,2), nc = 80; 0.027 to 0.040 over all fourteen cases, 0.037 at 1025 classes)
  box_decode_kernel  0.040  (the same boxes as decode_kernel on the same inputs)
  three engines, canvas 224x352, box logits up to |30.5| with spreads up to 43.6:
    h2    box_decode 0.072  decode 0.072  fused 0.074 of the bare bound (0.026 with its logit term of at most 0.40 px)
    fp16  box_decode 0.069  decode 0.069  fused 0.078 of the bare bound (0.001 with its logit term of at most 61 px)
  so the fused epilogue's exp2 / butterfly form is as close to the float64 decode of the stored logits as the two kernels are,
  and the logit term, which the fp16 per-layer bound makes very wide, is not what lets it pass.
No kernel needed a change for a wrong result.  decode_kernel now takes fewer than 64 anchors per workgroup when 64 rows do not fit
into LDS (it used to refuse nc + nm > 191 with a bare HIP error at the first forward): the 160- and 1025-class cases run that.

Sensitivity, tried once, on scratch libraries with one VALUE changed each (no address touched); all five fail here:
  pool padding 0 instead of the lowest value     7 tests: every global-33x63 case and the grid-stride case ("negative": every
                                                 element of all three windows; "normal": 1 of 99 792 and 45 of 4 333 568 elements)
  h2 vmax comparing hi alone                     16 tests: every h2 pool case but 1x1 ("pairs": 81 of 288 up to 1125 of 2464
                                                 elements; "normal": 1 to 67 elements per case, e.g. 10420.855 for 10427.598)
  9x9 window cut at ad <= 3                      the same 7 global tests (38 % of the 9x9 elements)
  two bin weights swapped in box_decode_kernel   6 tests: all four box_decode cases (x13 189 to x16 994 of the bound) and both
                                                 three-engine tests (box_decode engine: 52.5 px for 68.0 px)
  the xor-32 step of the fused epilogue's sum    both three-engine tests (fused engine: 5.4e7 px for 171.9 px)
  dropped"""
import functools

import numpy as np
import pytest
import torch

import h2_ref
import misc_ref as M
from gpu_util import LAYER_TOL, check_pred_proto, frames_u8, need_gpu, plan_env

pytestmark = pytest.mark.gpu

GUARD = 64                                   # elements of poison in front of and behind every output buffer
POISON = {2: 0x7BC5, 4: 0x7F4A5A5A}          # per element size: large finite numbers no case produces
INT = {2: (torch.int16, np.int16, np.uint16), 4: (torch.int32, np.int32, np.uint32)}
ESIZE = {"fp16": 2, "fp32": 4, "h2": 4}
VEC = {"fp16": 8, "fp32": 4, "h2": 4}
FLOAT = {2: torch.float16, 4: torch.float32}


class Buf:
    """A poisoned device buffer of `shape` elements of `esize` bytes with GUARD elements of poison on either side."""

    def __init__(self, shape, esize):
        self.shape, self.esize = tuple(shape), esize
        self.n = int(np.prod(shape))
        tint, nint, _ = INT[esize]
        self.flat = torch.full((self.n + 2 * GUARD,), int(np.array(POISON[esize], INT[esize][2]).view(nint)), dtype=tint, device="cuda")
        self.ints = self.flat[GUARD:GUARD + self.n].view(self.shape)
        self.t = self.ints.view(FLOAT[esize])                       # what the wrappers take

    def put(self, chan, bits):
        """bits: unsigned numpy array [..., C] -> channels chan of the buffer."""
        self.ints[..., chan] = torch.from_numpy(np.ascontiguousarray(bits).view(INT[self.esize][1])).cuda()

    def get(self):
        """-> (the tensor's bits as an unsigned numpy array, True if both guard bands still hold the poison)."""
        a = self.flat.cpu().numpy().view(INT[self.esize][2])
        guards = np.concatenate((a[:GUARD], a[GUARD + self.n:]))
        return a[GUARD:GUARD + self.n].reshape(self.shape), bool((guards == POISON[self.esize]).all())


def encode(dtype, v):
    """float64 values -> (the values as the type stores them, float64; their bits, unsigned)."""
    if dtype == "fp16":
        h = np.asarray(v).astype(np.float16)
        return h.astype(np.float64), h.view(np.uint16)
    if dtype == "fp32":
        f = np.asarray(v).astype(np.float32)
        return f.astype(np.float64), f.view(np.uint32)
    hi, lo = h2_ref.enc_act(np.asarray(v, np.float32))
    return hi + lo, h2_ref.bits(hi, lo).view(np.uint32)


def decode(dtype, bits):
    """stored bits -> float64 values (h2: hi + lo, the value the kernel compares; the common 1/16 does not matter)."""
    if dtype == "fp16":
        return bits.view(np.float16).astype(np.float64)
    if dtype == "fp32":
        return bits.view(np.float32).astype(np.float64)
    return (bits & 0xFFFF).astype(np.uint16).view(np.float16).astype(np.float64) + (bits >> 16).astype(np.uint16).view(np.float16).astype(np.float64)


# ---- SPPF pools ----------------------------------------------------------------------------------------------------------------------
SCALES = (1e-3, 1.0, 300.0)
SPOTS = ("top-left", "top-right", "bottom-left", "bottom-right", "centre")


def spot_yx(H, W, c):
    return [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)][c % 5]


def h2_pairs(rng, shape):
    """(iv) raw h2 pairs, one family per channel (c % 4):
    0  equal hi, lo of both signs and several magnitudes (and both zeros): only lo decides, and as a SIGNED number;
    1  neighbouring hi with lo chosen against it: hi + lo of (1025, -0.5) equals that of (1024, +0.5) (the tie an encoder can
       produce), and raw pairs such as (1025, -0.75) lie BELOW (1024, +0.5): the larger hi is the smaller or the equal value;
       the same mirrored for negative hi;
    2  the four spellings of zero among small negative values: the maximum is a zero, of whichever spelling;
    3  +-65504 (the largest fp16, lo = 0) among ordinary values."""
    B, H, W, C = shape
    fam = [
        [(1024.0, l) for l in (0.5, -0.5, 0.25, -0.25, 2.0 ** -10, -2.0 ** -10, 0.0, -0.0, 0.4375, -0.4375)],
        [(1024.0, 0.5), (1025.0, -0.5), (1025.0, -0.75), (1026.0, -1.75), (1024.0, 0.25), (1025.0, -1.0),
         (-1025.0, 0.5), (-1024.0, -0.5), (-1024.0, -0.75), (-1023.0, -1.75)],
        [(0.0, 0.0), (-0.0, -0.0), (0.0, -0.0), (-0.0, 0.0), (-2.0 ** -14, 0.0), (-1.0, 2.0 ** -12), (-2.0 ** -24, -0.0)],
        [(65504.0, 0.0), (-65504.0, 0.0), (1000.0, 0.25), (-1000.0, -0.25), (3.0, 0.0), (65472.0, 15.0)],
    ]
    hi, lo = np.zeros(shape), np.zeros(shape)
    for c in range(C):
        f = np.array(fam[c % 4])
        p = np.array([0.3] + [0.7 / (len(f) - 1)] * (len(f) - 1)) if c % 4 == 3 else None      # +65504 often: it has to win
        if c % 4 == 2:
            p = np.array([0.02] * 4 + [0.92 / 3] * 3)                                           # zeros rare: windows with and without one
        i = rng.choice(len(f), size=(B, H, W), p=p)
        hi[..., c], lo[..., c] = f[i, 0], f[i, 1]
    return hi + lo, h2_ref.bits(hi, lo).view(np.uint32)


def pool_content(kind, dtype, shape, seed):
    """-> (values float64, bits): one input slice [B,H,W,C] of a pool case."""
    rng = np.random.default_rng(seed)
    B, H, W, C = shape
    scale = np.array([SCALES[c % 3] for c in range(C)])
    if kind == "pairs":
        return h2_pairs(rng, shape)
    v = rng.standard_normal(shape) * scale
    if kind == "negative":                   # (ii) a pool padded with 0 is wrong at every clipped window
        v = -np.abs(v) - scale * 1e-2
    if kind == "peak":                       # (iii) one strictly largest element per channel and frame
        for b in range(B):
            for c in range(C):
                y, x = spot_yx(H, W, b + c)
                v[b, y, x, c] = 8.0 * scale[c] + np.abs(v[b, :, :, c]).max()
    val, bits = encode(dtype, v)
    if kind == "negative":
        assert (val < 0).all()
    return val, bits


def run_pool(dtype, shape, ld, in_coff, out_coff, path, kinds, shared=True, seed=0):
    import vti_amd
    B, H, W, C = shape
    es = ESIZE[dtype]
    for kind in kinds:
        val, bits = pool_content(kind, dtype, shape, seed)
        buf = Buf((B, H, W, ld), es)
        src = buf if shared else Buf((B, H, W, ld), es)
        src.put(slice(in_coff, in_coff + C), bits)
        _, got_path = vti_amd.debug_sppf_pool(src.t, C, dtype, in_coff=in_coff, out=buf.t, out_coff=out_coff)
        torch.cuda.synchronize()
        assert got_path == path, f"{kind}: the launcher chose path {got_path}, the case is meant for {path}"
        out, guards = buf.get()
        assert guards, f"{kind}: a guard band was written"
        inp = out if shared else src.get()[0]
        assert np.array_equal(inp[..., in_coff:in_coff + C], bits), f"{kind}: the input slice changed"
        written = np.zeros(ld, bool)
        written[out_coff:out_coff + 3 * C] = True
        if shared:
            written[in_coff:in_coff + C] = True
        assert (out[..., ~written] == POISON[es]).all(), f"{kind}: a channel outside the slices was written"
        if not shared:
            assert (src.get()[0][..., [c for c in range(ld) if not in_coff <= c < in_coff + C]] == POISON[es]).all() and src.get()[1]
        ob = [out[..., out_coff + i * C:out_coff + (i + 1) * C] for i in range(3)]
        ov = [decode(dtype, np.ascontiguousarray(o)) for o in ob]
        for r, ok, o in zip(M.POOL_RADII, M.pool_verdict(val, bits, ov, ob), ov):
            bad = np.argwhere(~ok)
            assert ok.all(), (f"{kind}, {2 * r + 1}x{2 * r + 1}: {len(bad)} of {ok.size} elements break the rule, first at (b, y, x, c) = "
                              f"{bad[0].tolist()}: got {o[tuple(bad[0])]!r}, window maximum {M.pool_ref(val)[M.POOL_RADII.index(r)][tuple(bad[0])]!r}")
        if kind == "peak":
            for b in range(B):
                for c in range(C):
                    y, x = spot_yx(H, W, b + c)
                    peak = val[b, y, x, c]
                    yy, xx = np.mgrid[0:H, 0:W]
                    for r, o in zip(M.POOL_RADII, ov):
                        square = (np.abs(yy - y) <= r) & (np.abs(xx - x) <= r)
                        assert np.array_equal(o[b, :, :, c] == peak, square), f"peak at {SPOTS[(b + c) % 5]}, {2 * r + 1}x{2 * r + 1}, frame {b} channel {c}"
                        assert (o[b, :, :, c][~square] < peak).all()


def c_of(dtype, c16):
    """The issue's channel counts are given for fp16; the 4-byte types take half as many (the same number of 16-byte vectors)."""
    return c16 if dtype == "fp16" else c16 // 2


POOL_GEOMS = (
    # name, (H, W), channels for fp16, expected path, layout
    [(f"lds4-{h}x{w}", (h, w), 32, 4, "engine") for h, w in ((7, 11), (20, 20), (16, 32), (1, 1), (1, 9), (9, 1), (3, 4))] +
    [("lds4-7x11-C128", (7, 11), 128, 4, "engine"), ("lds4-7x11-two-buffers", (7, 11), 32, 4, "two"), ("lds4-7x11-odd", (7, 11), 32, 4, "odd"),
     ("lds1-remainder-7x11", (7, 11), 24, 1, "engine"), ("lds1-remainder-7x11-odd", (7, 11), 24, 1, "odd")] +
    [(f"lds1-size-{h}x{w}", (h, w), 32, 1, "engine") for h, w in ((19, 27), (23, 30), (32, 64))] +
    [("global-33x63", (33, 63), 32, 0, "engine"), ("global-33x63-odd", (33, 63), 24, 0, "odd")])


@pytest.mark.parametrize("dtype", ["fp16", "fp32", "h2"])
@pytest.mark.parametrize("name,hw,c16,path,layout", POOL_GEOMS, ids=[g[0] for g in POOL_GEOMS])
def test_sppf_pool(dtype, name, hw, c16, path, layout):
    """B = 2.  lds4: four vectors per lane group (512 pixels at most, C a multiple of four vectors), maps narrower than the windows
    included; lds1 by channel remainder (C = 3 vectors) and by size (513 to exactly 2048 pixels); global above that.  Layouts:
    the engine's (ld = 4 C, input first, one buffer), two buffers, and odd (ld = 4 C + 3 vectors, in_coff = 1 vector, out_coff =
    in_coff + C + 1 vector).  Contents (i) normals at scales 1e-3, 1, 300 by channel, (ii) all negative, (iii) one peak per
    channel at a corner or the centre, (iv) h2: raw pairs."""
    need_gpu()
    C = c_of(dtype, c16) if name != "lds4-7x11-C128" else 128
    v = VEC[dtype]
    ld, in_coff, out_coff = (4 * C + 3 * v, v, v + C + v) if layout == "odd" else (4 * C, 0, C)
    kinds = ("normal", "negative", "peak") + (("pairs",) if dtype == "h2" else ())
    run_pool(dtype, (2,) + hw + (C,), ld, in_coff, out_coff, path, kinds, shared=layout != "two", seed=len(name))


def test_sppf_pool_global_grid_stride():
    """46x46 at C = 1024 in fp32, B = 2: 1 083 392 vectors, more than the 4096 x 256 lanes of the global kernel's largest grid, so
    its grid-stride loop takes a second step."""
    need_gpu()
    assert 2 * 46 * 46 * 1024 // 4 > 4096 * 256
    run_pool("fp32", (2, 46, 46, 1024), 4096, 0, 1024, 0, ("normal",))


# ---- upsample --------------------------------------------------------------------------------------------------------------------------
UP_GEOMS = [("1x1", 2, (1, 1), 16), ("7x11", 2, (7, 11), 16), ("23x30", 2, (23, 30), 16), ("40x40-C512", None, (40, 40), 512)]


@pytest.mark.parametrize("dtype", ["fp16", "fp32", "h2"])
@pytest.mark.parametrize("name,B,hw,C", UP_GEOMS, ids=[g[0] for g in UP_GEOMS])
def test_upsample2x(dtype, name, B, hw, C):
    """Bit-equal to up_ref on arbitrary bit patterns (NaNs and infinities included: a copy), in and out both channel slices of
    wider tensors.  40x40 -> 80x80 at C = 512 is more than 4096 x 256 vectors (B = 3 for fp16, whose vectors hold 8 elements)."""
    need_gpu()
    import vti_amd
    es, v = ESIZE[dtype], VEC[dtype]
    if B is None:
        B = 3 if dtype == "fp16" else 2
        assert B * 80 * 80 * C // v > 4096 * 256
    H, W = hw
    in_ld, in_coff, out_ld, out_coff = C + 2 * v, v, 2 * C + 3 * v, C + v
    rng = np.random.default_rng(H * W + es)
    bits = rng.integers(0, 2 ** (8 * es), (B, H, W, C), dtype=np.uint64).astype(INT[es][2])
    src, dst = Buf((B, H, W, in_ld), es), Buf((B, 2 * H, 2 * W, out_ld), es)
    src.put(slice(in_coff, in_coff + C), bits)
    vti_amd.debug_upsample2x(src.t, C, dst.t, dtype, in_coff=in_coff, out_coff=out_coff)
    torch.cuda.synchronize()
    out, guards = dst.get()
    assert guards
    assert np.array_equal(out[..., out_coff:out_coff + C], M.up_ref(bits))
    keep = np.ones(out_ld, bool)
    keep[out_coff:out_coff + C] = False
    assert (out[..., keep] == POISON[es]).all()
    inp, guards = src.get()
    keep = np.ones(in_ld, bool)
    keep[in_coff:in_coff + C] = False
    assert guards and np.array_equal(inp[..., in_coff:in_coff + C], bits) and (inp[..., keep] == POISON[es]).all()


# ---- decode ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def decode_case(li, nc, nm):
    """(inputs, reference) of one decode case: computed once, shared, never written to."""
    levels = M.DECODE_LEVELS[li]
    box, cls, mc, which = M.decode_inputs(levels, 2, nc, nm, seed=10 * li + nc)
    return (box, cls, mc, which), M.decode_ref(box, cls, mc, levels, M.DECODE_STRIDES)


def run_decode(li, nc, nm, box_only):
    import vti_amd
    levels = M.DECODE_LEVELS[li]
    (box, cls, mc, which), (ref, E, bound) = decode_case(li, nc, nm)
    B, A, no = ref.shape
    dev = lambda ts: [torch.from_numpy(t).cuda() for t in ts]
    pred = Buf((B, A, no), 4)
    vti_amd.debug_decode(dev(box), None if box_only else dev(cls), None if box_only else dev(mc), levels, M.DECODE_STRIDES, nc, nm,
                         pred.t, box_only=box_only)
    torch.cuda.synchronize()
    out, guards = pred.get()
    assert guards
    got = out.view(np.float32).astype(np.float64)
    ratio = np.abs(got[..., :4] - ref[..., :4]) / bound
    side = ratio.max(-1)                      # per anchor; by set: the sets of its four sides
    per_set = {name: float(ratio[(which == i).any(-1)].max()) for i, name in enumerate(M.BOX_SETS)}
    print(f"{'box_decode_kernel' if box_only else 'decode_kernel'} levels {levels} nc={nc} nm={nm}: max |d box| / bound = {ratio.max():.3f}; "
          + ", ".join(f"{k}: {v:.3f}" for k, v in per_set.items()))
    worst = np.unravel_index(ratio.argmax(), ratio.shape)
    assert (ratio <= 1.0).all(), f"box {worst}: got {got[worst]!r}, reference {ref[worst]!r}, bound {bound[worst]:.3e} (x{ratio.max():.2f})"
    if box_only:
        assert (out[..., 4:] == POISON[4]).all(), "box_only wrote beyond the four box values"
        return float(side.max())
    logits = np.concatenate(cls, 1)
    ok = M.scores_ok(got[..., 4:4 + nc], ref[..., 4:4 + nc], logits)
    assert ok.all(), f"{(~ok).sum()} scores miss 4 ulps, first {np.argwhere(~ok)[0].tolist()}"
    assert set(got[..., 4:4 + nc][np.abs(logits) == 100.0].tolist()) == {0.0, 1.0}
    assert np.array_equal(out[..., 4 + nc:], np.concatenate(mc, 1).view(np.uint32)), "coefficients are not a bit-for-bit copy"
    return float(side.max())


@pytest.mark.parametrize("li", range(len(M.DECODE_LEVELS)))
@pytest.mark.parametrize("nc,nm", M.DECODE_CLASSES)
def test_decode_kernel(li, nc, nm):
    """The full decode: 107 anchors in tiles of 64 + 13, 24 and 6 (all clipped), B = 2, every logit set at every level; nc + nm from
    33 to the limit of 191."""
    need_gpu()
    run_decode(li, nc, nm, box_only=False)


@pytest.mark.parametrize("li", range(len(M.DECODE_LEVELS)))
@pytest.mark.parametrize("nc,nm", [(2, 32), (80, 32)])
def test_box_decode_kernel(li, nc, nm):
    """The box-only decode on the same inputs: the same boxes, and channels 4 and up of pred left at the poison."""
    need_gpu()
    run_decode(li, nc, nm, box_only=True)


# ---- the three DFL paths on a trained-like head -----------------------------------------------------------------------------------------
CANVAS, NC, B3 = (224, 352), 80, 2
BOX_GAIN = 8.0


@functools.lru_cache(maxsize=None)
def peaked_blob():
    """random_weights with the box towers' last convs (weight and bias) multiplied by 8: box logits with spreads of tens, as a
    trained checkpoint has, where the stock blob's are of order 1.  Edited through the oracle's container reader / writer."""
    import vti_amd
    from oracle.blob import read_blob, write_blob
    blob = vti_amd.random_weights(vti_amd.Engine("n", NC, H=CANVAS[0], W=CANVAS[1], max_batch=1), seed=1, gain=1.7)
    meta, convs = read_blob(blob)
    rows = []
    for name, (c1, c2, k, s, kind, w, b) in convs.items():
        g = BOX_GAIN if name in ("model.22.cv2.0.2", "model.22.cv2.1.2", "model.22.cv2.2.2") else 1.0
        rows.append((name, c1, c2, k, s, kind, w * np.float32(g), b * np.float32(g)))
    return write_blob(meta["scale"], meta["nc"], meta["nm"], meta["reg_max"], rows)


def dfl_sensitivity(v, delta):
    """The most the float64 expectation of rows v [..., 16] moves when every logit moves by at most delta: d is monotone in each
    logit with the sign of (k - d), so the extremes lie at the threshold patterns -delta below bin t, +delta from t on (and the
    mirror image); all 17 of each are tried."""
    d0 = M.dfl_ref(v)[0]
    worst = np.zeros(d0.shape)
    k = np.arange(16)
    for t in range(17):
        s = np.where(k >= t, delta, -delta)
        for sign in (1.0, -1.0):
            worst = np.maximum(worst, np.abs(M.dfl_ref(v + sign * s)[0] - d0))
    return worst


@pytest.mark.parametrize("dtype", ["h2", "fp16"])
def test_three_dfl_paths_on_a_peaked_head(monkeypatch, dtype):
    """Canvas 224x352, B = 2, three engines on one blob: the default plan (DFL + dist2bbox in the box towers' fused epilogue, no
    decode launch), VTI_NO_DFL_FUSE=1 (box_decode_kernel) and VTI_NO_PRED_SCATTER=1 (decode_kernel).  Reference: decode_ref in
    float64 on the box logits read back from the NO_DFL_FUSE engine.  The boxes of the two engines that decode stored logits
    must lie within misc_ref's bound of it.  The fused engine never stores its logits: its bound gains what a logit difference of
    delta = LAYER_TOL[dtype] * max(|logit|.max(), 1) -- the per-layer bound every conv output of these engines is held to -- can
    move the expectation by, measured on the CPU as decode_ref's own worst case over that box (dfl_sensitivity), times the
    stride (halved for cx, cy)."""
    need_gpu()
    import vti_amd
    H, W = CANVAS
    x = torch.from_numpy(frames_u8(B3, H, W, seed=3)).cuda()
    engs, preds, protos = {}, {}, {}
    for key, env in (("fused", {}), ("box_decode", {"VTI_NO_DFL_FUSE": "1"}), ("decode", {"VTI_NO_PRED_SCATTER": "1"})):
        plan_env(monkeypatch, env)
        eng = vti_amd.Engine("n", NC, H=H, W=W, max_batch=B3, dtype=dtype)
        eng.load_weights(peaked_blob(), 0)
        pred, proto = eng.forward(x, swap_rb=True)
        torch.cuda.synchronize()
        engs[key], preds[key], protos[key] = eng, pred.cpu(), proto.float().cpu()
    # the three plans differ as intended: who launches a decode, and which tower outputs exist outside pred
    idx = {t["name"]: i for i, t in enumerate(engs["fused"].conv_table())}
    assert engs["box_decode"].num_launches == engs["fused"].num_launches + 1 == engs["decode"].num_launches

    def readable(eng, name):
        try:
            eng.debug_conv_output(idx[name], B3)
            return True
        except vti_amd.VtiError:
            return False
    for l in range(3):
        box, cls = f"model.22.cv2.{l}.2", f"model.22.cv3.{l}.2"
        assert all(e.conv_table()[idx[n]]["fused"] for e in engs.values() for n in (box, cls))
        assert [readable(engs[k], box) for k in ("fused", "box_decode", "decode")] == [False, True, True]
        assert [readable(engs[k], cls) for k in ("fused", "box_decode", "decode")] == [False, False, True]
    levels = [(H // s, W // s) for s in M.DECODE_STRIDES]
    logits = [engs["box_decode"].debug_conv_output(idx[f"model.22.cv2.{l}.2"], B3).cpu().permute(0, 2, 3, 1).reshape(B3, h * w, 64).numpy()
              for l, (h, w) in enumerate(levels)]
    rows = np.concatenate([b.reshape(B3, -1, 4, 16) for b in logits], 1).astype(np.float64)
    spread = rows.max(-1) - rows.min(-1)
    assert spread.max() > 10.0, spread.max()
    zeros = lambda n: [np.zeros((B3, h * w, n), np.float32) for h, w in levels]
    ref, E, bound = M.decode_ref(logits, zeros(1), zeros(1), levels, M.DECODE_STRIDES)
    delta = LAYER_TOL[dtype] * max(float(np.abs(rows).max()), 1.0)
    sens = dfl_sensitivity(rows, delta)                                   # [B, A, 4] bins
    stride = np.concatenate([np.full(h * w, float(s)) for (h, w), s in zip(levels, M.DECODE_STRIDES)])[None, :, None]
    sx, sy = sens[..., 0] + sens[..., 2], sens[..., 1] + sens[..., 3]
    extra = np.stack((sx / 2, sy / 2, sx, sy), -1) * stride
    print(f"{dtype}: box logits |max| {np.abs(rows).max():.1f}, largest spread {spread.max():.1f}; delta {delta:.2e} logits -> "
          f"at most {extra.max():.3e} px on top of a bound of at most {bound.max():.3e} px")
    for key in ("box_decode", "decode", "fused"):
        got = preds[key].permute(0, 2, 1)[..., :4].double().numpy()
        lim = bound + (extra if key == "fused" else 0.0)
        ratio = np.abs(got - ref[..., :4]) / lim
        print(f"{dtype} {key}: max |d box| / bound = {ratio.max():.3f} (without the logit term: {(np.abs(got - ref[..., :4]) / bound).max():.3f})")
        worst = np.unravel_index(ratio.argmax(), ratio.shape)
        assert (ratio <= 1.0).all(), f"{key}: box {worst}: got {got[worst]!r}, reference {ref[..., :4][worst]!r}, bound {lim[worst]:.3e}"
    # classes and coefficients: the three engines agree under the bounds that hold against the oracle
    taps = {f"model.22.cv3.{l}.2": engs["decode"].debug_conv_output(idx[f"model.22.cv3.{l}.2"], B3).cpu() for l in range(3)}
    for key in ("fused", "box_decode"):
        check_pred_proto(preds[key], protos[key], preds["decode"], protos["decode"].permute(0, 3, 1, 2), taps, dtype, LAYER_TOL[dtype], NC, H, W)
