"""The ops the planner fuses, each stated once as plain torch float64 on NCHW tensors.  Takes nothing from the library:
test_fused_ref.py pins every function to the taps of oracle/model.py's OracleModel for the same convs, and
test_gpu_fused_ops.py holds the kernels (stem_l1_kernel, bneck_pk, conv_stage2 with its epilogues, convfold_kernel, conv1_pk with
up_src) against these statements, one op at a time.

Every function takes two hooks and an accumulation type:
  q_act  storage rounding of an activation (a float64 tensor -> float64 tensor holding storage values),
  q_w    the weights of ONE conv as the engine holds them (float32 numpy OIHW / IOHW -> float64 tensor),
  acc    torch.float64 (the reference) or torch.float32: the same evaluation -- the same rounded operands, the same rounding of
         every intermediate -- with the convolutions themselves computed in float32.  |f(acc=float32) - f(float64)| is the
         references' own error; a half-unit flip of a rounded intermediate is inside it.
hooks(dtype) gives the pair for "fp16" (round to nearest fp16), "h2" (h2_ref.q_act / h2_ref.q_w) and "fp32" (the identity).
Activations stay float64 throughout (SiLU, sigmoid and the decode are always evaluated in float64); every function returns
(out, aux) with aux["pre"] the pre-activations and aux["mid"] the rounded intermediates of its stages, for the tests' bounds.

Where the intermediates are rounded is what the kernels do (read in csrc/, stated per function)."""
import numpy as np
import torch
import torch.nn.functional as F

import h2_ref
import misc_ref


def hooks(dtype):
    """-> (q_act, q_w) of an engine dtype."""
    if dtype == "fp16":
        return (lambda t: t.to(torch.float16).to(torch.float64)), (lambda w: torch.from_numpy(np.array(w, np.float32)).to(torch.float16).to(torch.float64))
    if dtype == "h2":
        return (lambda t: torch.from_numpy(h2_ref.q_act(t.numpy()))), (lambda w: torch.from_numpy(h2_ref.q_w(np.array(w, np.float32))))
    if dtype == "fp32":
        return (lambda t: t), (lambda w: torch.from_numpy(np.array(w, np.float32)).to(torch.float64))
    raise ValueError(dtype)


def _b(b):
    return torch.from_numpy(np.array(b, np.float32)).to(torch.float64)


def conv(x, w, b, k, s, acc):
    """x float64 NCHW, w float64 OIHW (as held), b float64: the conv with padding k // 2, evaluated in `acc`, returned as float64."""
    return F.conv2d(x.to(acc), w.to(acc), b.to(acc), stride=s, padding=k // 2).to(torch.float64)


def deconv(x, w, b, acc):
    """ConvTranspose2d(2, 2): w float64 IOHW."""
    return F.conv_transpose2d(x.to(acc), w.to(acc), b.to(acc), stride=2).to(torch.float64)


def silu(y):
    return F.silu(y)


def stem_l1(frames_u8, swap_rb, w0, b0, w1, b1, w2, b2, q_act, q_w, acc=torch.float64, q_in=None, q_w0=None):
    """stem_l1_kernel: u8 frame [B,H,W,3] (numpy) -> / 255 in float32 (what torch's `im.float() / 255` gives, as test_stem_conv_u8
    does), rounded to storage -> 3x3 s2 SiLU -> q -> 3x3 s2 SiLU -> q -> 1x1 SiLU.  The kernel keeps the stem's tile and layer 1's
    register tile in the storage type (conv.hip, phases 2 and 4), hence the two q.  q_in replaces the input's conversion and q_w0
    the stem's weight hook: the h2 kernel stages the bytes as exact fp16 integers and carries the 1 / 255 in the stem's weights
    (pack_stem_toeplitz), i.e. q_in = bytes / 255 in float64 and q_w0 = 255 * q_w(float32(w / 255))."""
    x = torch.from_numpy(np.ascontiguousarray(frames_u8[..., ::-1] if swap_rb else frames_u8)).permute(0, 3, 1, 2).contiguous()
    x = q_in(x) if q_in else q_act((x.float() / 255).to(torch.float64))
    p0 = conv(x, (q_w0 or q_w)(w0), _b(b0), 3, 2, acc)
    m0 = q_act(silu(p0))
    p1 = conv(m0, q_w(w1), _b(b1), 3, 2, acc)
    m1 = q_act(silu(p1))
    p2 = conv(m1, q_w(w2), _b(b2), 1, 1, acc)
    return silu(p2), dict(pre=[p0, p1, p2], mid=[m0, m1], x=x)


def bneck(x, w1, b1, w2, b2, shortcut, q_act, q_w, acc=torch.float64, tail=None):
    """bneck_pk, the Bottleneck pair: y2 = [x +] silu(W2 * q(silu(W1 * x + b1)) + b2); the first conv's tile lives in LDS in the
    storage type (the T image).  tail = (y0, wt, bt): the C2f's closing 1x1 in the same kernel, out = silu(Wt . [y0 | x | q(y2)]
    + bt) with x = y1.  Read in bneck_pk (conv_pk.hip, phase 2's epilogue): y2 IS rounded to storage before the tail's MFMA, in
    both instantiations that have a tail -- fp16 casts it (`xB[j] = (T)v[0][j]`), h2 encodes it (`pack4<T>(v[0])`, saturating) --
    "as it would have been stored"; mirrored here.  The tail's weights are one conv's: the h2 packer scales Wa and Wb jointly.
    -> (y2 or the tail's output, aux)."""
    p1 = conv(x, q_w(w1), _b(b1), 3, 1, acc)
    m1 = q_act(silu(p1))
    p2 = conv(m1, q_w(w2), _b(b2), 3, 1, acc)
    y2 = silu(p2) + x if shortcut else silu(p2)
    if tail is None:
        return y2, dict(pre=[p1, p2], mid=[m1])
    y0, wt, bt = tail
    y2q = q_act(y2)
    p3 = conv(torch.cat((y0, x, y2q), 1), q_w(wt), _b(bt), 1, 1, acc)
    return silu(p3), dict(pre=[p1, p2, p3], mid=[m1, y2q], y2=y2)


def tower(x, w1, b1, w2, b2, mode, q_act, q_w, acc=torch.float64, stride=None):
    """conv_stage2 on a head tower: 3x3 SiLU -> q -> 1x1 (no activation: the heads' last convs), then by `mode`
      "raw"      the logits                                                        [B, c2, h, w]
      "sigmoid"  (scores, best): sigmoid, and per pixel (max score, first class that has it)      best [B, h, w, 2]
      "dfl"      DFL expectation + dist2bbox at `stride`, anchors at cell centres (misc_ref.decode_ref): (cx, cy, w, h) [B, h*w, 4];
                 aux["dfl_bound"] is misc_ref's bound of an fp32 decode of the same logits, aux["logits"] the logits."""
    p1 = conv(x, q_w(w1), _b(b1), 3, 1, acc)
    m1 = q_act(silu(p1))
    logits = conv(m1, q_w(w2), _b(b2), 1, 1, acc)
    aux = dict(pre=[p1, logits], mid=[m1], logits=logits)
    if mode == "raw":
        return logits, aux
    if mode == "sigmoid":
        s = torch.sigmoid(logits)
        mx, arg = s.max(1)                      # torch: the first of equal maxima
        first = (s == mx[:, None]).to(torch.float64).argmax(1)
        aux["best"] = torch.stack((mx, first.to(torch.float64)), -1)
        return s, aux
    if mode == "dfl":
        B, c2, h, w = logits.shape
        assert c2 == 64 and stride
        box = logits.permute(0, 2, 3, 1).reshape(B, h * w, 64).numpy()
        none = np.zeros((B, h * w, 0))
        pred, E, bound = misc_ref.decode_ref([box], [none], [none], [(h, w)], [stride])
        aux["dfl_bound"] = torch.from_numpy(bound)
        return torch.from_numpy(pred[..., :4]), aux
    raise ValueError(mode)


def proto_fold(x, wu, bu, wv, bv, w3, b3, q_act, q_w, acc=torch.float64):
    """The proto branch behind proto.cv1 as the three convs it is: ConvTranspose2d(2, 2) -> q -> 3x3 SiLU -> q -> 1x1 SiLU.  NOT
    the fold: convfold_kernel composes the ConvTranspose into the 3x3 (weights.cpp: pack_conv_fold) and never forms U; it rounds
    the composed weights once where this statement rounds wu, wv and U (test_gpu_fused_ops.py derives that difference)."""
    u = q_act(deconv(x, q_w(wu), _b(bu), acc))
    p2 = conv(u, q_w(wv), _b(bv), 3, 1, acc)
    m2 = q_act(silu(p2))
    p3 = conv(m2, q_w(w3), _b(b3), 1, 1, acc)
    return silu(p3), dict(pre=[u, p2, p3], mid=[u, m2])


def up_concat_1x1(a, b, w, bias, q_act, q_w, acc=torch.float64):
    """conv1_pk with up_src: nearest 2x of `a` (half the size), concat [up(a) | b], 1x1 SiLU."""
    x = torch.cat((F.interpolate(a, scale_factor=2, mode="nearest"), b), 1)
    p = conv(x, q_w(w), _b(bias), 1, 1, acc)
    return silu(p), dict(pre=[p], mid=[], x=x)
