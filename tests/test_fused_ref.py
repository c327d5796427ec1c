"""tests/fused_ref.py against oracle/model.py on one small canvas (n scale, 64x96, 2 frames, the seeded blob): every function, fed
the oracle's own tap as its input and the blob's tensors as its weights, must reproduce the taps of the convs it states --
EQUAL in float64 (the same ATen ops in the same order), and in float32 within the fp32 noise floor of those convs, measured here
as |fp32 oracle - fp64 oracle| on the same taps.  With the fp16 hooks it must agree with the fp16-mode oracle, which rounds at
the same points, up to the roundings that the oracle's float32 SiLU flips."""
import numpy as np
import pytest
import torch

import fused_ref
from gpu_util import frames_u8

H, W, B = 64, 96, 2


@pytest.fixture(scope="module")
def world(lib_built):
    vti_amd = lib_built
    from oracle.model import OracleModel
    eng = vti_amd.Engine("n", 80, H=H, W=W, max_batch=B, dtype="fp32")
    blob = vti_amd.random_weights(eng, seed=1, cls_bias=-2.0)
    tensors = vti_amd.unpack_container(blob)[2]
    fr = frames_u8(B, H, W, seed=5)
    out = {}
    for mode in ("fp64", "fp32", "fp16"):
        om = OracleModel(blob, H, W, mode=mode)
        pred, proto = om.forward_u8(fr, swap_rb=True, record=True)
        out[mode] = ({k: v.double() for k, v in om.taps.items()}, pred.double())
    return tensors, fr, out


def _cases(tensors, fr, taps, pred, q_act, q_w, acc):
    """-> {name: (got, want)} of every function on the taps of one oracle mode."""
    t = lambda n: tensors[n]
    res = {}
    res["stem_l1"] = (fused_ref.stem_l1(fr, True, *t("model.0"), *t("model.1"), *t("model.2.cv1"), q_act, q_w, acc)[0], taps["model.2.cv1"])
    y0, y1 = taps["model.2.cv1"].chunk(2, 1)
    args = (y1, *t("model.2.m.0.cv1"), *t("model.2.m.0.cv2"), True, q_act, q_w, acc)
    res["bneck"] = (q_act(fused_ref.bneck(*args)[0]), taps["model.2.m.0.cv2"])
    res["bneck_tail"] = (fused_ref.bneck(*args, tail=(y0, *t("model.2.cv2")))[0], taps["model.2.cv2"])
    x15 = taps["model.15.cv1"].chunk(2, 1)[1]
    res["bneck_plain"] = (q_act(fused_ref.bneck(x15, *t("model.15.m.0.cv1"), *t("model.15.m.0.cv2"), False, q_act, q_w, acc)[0]), taps["model.15.m.0.cv2"])
    p3 = {tw: taps[f"model.22.{tw}.0.0"] for tw in ("cv2", "cv3", "cv4")}      # the towers' first convs feed the fused (3x3, 1x1) ops
    hw = p3["cv2"].shape[2] * p3["cv2"].shape[3]
    res["tower_raw"] = (fused_ref.tower(p3["cv4"], *t("model.22.cv4.0.1"), *t("model.22.cv4.0.2"), "raw", q_act, q_w, acc)[0], taps["model.22.cv4.0.2"])
    s, aux = fused_ref.tower(p3["cv3"], *t("model.22.cv3.0.1"), *t("model.22.cv3.0.2"), "sigmoid", q_act, q_w, acc)
    res["tower_sigmoid"] = (s.reshape(B, 80, hw), pred[:, 4:84, :hw])
    res["tower_best"] = (aux["best"][..., 0].reshape(B, hw), pred[:, 4:84, :hw].max(1)[0])
    box, aux = fused_ref.tower(p3["cv2"], *t("model.22.cv2.0.1"), *t("model.22.cv2.0.2"), "dfl", q_act, q_w, acc, stride=8)
    res["tower_dfl_logits"] = (aux["logits"], taps["model.22.cv2.0.2"])
    res["tower_dfl"] = (box.permute(0, 2, 1), pred[:, :4, :hw])
    res["proto_fold"] = (fused_ref.proto_fold(taps["model.22.proto.cv1"], *t("model.22.proto.upsample"), *t("model.22.proto.cv2"), *t("model.22.proto.cv3"),
                                              q_act, q_w, acc)[0], taps["model.22.proto.cv3"])
    res["up_concat_1x1"] = (fused_ref.up_concat_1x1(taps["model.9.cv2"], taps["model.6.cv2"], *t("model.12.cv1"), q_act, q_w, acc)[0], taps["model.12.cv1"])
    return res


def test_float64_equals_the_oracle(world):
    tensors, fr, out = world
    taps, pred = out["fp64"]
    ident, q_w = fused_ref.hooks("fp32")
    for name, (got, want) in _cases(tensors, fr, taps, pred, ident, q_w, torch.float64).items():
        if name == "tower_dfl":      # the oracle's decode goes through float32 anchors and another softmax: not the same ops
            assert (got - want).abs().max() < 1e-9, name
        else:
            assert want is not None and got.shape == want.shape and torch.equal(got, want), (name, (got - want).abs().max())


def test_float32_stays_within_the_fp32_noise_floor(world):
    """acc=float32 evaluates the same convs as the fp32 oracle, on fp64 taps as inputs; the two differ by the inputs' and the
    activations' precision, i.e. by no more than the fp32 oracle differs from the fp64 one on the same tap, which is measured
    here, plus the references' own float32 error, measured too."""
    tensors, fr, out = world
    taps64, pred64 = out["fp64"]
    taps32, pred32 = out["fp32"]
    ident, q_w = fused_ref.hooks("fp32")
    r64 = _cases(tensors, fr, taps64, pred64, ident, q_w, torch.float64)
    r32 = _cases(tensors, fr, taps64, pred64, ident, q_w, torch.float32)
    o32 = _cases(tensors, fr, taps32, pred32, ident, q_w, torch.float32)
    for name in r64:
        own = (r32[name][0] - r64[name][0]).abs().max().item()
        floor = (o32[name][1] - r64[name][1]).abs().max().item()
        d = (r32[name][0] - o32[name][1]).abs().max().item()
        print(f"fused_ref {name:18s} |ref32 - ref64| {own:.3e}  |oracle32 - oracle64| {floor:.3e}  |ref32 - oracle32| {d:.3e}")
        assert own > 0 or name == "tower_best" or floor == 0, name          # the float32 evaluation is a different one
        assert d <= own + floor and own <= 4 * floor + 1e-12, (name, d, own, floor)


def test_fp16_hooks_round_where_the_fp16_oracle_rounds(world):
    tensors, fr, out = world
    taps, pred = out["fp16"]
    q_act, q_w = fused_ref.hooks("fp16")
    for name, (got, want) in _cases(tensors, fr, taps, pred, q_act, q_w, torch.float32).items():
        if want is None or name.startswith("tower_") and name != "tower_raw" and name != "tower_dfl_logits":
            continue
        if not name.startswith("tower_"):
            got = q_act(got)            # the oracle's tap is the stored output
        # the oracle evaluates SiLU in float32, fused_ref in float64: a value next to a rounding boundary may land on the other side, and
        # what it feeds moves with it -- by one fp16 unit in the last place at the tensor's maximum, at a few places
        ulp = 2.0 ** (torch.floor(torch.log2(want.abs().max())) - 10)
        d = (got - want).abs()
        assert (d <= ulp).all() and (d > 0).double().mean() < 0.02, (name, d.max(), (d > 0).double().mean())


def test_h2_hooks_are_h2_ref():
    import h2_ref
    q_act, q_w = fused_ref.hooks("h2")
    rng = np.random.default_rng(0)
    v = rng.standard_normal((2, 3, 4, 5)) * 100
    w = rng.standard_normal((4, 3, 3, 3)).astype(np.float32)
    assert np.array_equal(q_act(torch.from_numpy(v)).numpy(), h2_ref.q_act(v)) and np.array_equal(q_w(w).numpy(), h2_ref.q_w(w))
    assert np.array_equal(q_act(torch.tensor([1e6, -1e6], dtype=torch.float64)).numpy(), [h2_ref.H2_MAX, -h2_ref.H2_MAX])
