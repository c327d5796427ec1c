"""The whole h2 forward on weights with a wide range, layer by layer AND channel by channel.

Every other layerwise test draws He-scaled weights: within a conv all channels are alike and the per-conv weight scale SW of the
h2 packers (weights.cpp: pack_conv, pack_conv_stage2, pack_convfold, pack_stem_toeplitz, pack_conv_l1pairs, the jointly scaled
tail of model.2, the plain chunk packing) meets one kind of tensor.  Here (recipe below, seeded, generated -- nothing committed):
every conv of the seeded blob gets per-output-channel factors 2^u, u in -6..2, and per-input-channel factors 2^v, v in -3..3, then
ONE scalar per conv from a single calibrating pass of the CPU oracle that brings the conv's pre-activation to standard deviation
1 on the test frames.  Packed weights span ~2^11 within a conv, SW differs widely between convs, activations stay in range.

Canvas 320x320: the smallest whose DEFAULT n-scale plan has every kernel family (k, s, kind, fused, persistent) of the 640x640
plan -- below 1600 pixels on the P3 map the unfused 1x1 convs leave the persistent kernel (128x160 and 224x352 lack it);
asserted on the host.

Checks for B = 2 frames: check_conv_rows / check_pred_proto with the unchanged h2 bounds against the fp32 oracle, and per channel
    E = max |engine - fp64 oracle|                                     (per channel of every materialised conv output)
    R = max |h2-emulating oracle - fp64 oracle| + max |fp32 oracle - fp64 oracle|     (the references alone: storage + fp32)
    E <= 3 R + one h2 unit in the last place at the channel's maximum.
R itself is checked first: finite, and below the per-layer bound for every channel.

Measured (MI355X), 52 materialised rows: the largest excess of E over that unit is 2.43 R, at model.21.cv2 channel 38 (E 4.07e-5,
R 1.64e-5 at a channel maximum of 2.30; a 10x10 map, so R is the maximum of 200 samples), then 2.21 R at model.21.cv1 and
1.72 R at model.21.m.0.cv2; every row above the P5 neck stays below 1.4 R and the backbone below 1.05 R.  R alone is at most
1.5e-5 of a layer's maximum (bound 4e-5).
"""
import functools

import numpy as np
import pytest
import torch

import h2_ref
from gpu_util import LAYER_TOL, check_conv_rows, check_pred_proto, frames_u8, h2_oracle, need_gpu, plan_families, plan_env

pytestmark = pytest.mark.gpu

NC, HW, B, SEED, CAP = 80, (320, 320), 2, 5, 3.0


@functools.lru_cache(maxsize=None)
def frames():
    return frames_u8(B, *HW, seed=3)        # shared: nobody writes to it


@functools.lru_cache(maxsize=None)
def wide_blob():
    import vti_amd
    from oracle.model import OracleModel
    plan = vti_amd.Engine("n", NC, H=HW[0], W=HW[1], max_batch=1)
    meta, table, tensors = vti_amd.unpack_container(vti_amd.random_weights(plan, seed=1, gain=1.7))
    rng = np.random.default_rng(SEED)
    wide = {}
    for t in table:
        w, b = tensors[t["name"]]
        fo = (2.0 ** rng.integers(-6, 3, t["c2"])).astype(np.float32)
        fi = (2.0 ** rng.integers(-3, 4, t["c1"])).astype(np.float32)
        sh_o, sh_i = ((1, -1, 1, 1), (-1, 1, 1, 1)) if t["kind"] == 2 else ((-1, 1, 1, 1), (1, -1, 1, 1))
        wide[t["name"]] = (w * fo.reshape(sh_o) * fi.reshape(sh_i), b * fo)
    pack = lambda tensors: vti_amd.pack_container(meta["scale"], meta["nc"], meta["nm"], meta["reg_max"], plan.conv_table(), tensors)

    class Calibrating(OracleModel):
        """One pass: each conv is rescaled, as it is reached, by the scalar that gives its pre-activation standard deviation 1."""

        def conv(self, x, name, res=None, out_fp32=False):
            w, b, k, s, kind = self.p[name]
            z = torch.nn.functional.conv_transpose2d(x, w, b, stride=s) if kind == 2 else torch.nn.functional.conv2d(x, w, b, stride=s, padding=k // 2)
            g = np.float32(1.0 / float(z.std()))
            self.p[name] = (w * g, b * g, k, s, kind)
            return super().conv(x, name, res, out_fp32)

    om = Calibrating(pack(wide), *HW, mode="fp32")
    om.forward_u8(frames(), swap_rb=True)
    return pack({n: (w.numpy(), b.numpy()) for n, (w, b, _, _, _) in om.p.items()})


@functools.lru_cache(maxsize=None)
def references():
    """taps of the fp32, fp64 and h2-emulating oracles (+ the fp32 oracle's pred / proto); computed once, never written to."""
    from oracle.model import OracleModel
    out = {}
    for mode in ("fp32", "fp64", "h2"):
        om = h2_oracle(wide_blob(), *HW) if mode == "h2" else OracleModel(wide_blob(), *HW, mode=mode)
        pred, proto = om.forward_u8(frames(), swap_rb=True, record=True)
        out[mode] = (pred, proto, om.taps)
    return out


def channel_maxima(t):
    return t.abs().amax((0, 2, 3)).double().numpy()


def reference_error(name):
    """(R, the fp64 tap's per-channel maximum) for conv `name`."""
    ref = references()
    t64 = ref["fp64"][2][name]
    return channel_maxima(ref["h2"][2][name].double() - t64) + channel_maxima(ref["fp32"][2][name].double() - t64), channel_maxima(t64)


def test_wide_weights_forward_per_channel(monkeypatch):
    need_gpu()
    import vti_amd
    plan_env(monkeypatch, {})
    table640 = vti_amd.Engine("n", NC, H=640, W=640, max_batch=B, dtype="h2").conv_table()
    eng = vti_amd.Engine("n", NC, H=HW[0], W=HW[1], max_batch=B, dtype="h2")
    table = eng.conv_table()
    assert plan_families(table) >= plan_families(table640), plan_families(table640) - plan_families(table)

    # the blob is what the recipe promises, and the references alone stay inside what is asserted below
    _, _, tensors = vti_amd.unpack_container(wide_blob())
    spans = [np.log2(np.abs(w).max() / np.abs(w).reshape(w.shape[0], -1).max(1).min()) for w, _ in tensors.values()]
    sws = [h2_ref.enc_w(w)[2] for w, _ in tensors.values()]
    assert min(spans) >= 6 and max(sws) / min(sws) >= 2 ** 4, (min(spans), max(sws) / min(sws))      # here: 2^6.6 .. 2^9.8 within a conv (channel maxima), SW over 2^5
    ref = references()
    tol = LAYER_TOL["h2"]
    for t in table:
        tap = ref["fp32"][2][t["name"]]
        assert torch.isfinite(tap).all() and 0.05 < float(tap.std()) < 20 and float(tap.abs().max()) < 4094, t["name"]
        R, cmax = reference_error(t["name"])
        assert np.isfinite(R).all() and (R <= tol * max(cmax.max(), 1.0)).all(), (t["name"], R.max(), cmax.max())

    eng.load_weights(wide_blob(), 0)
    pred, proto = eng.forward(torch.from_numpy(frames()).cuda(), swap_rb=True)
    torch.cuda.synchronize()
    opred, oproto, taps = ref["fp32"]
    checked, _, _ = check_conv_rows(eng, taps, B, "h2", tol)
    assert checked >= len(table) - 28
    check_pred_proto(pred, proto, opred, oproto, taps, "h2", tol, NC, *HW)

    worst, failures, rows = (0.0, None, None), [], 0
    for i, t in enumerate(table):
        try:
            got = eng.debug_conv_output(i, B).cpu().double()
        except vti_amd.VtiError:
            continue        # lives in registers or in pred only: check_conv_rows names which rows may
        rows += 1
        E = channel_maxima(got - ref["fp64"][2][t["name"]])
        R, cmax = reference_error(t["name"])
        unit = cmax * 2.0 ** -23 if t["kind"] == 1 else h2_ref.unit(cmax)      # kind 1: the heads' last convs, kept in fp32
        ratio = np.maximum(E - unit, 0) / np.maximum(R, 1e-300)
        c = int(np.argmax(ratio))
        print(f"h2wide {i:2d} {t['name']:26s} worst channel {c:3d}: E {E[c]:.3e} R {R[c]:.3e} unit {unit[c]:.3e} max {cmax[c]:.3e} (layer {cmax.max():.3e})  (E - unit)/R {ratio[c]:.3f}")
        if ratio[c] > worst[0]:
            worst = (float(ratio[c]), t["name"], c)
        if not (E <= CAP * R + unit).all():
            failures.append(f"{t['name']} channel {c}: E {E[c]:.3e} > 3 * {R[c]:.3e} + {unit[c]:.3e}")
    print(f"h2wide {rows} rows: largest (E - unit)/R {worst[0]:.3f} at {worst[1]} channel {worst[2]}")
    assert rows == checked and not failures, failures
