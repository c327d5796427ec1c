"""Pins which kernels the planner picks on the two canvases of test_gpu_forward_ragged.py, and that their tiles are clipped there
(host only: vti_create touches no GPU).  Those GPU tests are only worth their time while these canvases reach the stem, bottleneck,
fold, tower and conv1_pk kernels with partial tiles; a planner change that moves them elsewhere must show up here.

  A  224x352: maps 56x88, 28x44, 14x22, 7x11 -- every tile of every fused / persistent kernel is clipped
  B  608x736: maps 152x184, 76x92, 38x46, 19x23 -- about the smallest canvas whose DEFAULT plan has conv1_pk and both Upsample folds"""
import pytest

from gpu_util import PLAIN_PLAN, plan_env

CASES = [   # H, W, dtype, max_batch
    (224, 352, "h2", 3), (224, 352, "h2", 64), (224, 352, "fp16", 3), (224, 352, "fp16", 64), (224, 352, "fp32", 3),
    (608, 736, "h2", 1), (608, 736, "fp16", 1),
]
LAUNCHES = {"h2": 64, "fp16": 61, "fp32": 66}       # default plan without the two Upsample+Concat folds


def plan(vti_amd, monkeypatch, H, W, dtype, max_batch, env):
    plan_env(monkeypatch, env)
    eng = vti_amd.Engine("n", 80, H=H, W=W, max_batch=max_batch, dtype=dtype)
    table = eng.conv_table()
    assert len(table) == 76
    return eng, {t["name"]: t for t in table}


def conv1_pk(t):
    return t["k"] == 1 and t["persistent"] and not t["fused"]


@pytest.mark.parametrize("H,W,dtype,max_batch", CASES, ids=lambda v: str(v))
def test_ragged_canvases_reach_the_fused_kernels(lib_built, monkeypatch, H, W, dtype, max_batch):
    eng, t = plan(lib_built, monkeypatch, H, W, dtype, max_batch, {})
    assert eng.num_anchors == (1617 if H == 224 else 9177)
    # stem_l1_kernel: layer 1 and its fused stage 2 on 8x40 tiles, clipped at the right edge
    for name in ("model.1", "model.2.cv1"):
        r = t[name]
        assert r["fused"] and r["tile"] == (8, 40) and (r["h_out"], r["w_out"]) == (H // 4, W // 4) and r["w_out"] % 40 != 0, r
    # bneck_pk: model.2.m.0 (+ the C2f's closing 1x1 as its tail with h2 / fp16 storage) on 8x20 tiles, 16x20 at a large batch
    bt = (16, 20) if max_batch == 64 else (8, 20)
    tail = ("model.2.cv2",) if dtype != "fp32" else ()
    for name in ("model.2.m.0.cv1", "model.2.m.0.cv2") + tail:
        r = t[name]
        assert r["persistent"] and r["tile"] == bt and r["fused"] == (name != "model.2.m.0.cv1"), r
        assert r["h_out"] % 16 != 0 and r["w_out"] % 20 != 0, r
    if dtype == "fp32":
        assert conv1_pk(t["model.2.cv2"])       # no tail in fp32: a conv1_pk of its own
    # fp16: 32 channels fit one K chunk, so the bottlenecks of model.4 and model.15 are bneck_pk pairs on the P3 map
    for name in ("model.4.m.0.cv2", "model.4.m.1.cv2", "model.15.m.0.cv2"):
        r = t[name]
        assert r["persistent"] and r["fused"] == (dtype == "fp16"), r
        if dtype == "fp16":
            assert r["tile"] == bt and (r["h_out"], r["w_out"]) == (H // 8, W // 8) and r["h_out"] % bt[0] != 0 and r["w_out"] % 20 != 0, r
    # convfold_kernel: the ConvTranspose's row carries the fold's tile (in low-resolution pixels); persistent in fp16 only
    up, cv2, cv3 = (t["model.22.proto." + n] for n in ("upsample", "cv2", "cv3"))
    assert up["tile"] == cv2["tile"] == cv3["tile"] == ((8, 20) if dtype == "h2" else (4, 20)) and cv3["fused"] and not up["fused"] and not cv2["fused"]
    assert up["persistent"] == cv2["persistent"] == (dtype == "fp16")
    assert up["w_in"] % 20 != 0 and (up["h_in"] % 8 != 0 or dtype != "h2"), up        # clipped at the right edge; h2's 8-row tiles at the bottom too
    # head towers: every last 1x1 runs in its 3x3's kernel
    for tower in ("cv2", "cv3", "cv4"):
        for lvl in range(3):
            r, prod = t[f"model.22.{tower}.{lvl}.2"], t[f"model.22.{tower}.{lvl}.1"]
            assert r["fused"] and not prod["fused"] and r["tile"] == prod["tile"], r
    if dtype == "h2":       # persistent box towers (16x20 tiles on canvas A) on the ragged P3 / P4 maps
        for lvl in (0, 1):
            r = t[f"model.22.cv2.{lvl}.1"]
            assert r["persistent"] and r["tile"][1] == 20 and r["h_out"] % r["tile"][0] != 0 and r["w_out"] % 20 != 0, r
            assert r["tile"] == (16, 20) or H != 224, r
    # 3x3 persistent kernels on ragged P3 / P4 maps
    r = t["model.3"]
    assert r["persistent"] and r["h_out"] % r["tile"][0] == 0 and r["w_out"] % r["tile"][1] != 0, r
    # launches, and the two Upsample+Concat folds (they need their consumer on conv1_pk)
    pk1 = [n for n, r in t.items() if conv1_pk(r)]
    if H == 224:
        assert pk1 == (["model.2.cv2"] if dtype == "fp32" else []), pk1     # maps below 1600 px stay on the per-tile kernel
        assert eng.num_launches == LAUNCHES[dtype]
        eng1, t1 = plan(lib_built, monkeypatch, H, W, dtype, max_batch, {"VTI_PK1_ALL": "1"})
        assert eng1.num_launches == LAUNCHES[dtype] - 2
        for name in ("model.12.cv1", "model.15.cv1", "model.9.cv2", "model.21.cv1"):
            assert conv1_pk(t1[name]), t1[name]
        for name in ("model.12.cv1", "model.15.cv1"):          # 160-pixel linear tiles over rows of 22 / 44
            r = t1[name]
            assert r["tile"][1] == 80 and (r["tile"][0] * 80) % r["w_out"] != 0 and (max_batch * r["h_out"] * r["w_out"]) % (r["tile"][0] * 80) != 0, r
    else:
        for name in ("model.12.cv1", "model.15.cv1"):
            r = t[name]
            assert conv1_pk(r) and r["tile"][1] == 80 and (r["tile"][0] * 80) % r["w_out"] != 0 and (r["h_out"] * r["w_out"]) % (r["tile"][0] * 80) != 0, r
        assert eng.num_launches == LAUNCHES[dtype] - 2
        eng0, _ = plan(lib_built, monkeypatch, H, W, dtype, max_batch, {"VTI_NO_UPFUSE": "1"})
        assert eng0.num_launches == LAUNCHES[dtype]


@pytest.mark.parametrize("H,W,dtype,max_batch", CASES, ids=lambda v: str(v))
def test_plain_plan_has_no_fusion(lib_built, monkeypatch, H, W, dtype, max_batch):
    """Every fusion switch set: 80 launches, nothing fused, nothing persistent --
    the plan the GPU test uses to tell a fusion's error from a base kernel's."""
    eng, t = plan(lib_built, monkeypatch, H, W, dtype, max_batch, PLAIN_PLAN)
    assert not [n for n, r in t.items() if r["fused"] or r["persistent"]]
    assert eng.num_launches == 80
