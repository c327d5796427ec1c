"""Shared helpers for the -m gpu parity tests (all call through the C ABI via vti_amd)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F


def need_gpu():
    import pytest
    if not torch.cuda.is_available():
        pytest.skip("no GPU in this container (run with gpurun)")


@functools.lru_cache(maxsize=8)
def engine_and_oracle(scale, nc, H, W, B, dtype, seed=1, cls_bias=None, gain=1.7):
    import vti_amd
    from oracle.model import OracleModel
    eng = vti_amd.Engine(scale, nc, H=H, W=W, max_batch=B, dtype=dtype)
    blob = vti_amd.random_weights(eng, seed=seed, cls_bias=cls_bias, gain=gain)
    eng.load_weights(blob, 0)
    # the h2 engine (split-fp16 pairs, ~22 bits) is held against the plain fp32 oracle
    return eng, OracleModel(blob, H, W, mode="fp32" if dtype == "h2" else dtype), blob


# planner switches: set them all and no conv is fused or persistent.  Every VTI_* switch, planner and launch path alike, is read
# once when a context is created (vti_create; per call for vti_debug_conv2d) and kept in it: a change made afterwards reaches the
# next engine, never a forward of an existing one, and no switch is frozen at the first plan of the process any more.
PLAIN_SWITCHES = ("VTI_NO_FUSE", "VTI_NO_FOLD", "VTI_NO_BNECK", "VTI_NO_STEM_FUSE", "VTI_NO_UPFUSE", "VTI_NO_PK", "VTI_NO_PK1", "VTI_NO_PK2")
PLAIN_PLAN = {k: "1" for k in PLAIN_SWITCHES}


def plan_env(monkeypatch, env):
    """Exactly the planner switches in `env` for the engines created from here on (cleared again when the test ends)."""
    for k in PLAIN_SWITCHES + ("VTI_PK1_ALL",):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def frames_u8(B, H, W, seed=0):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, (B, H, W, 3), dtype=np.uint8)


LAYER_TOL = {"h2": 4e-5, "fp32": 2e-5, "fp16": 6e-3}      # per-layer bound, relative to max(|ref|.max(), 1): see test_gpu_forward.py
SIG_BITS = {"h2": 22, "fp32": 24, "fp16": 11}              # significant bits of the engine's activation storage


def storage_ulp(dtype, vmax):
    """One unit in the last place of the engine's storage type at magnitude `vmax`."""
    import math
    return 2.0 ** (math.floor(math.log2(max(vmax, 2.0 ** -14))) - (SIG_BITS[dtype] - 1))


def h2_oracle(blob, H, W):
    """The fp32 oracle with the h2 storage's rounding (tests/h2_ref.py) where the h2 engine rounds: every conv's weights as one
    (wh + wl) / SW per conv, the input and every stored conv output as a saturating (hi + lo) / 16 pair."""
    import h2_ref
    from oracle.model import OracleModel

    class H2Oracle(OracleModel):
        def __init__(self, blob, H, W):
            super().__init__(blob, H, W, "fp32")
            for name, (w, b, k, s, kind) in list(self.p.items()):
                self.p[name] = (torch.from_numpy(h2_ref.q_w(w.numpy())).float(), b, k, s, kind)

        def q(self, t):
            return torch.from_numpy(h2_ref.q_act(t.numpy())).float()

    return H2Oracle(blob, H, W)


def plan_families(table):
    """The kernel families of a plan: (k, s, kind, fused, persistent) of its conv-table rows."""
    return {(t["k"], t["s"], t["kind"], bool(t["fused"]), bool(t["persistent"])) for t in table}


def clipped_mask(t, B, folded=False, n=None):
    """bool [n, h, w] (the first n of the B frames that ran; default all): the output pixels of conv-table row `t` that the kernel computes in a tile clipped by the map's edge, or
    None where the map divides into whole tiles (or where every pixel sits in a clipped tile, so there is nothing to compare with).
      * conv1_pk (an unfused persistent 1x1) walks tiles of tile_h * tile_w consecutive pixels of the flattened [B*h*w] index
        space: its only clipped tile holds the batch's trailing (B*h*w) % (tile_h*tile_w) pixels;
      * every other row: the last h % tile_h rows and the last w % tile_w columns, on the tile of the kernel that produced the
        row (a fused row carries its producer's tile); `folded` marks proto.cv2 / proto.cv3 behind the folded ConvTranspose,
        whose kernel tiles the low-resolution map, so that its output tile is twice the table's in both directions.
    A direction in which a single tile spans the map is left out: it has no whole tile to compare with."""
    h, w = t["h_out"], t["w_out"]
    th, tw = t["tile"]
    m = torch.zeros((B, h, w), dtype=torch.bool)
    if t["k"] == 1 and t["persistent"] and not t["fused"]:
        r = (B * h * w) % (th * tw)
        m.view(-1)[B * h * w - r:] = r > 0
        m = m[:n]
        return m if m.any() and not m.all() else None
    if folded:
        th, tw = 2 * th, 2 * tw
    rh = h % th if h > th else 0
    rw = w % tw if w > tw else 0
    if rh == 0 and rw == 0:
        return None
    if rh:
        m[:, h - rh:, :] = True
    if rw:
        m[:, :, w - rw:] = True
    return m[:n]


def check_conv_rows(eng, taps, B, dtype, tol, band=None, report=None, B_run=None):
    """The per-row loop of the layer-by-layer parity tests: every conv output the plan materialises, read back through
    debug_conv_output, must lie within `tol` * max(|ref|.max(), 1) of the oracle's tap; a row that cannot be read must be one the
    plan is known to keep out of memory.  With `band` (a factor), every row whose map is ragged against its tile must also keep the
    maximum error on its clipped tiles within `band` times the maximum error on the rest of the same map (floor: one unit in the
    last place of the storage type at the layer's maximum).  Returns (rows checked, largest band ratio seen, its row's name);
    `report`, if given, is called with one line per row; `B_run` is the batch of the last forward where only its first B frames
    are checked."""
    import pytest
    import vti_amd
    table = eng.conv_table()
    checked, worst, worst_name, folded = 0, 0.0, None, False
    for i, t in enumerate(table):
        if i + 1 < len(table) and table[i + 1]["fused"]:
            # this row's output feeds a conv fused into its kernel and never reaches memory;
            # it is verified through that conv's output (next row)
            with pytest.raises(vti_amd.VtiError):
                eng.debug_conv_output(i, B)
            continue
        try:
            got = eng.debug_conv_output(i, B).cpu()
        except vti_amd.VtiError:
            # class / coefficient towers whose fused 1x1 writes straight into pred, and (fp16 / h2 engine) box towers whose fused
            # 1x1 stage also does DFL + dist2bbox: checked via pred
            # ... and proto.upsample when the plan folded it into proto.cv2 (four 2x2 convs on the low-resolution map): checked
            # through proto.cv3's output
            # ... and the second 3x3 of a bottleneck whose C2f's closing 1x1 runs in the same kernel (y2 stays in registers)
            assert (t["fused"] and (".cv3." in t["name"] or ".cv4." in t["name"] or ".m." in t["name"] or (dtype != "fp32" and ".cv2." in t["name"]))) or \
                   t["name"] == "model.22.proto.upsample", t["name"]
            folded = folded or t["name"] == "model.22.proto.upsample"
            continue
        checked += 1
        ref = taps[t["name"]]
        assert got.shape == ref.shape and torch.isfinite(ref).all(), t["name"]
        d = (got - ref).abs()
        err, rmax = d.max().item(), ref.abs().max().item()
        line = f"{i:2d} {t['name']:26s} {t['h_out']}x{t['w_out']} tile={t['tile']} max|d|={err:.3e} ref max={rmax:.3e} rel={err / max(rmax, 1.0):.2e}"
        if band is not None:
            m = clipped_mask(t, B_run or B, folded and t["name"].startswith("model.22.proto.cv"), B)
            if m is not None:
                dm = d.amax(1)          # [B, h, w]: worst channel per pixel
                e_band, e_in, floor = dm[m].max().item(), dm[~m].max().item(), storage_ulp("fp32" if t["kind"] == 1 else dtype, rmax)     # kind 1: the heads' last convs, kept in fp32
                ratio = e_band / max(e_in, floor / band)
                line += f" band={e_band:.3e} interior={e_in:.3e} floor={floor:.2e} ratio={ratio:.2f}"
                if ratio > worst:
                    worst, worst_name = ratio, t["name"]
                if report:
                    report(line)
                assert e_band <= max(band * e_in, floor), f"{t['name']}: clipped tiles max|d|={e_band:.3e} vs interior {e_in:.3e} (x{e_band / max(e_in, 1e-30):.1f}), floor {floor:.2e}"
                line = None
        if report and line:
            report(line)
        assert err <= tol * max(rmax, 1.0), f"{t['name']}: max|d|={err:.3e} ref max={rmax:.3e}"
    return checked, worst, worst_name


def check_pred_proto(pred, proto, opred, oproto, taps, dtype, tol, nc, H, W):
    """The n-scale pred / proto bounds of the layer-by-layer parity tests (pred, proto: the engine's, on any device; opred, oproto:
    the reference's, which may be the oracle's or another plan's output brought to the oracle's layout)."""
    assert pred.shape == opred.shape and torch.isfinite(pred).all()
    e = (pred.cpu() - opred).abs()
    # scores: |d sigmoid| <= |d logit| / 4 and |d logit| <= tol * max|logit| (per-layer bound)
    logit_max = max(taps[f"model.22.cv3.{l}.2"].abs().max().item() for l in range(3))
    exact = dtype in ("fp32", "h2")
    cls_tol = max(1e-4 if exact else 2e-2, tol * logit_max)
    box_px, mc_tol = ((5e-3 if dtype == "fp32" else 2e-2), 1e-3) if exact else (4.0, 0.01 * opred[:, 4 + nc:].abs().max().item() + 0.2)
    assert e[:, 4:4 + nc].max() < cls_tol
    assert e[:, :4].max() < box_px and e[:, :4].max() / max(H, W) < (1e-3 if exact else 1e-2)
    assert e[:, 4 + nc:].max() < mc_tol
    pe = (proto.float().cpu().permute(0, 3, 1, 2) - oproto).abs().max().item()
    assert pe < (1e-3 if exact else 0.1)


def ref_conv(x_nhwc, w, b, k, s, kind, dtype, res=None, act=None):
    """torch-CPU reference of one engine conv on NHWC float input; fp16 mode rounds operands and result."""
    q = (lambda t: t.half().float()) if dtype == "fp16" else (lambda t: t)      # fp32 and h2: no operand rounding
    x = q(torch.as_tensor(x_nhwc).float()).permute(0, 3, 1, 2)
    w = q(torch.as_tensor(w).float())
    b = torch.as_tensor(b).float()
    if kind == 2:
        y = F.conv_transpose2d(x.double(), w.double(), b.double(), stride=s).float()
    else:
        y = F.conv2d(x.double(), w.double(), b.double(), stride=s, padding=k // 2).float()
    if kind == 0 if act is None else act:
        y = F.silu(y)
    if res is not None:
        y = y + q(torch.as_tensor(res).float()).permute(0, 3, 1, 2)
    return y.permute(0, 2, 3, 1).contiguous()


def mask_iou(a, b):
    a = np.asarray(a) > 0
    b = np.asarray(b) > 0
    u = np.logical_or(a, b).sum()
    return 1.0 if u == 0 else np.logical_and(a, b).sum() / u


def synth_pred(rng, B, nc, nm, A, H=640, W=640, n_inst=50, dup=5, bg=0.05):
    """SURVEY section 8d post-processing stress: `n_inst` planted, well separated boxes per frame (conf in
    [0.5,0.9]) x `dup` jittered duplicates each (IoU > 0.7) + background scores below conf."""
    pred = np.zeros((B, 4 + nc + nm, A), np.float32)
    pred[:, 4:4 + nc] = rng.uniform(0, bg, (B, nc, A)).astype(np.float32)
    pred[:, 0] = rng.uniform(0, W, (B, A))
    pred[:, 1] = rng.uniform(0, H, (B, A))
    pred[:, 2:4] = rng.uniform(8, 80, (B, 2, A))
    pred[:, 4 + nc:] = rng.standard_normal((B, nm, A)).astype(np.float32)
    g = int(np.ceil(np.sqrt(n_inst)))
    for b in range(B):
        slots = rng.choice(A, n_inst * dup, replace=False)
        for i in range(n_inst):
            cx = (i % g + 0.5) * W / g + rng.uniform(-3, 3)
            cy = (i // g + 0.5) * H / g + rng.uniform(-3, 3)
            w, h = rng.uniform(0.45, 0.8, 2) * np.array([W / g, H / g])
            c = int(rng.integers(nc))
            for d in range(dup):
                a = slots[i * dup + d]
                pred[b, :4, a] = [cx + rng.normal(0, 0.5), cy + rng.normal(0, 0.5), w + rng.normal(0, 0.5), h + rng.normal(0, 0.5)]
                pred[b, 4:4 + nc, a] = rng.uniform(0, bg, nc)
                pred[b, 4 + c, a] = rng.uniform(0.5, 0.9)
    return pred
