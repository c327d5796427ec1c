"""stem_l1_kernel alone (vti_debug_run_op on model.1's op) at the geometries that decide how its waves share a tile, for h2 (one
8-wave workgroup per CU: waves 0-3 own three of the tile's twenty 16-pixel m-tiles, waves 4-7 two) and fp16 (two 4-wave
workgroups, five m-tiles per wave), against tests/fused_ref.py with test_gpu_fused_ops.py's bound (`check`, `_chain`: no new
constant).  Each case runs with swap_rb 0 and 1, with model.2.cv1 fused (conv_stage2 on the register tile) and with
VTI_NO_STEM_FUSE3=1 (layer 1 leaves through conv_epilogue and is compared as stored).

  case    frames          layer-1 map   tiles  what it covers
  tile    1 x 32x160      8x40          1      one full tile: every m-tile of every wave holds valid pixels
  clip    2 x 64x192      16x48         8      a second tile column of 8 pixels: m-tiles with 8 valid lanes and wholly invalid ones
  batch   13 x 224x352    56x88         273    more tiles than the 256 workgroups: 17 of them run the persistent loop and the
                                               next-tile prefetch twice; the third tile column is clipped to 8 pixels

`clip` stands where a 2 x 36x171 frame was asked for (a row clip, an odd width, a 3-pixel column, the byte-wise staging of rows
that are no whole dwords).  The engine plans canvases whose sides are multiples of 32 only (plan.cpp: derive_channels), so a
layer-1 map is always a multiple of 8 in both directions: its rows are never clipped by the 8-row tile, a clipped column is 8,
16, 24 or 32 pixels wide, a row of the frame is a whole number of dwords, and vti_debug_run_op cannot reach the kernel's
`aligned == false` staging at all.  64x192 is the smallest canvas with the narrowest clipped column the planner admits.

Untouched bytes: the engine is created one frame larger than the batch that runs; the op's output view is filled with SENTINEL
for all frames first (vti_debug_set_conv_output), and afterwards the spare frame (the memory right behind the last valid map,
where a tile row past the map's bottom would land) and, unfused, model.2.cv1's whole view must still hold it, and pred, proto
and best their byte pattern (test_gpu_fused_ops.py's poison).  Inside the map every value must have been replaced: SENTINEL is
far outside any bound.
"""
import functools

import numpy as np
import pytest
import torch

import fused_ref
from gpu_util import need_gpu, plan_env
from test_gpu_fused_ops import STEM, Op, _chain, base, bias, check, he, hooks, pattern_left

pytestmark = pytest.mark.gpu

NC = 80
CASES = {"tile": (1, 32, 160), "clip": (2, 64, 192), "batch": (13, 224, 352)}
SENTINEL = 1536.0       # exact in fp16 and h2; the op's outputs are SiLU values of magnitude ~1


@functools.lru_cache(maxsize=None)
def _engine(dtype, case, fuse3):
    import vti_amd
    B, H, W = CASES[case]
    return vti_amd.Engine("n", NC, H=H, W=W, max_batch=B + 1, dtype=dtype)


def engine(monkeypatch, dtype, case, fuse3):
    """Cached per (dtype, case, plan); the switch is read when the engine is created."""
    plan_env(monkeypatch, {})
    if fuse3:
        monkeypatch.delenv("VTI_NO_STEM_FUSE3", raising=False)
    else:
        monkeypatch.setenv("VTI_NO_STEM_FUSE3", "1")
    return _engine(dtype, case, fuse3)


@functools.lru_cache(maxsize=None)
def weights():
    rng = np.random.default_rng(70)
    return {STEM[0]: (he(rng, (16, 3, 3, 3)), bias(rng, 16)), STEM[1]: (he(rng, (32, 16, 3, 3)), bias(rng, 32)),
            STEM[2]: (he(rng, (32, 32, 1, 1)), bias(rng, 32))}


@functools.lru_cache(maxsize=None)
def frames(case):
    B, H, W = CASES[case]
    return np.random.default_rng(71).integers(0, 256, (B, H, W, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def reference(dtype, case, swap):
    """fused_ref.stem_l1 in float64 and float32, once per (dtype, case, swap) and shared by the fused and the unfused plan."""
    ws = weights()
    q_act, q_w = hooks(dtype)
    kw = {}
    if dtype == "h2":       # bytes as exact integers, the 1 / 255 inside the stem's weights (as test_gpu_fused_ops.stem_case)
        kw = dict(q_in=lambda x: x.double() / 255,
                  q_w0=lambda w: q_w((np.asarray(w, np.float64) / 255.0).astype(np.float32)) * 255.0)
    args = (frames(case), swap, *ws[STEM[0]], *ws[STEM[1]], *ws[STEM[2]], q_act, q_w)
    return fused_ref.stem_l1(*args, acc=torch.float64, **kw), fused_ref.stem_l1(*args, acc=torch.float32, **kw)


def load(eng):
    import vti_amd
    meta, table, tensors = base()
    t = dict(tensors)
    t.update(weights())
    eng.load_weights(vti_amd.pack_container(meta["scale"], meta["nc"], meta["nm"], meta["reg_max"], table, t), 0)


class StemOp(Op):
    """Op with pred / proto / best sized for this engine's canvas."""

    def run(self, B, x, swap):
        dev, (_, H, W) = self.eng.device, self.case
        fill = lambda *s: torch.full(s, 0xFF, dtype=torch.uint8, device=dev)
        na = self.eng.num_anchors
        self.pred = fill(B, na, (4 + NC + 32) * 4).view(torch.float32)
        self.best = fill(B, na, 2 * 4).view(torch.float32)
        self.proto = fill(B, H // 4, W // 4, 32 * (2 if self.eng.dtype == "fp16" else 4)).view(self.eng.torch_dtype)
        convs = self.eng.debug_run_op(self.i, B, x=x, swap_rb=swap, pred=self.pred, proto=self.proto, best=self.best)
        torch.cuda.synchronize()
        return [self.names[c] for c in convs]


@pytest.mark.parametrize("fuse3", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("swap", [False, True], ids=["rgb", "swap_rb"])
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("dtype", ["h2", "fp16"])
def test_stem_waves(dtype, case, swap, fuse3, monkeypatch):
    need_gpu()
    B, H, W = CASES[case]
    eng = engine(monkeypatch, dtype, case, fuse3)
    load(eng)
    op = StemOp(eng, "model.1")
    op.case = CASES[case]
    t0, t1, t2 = op.rows(*STEM)
    assert t1["fused"] and t1["tile"] == (8, 40) and bool(t2["fused"]) == fuse3 and (t1["h_out"], t1["w_out"]) == (H // 4, W // 4), (t0, t1, t2)
    ntiles = B * (-(-t1["h_out"] // 8)) * (-(-t1["w_out"] // 40))
    assert ntiles == {"tile": 1, "clip": 8, "batch": 273}[case]
    out = STEM[2] if fuse3 else STEM[1]
    sent = np.full((B + 1, 32, H // 4, W // 4), SENTINEL, np.float32)
    assert (op.set(out, sent) == SENTINEL).all()
    if not fuse3:
        assert (op.set(STEM[2], sent) == SENTINEL).all()
    assert op.run(B, torch.from_numpy(frames(case)).cuda(), swap) == list(STEM if fuse3 else STEM[:2])
    held = op.get(out, B + 1)
    got, spare = held[:B], held[B]
    (o64, a64), (o32, a32) = reference(dtype, case, swap)
    _, q_w = hooks(dtype)
    ws = weights()
    p0, p1, p2 = a64["pre"]
    stages = [(None, p0, True), (q_w(ws[STEM[1]][0]).numpy(), p1, True)]
    if fuse3:
        slack = _chain(stages + [(q_w(ws[STEM[2]][0]).numpy(), p2, True)], dtype)
        check(f"stemwaves {dtype} {case} swap={int(swap)} fused", got, o64, o32, p2, True, dtype, slack)
    else:           # layer 1 as stored: silu(p1), rounded to storage by the kernel's store alone
        slack = _chain(stages, dtype)
        check(f"stemwaves {dtype} {case} swap={int(swap)} unfused", got, fused_ref.silu(p1), fused_ref.silu(a32["pre"][1]), p1, True, dtype, slack)
        assert (op.get(STEM[2], B + 1) == SENTINEL).all(), "model.2.cv1's view was written by the op that does not compute it"
    assert (spare == SENTINEL).all(), f"{int((spare != SENTINEL).sum())} values behind the last valid map were written"
    assert pattern_left(op.pred).all() and pattern_left(op.best).all() and pattern_left(op.proto).all()
