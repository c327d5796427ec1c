"""Layer-by-layer parity of the n-scale forward pass on canvases whose maps do not divide into the kernels' tiles.

Every other layerwise canvas has a width that is a multiple of 160, so stem_l1_kernel (8x40 tiles), bneck_pk (8x20 / 16x20),
convfold_kernel (4x20 / 8x20 low-resolution pixels), the fused head towers and conv1_pk's linear 80-pixel tiles never meet a
partial tile there.  letterbox_shape(auto=True) produces such canvases all the time (640x384, 960x736, 544x960).  Two canvases
(tests/test_plan_ragged.py pins, on the host, that they reach those kernels with clipped tiles):

  A  224x352  maps 56x88, 28x44, 14x22, 7x11 (1617 anchors): every tile of every fused / persistent kernel is clipped
  B  608x736  maps 152x184, 76x92, 38x46, 19x23: the default plan's conv1_pk rows and both Upsample+Concat folds

Bounds: the per-layer and pred / proto bounds of test_gpu_forward.py, unchanged.  On top of them the EDGE BAND check: for every
readable row whose map is ragged against the tile of the kernel that produced it, the maximum error on the clipped tiles may be
at most 4x the maximum error on the rest of the same map (floor: one unit in the last place of the storage type at the layer's
maximum).  With a correct kernel both are maxima of the same rounding-error distribution and the band has fewer samples, so the
ratio sits near or below 1; a dropped or misplaced tap, bias class or halo pixel costs far more than 10x -- and a layer-wide
maximum under the loose fp16 bound could hide it.  conv1_pk tiles the flattened [B*h*w] pixel index, so its clipped part is the
batch's trailing (B*h*w) % (tile_h*tile_w) pixels (gpu_util.clipped_mask).

Largest band / interior ratio measured on an MI355X over all cases below (37 to 76 ragged rows per case; the row that gave it):
  h2    1.59  model.21.cv1, canvas A under VTI_PK1_ALL=1 (conv1_pk, 71 trailing pixels of 231); 1.55 at max_batch=64 (model.6.m.0.cv2)
  fp16  2.00  model.21.cv2, same case: errors are whole fp16 units in the last place there, 4 on the band against 2 inside
  fp32  1.03  model.6.m.1.cv2, canvas A
The largest per-layer error in these runs: fp16 3.0e-3 of the layer's maximum (bound 6e-3).  No kernel needed a change.
Sensitivity, tried once: a library whose persistent fold took the interior bias class on tiles clipped at the right edge passed
test_gpu_forward.py and test_gpu_config5.py and failed every fp16 test here (band x8.9 to x18.5 on model.22.proto.cv3)."""
import functools

import pytest
import torch

from gpu_util import LAYER_TOL, PLAIN_PLAN, check_conv_rows, check_pred_proto, frames_u8, need_gpu, plan_env

pytestmark = pytest.mark.gpu

NC, SEED, GAIN, BAND = 80, 1, 1.7, 4.0
A, B_ = (224, 352), (608, 736)


@functools.lru_cache(maxsize=None)
def blob():
    """The seeded weights: they depend on the model description alone, not on canvas, dtype or plan."""
    import vti_amd
    return vti_amd.random_weights(vti_amd.Engine("n", NC, H=A[0], W=A[1], max_batch=1), seed=SEED, gain=GAIN)


@functools.lru_cache(maxsize=None)
def frames(B, H, W):
    return frames_u8(B, H, W, seed=3)       # shared: nobody writes to it


@functools.lru_cache(maxsize=None)
def oracle(H, W, B, mode, n):
    """(pred, proto, taps) of the CPU oracle on the first n of the B frames; computed once per key and never written to."""
    from oracle.model import OracleModel
    om = OracleModel(blob(), H, W, mode=mode)
    opred, oproto = om.forward_u8(frames(B, H, W)[:n], swap_rb=True, record=True)
    return opred, oproto, om.taps


def build(monkeypatch, hw, dtype, max_batch, env):
    """An engine planned under exactly the switches in `env` (not through engine_and_oracle: its cache key knows nothing of the
    environment)."""
    import vti_amd
    plan_env(monkeypatch, env)
    eng = vti_amd.Engine("n", NC, H=hw[0], W=hw[1], max_batch=max_batch, dtype=dtype)
    eng.load_weights(blob(), 0)
    return eng


def forward(eng, fr):
    pred, proto = eng.forward(torch.from_numpy(fr).cuda(), swap_rb=True)
    torch.cuda.synchronize()
    return pred, proto


def layerwise(eng, hw, B, n, dtype, pred, proto, band=BAND):
    """test_layerwise_parity's checks (+ the edge band) for the first n frames of the last forward; -> rows checked."""
    opred, oproto, taps = oracle(hw[0], hw[1], B, "fp32" if dtype == "h2" else dtype, n)
    tol = LAYER_TOL[dtype]
    checked, worst, name = check_conv_rows(eng, taps, n, dtype, tol, band=band, report=print, B_run=B)
    print(f"{hw[0]}x{hw[1]} {dtype} max_batch={eng.max_batch}: {checked} rows checked, largest band ratio {worst:.2f} ({name})")
    check_pred_proto(pred[:n], proto[:n], opred, oproto, taps, dtype, tol, NC, hw[0], hw[1])
    return checked


CASES = [   # canvas, B, dtype, switches
    (A, 3, "h2", {}), (A, 3, "fp16", {}), (A, 3, "fp32", {}),
    (B_, 1, "h2", {}), (B_, 1, "fp16", {}),
    (A, 3, "h2", {"VTI_PK1_ALL": "1"}), (A, 3, "fp16", {"VTI_PK1_ALL": "1"}),
]


@pytest.mark.parametrize("hw,B,dtype,env", CASES, ids=[f"{hw[0]}x{hw[1]}-{B}-{dtype}-{'+'.join(env) or 'default'}" for hw, B, dtype, env in CASES])
def test_layerwise_parity_ragged(monkeypatch, hw, B, dtype, env):
    """(a) + (b): every materialised conv output within the per-layer bound, clipped tiles no worse than 4x the interior, pred and
    proto within test_layerwise_parity's bounds."""
    need_gpu()
    eng = build(monkeypatch, hw, dtype, B, env)
    pred, proto = forward(eng, frames(B, *hw))
    checked = layerwise(eng, hw, B, B, dtype, pred, proto)
    assert checked >= len(eng.conv_table()) - 28      # as test_layerwise_parity: stem + layer 1, fused 3x3 mids, tower outputs that live in pred only


@pytest.mark.parametrize("dtype", ["h2", "fp16"])
def test_plain_plan_localises(monkeypatch, dtype):
    """(c) Canvas A with every fusion and every persistent kernel switched off: all 76 conv outputs exist and are within the
    per-layer bound, and the default plan's pred / proto agree with this plan's under the bounds that hold against the oracle.
    A failure in test_layerwise_parity_ragged with a pass here points at a fusion; a failure here points at a base kernel."""
    need_gpu()
    fr = frames(3, *A)
    plain = build(monkeypatch, A, dtype, 3, PLAIN_PLAN)
    table = plain.conv_table()
    assert len(table) == 76 and not any(t["fused"] or t["persistent"] for t in table) and plain.num_launches == 80
    ppred, pproto = forward(plain, fr)
    checked = layerwise(plain, A, 3, 3, dtype, ppred, pproto)
    assert checked == 76
    dflt = build(monkeypatch, A, dtype, 3, {})
    assert any(t["fused"] for t in dflt.conv_table())
    pred, proto = forward(dflt, fr)
    taps = oracle(A[0], A[1], 3, "fp32" if dtype == "h2" else dtype, 3)[2]
    check_pred_proto(pred, proto, ppred.cpu(), pproto.float().cpu().permute(0, 3, 1, 2), taps, dtype, LAYER_TOL[dtype], NC, *A)


@pytest.mark.parametrize("dtype", ["h2", "fp16"])
def test_plan_invariance_at_ragged_tiles(monkeypatch, dtype):
    """(d) Canvas A, 64 frames: the max_batch=64 plan (16x20 bottleneck tiles, larger tower and 3x3 tiles; every one clipped) must
    give BIT-identical pred / proto to the max_batch=3 plan on the same frames, as in
    test_batch_and_geometry_invariance_at_full_size where nothing is ragged; and its first frame passes the layerwise checks."""
    need_gpu()
    fr = frames(64, *A)
    big = build(monkeypatch, A, dtype, 64, {})
    small = build(monkeypatch, A, dtype, 3, {})
    tiles = lambda e: [t["tile"] for t in e.conv_table()]
    assert tiles(big) != tiles(small)
    x = torch.from_numpy(fr).cuda()
    pred, proto = big.forward(x, swap_rb=True)
    torch.cuda.synchronize()
    assert torch.isfinite(pred).all() and torch.isfinite(proto.float()).all()
    for lo in (0, 30, 61):
        p3, q3 = small.forward(x[lo:lo + 3].contiguous(), swap_rb=True)
        torch.cuda.synchronize()
        assert torch.equal(p3, pred[lo:lo + 3]), f"pred differs for frames {lo}..{lo + 2}: max|d|={(p3 - pred[lo:lo + 3]).abs().max().item():.3e}"
        assert torch.equal(q3, proto[lo:lo + 3]), f"proto differs for frames {lo}..{lo + 2}"
    checked = layerwise(big, A, 64, 1, dtype, pred, proto)
    assert checked >= len(big.conv_table()) - 28
