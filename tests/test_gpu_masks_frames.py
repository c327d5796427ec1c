"""-m gpu: vti_masks_native_frames, the ragged mask buffer.  The criterion is byte identity: frame b's slots are those the uniform
vti_masks_native writes for frame b at H0[b] x W0[b] from the same dets, xyxy, counts and prototypes.  The torch restatement of
tests/test_gpu_retina.py, applied to both, guards against the two moving together."""
import functools

import numpy as np
import pytest
import torch

from gpu_util import mask_iou, need_gpu, synth_pred
from test_gpu_retina import process_mask_native

pytestmark = pytest.mark.gpu

# both axes shrinking (two-taps footprint, small th) | upscaling (contiguous footprint) | the identity pads | no detections |
# widths that are no multiple of 64, portrait | landscape pads the other way
SHAPES = [(90, 120), (1080, 1920), (640, 640), (200, 300), (481, 333), (120, 90)]
EMPTY = 3
B, MAX_DET = len(SHAPES), 300


@functools.lru_cache(maxsize=None)
def _engine(dtype):
    import vti_amd
    eng = vti_amd.Engine("n", 80, H=640, W=640, max_batch=B, dtype=dtype)
    eng.load_weights(vti_amd.random_weights(eng, seed=2), 0)
    return eng


@functools.lru_cache(maxsize=None)
def _case(dtype, mode):
    """One ragged call and the uniform call at every frame's size, all on the same detections.  Computed once, never changed."""
    import vti_amd
    eng = _engine(dtype)
    rng = np.random.default_rng(11)
    pred = synth_pred(rng, B, 80, 32, eng.num_anchors, H=640, W=640, n_inst=25)
    pred[EMPTY, 4:4 + 80] = 0.0                                                       # a frame without detections between full ones
    proto = rng.standard_normal((B, 160, 160, 32)).astype(np.float32)
    proto_d = torch.from_numpy(proto).to(torch.float16 if dtype == "fp16" else torch.float32).cuda()
    dets, counts = eng.nms(torch.from_numpy(pred).cuda(), 0.25, 0.7, MAX_DET)
    table, _, _ = eng.pack_frames(SHAPES, "cuda")
    xyxy = eng.scale_boxes(dets, counts, frames=table)
    masks, off, bases = eng.masks_native_frames(dets, counts, xyxy, proto_d, table, mode)
    uniform = {}
    for b, (H0, W0) in enumerate(SHAPES):
        if b != EMPTY:
            uniform[b] = eng.masks_native(dets, counts, xyxy, proto_d, H0, W0, mode, "bits")
    torch.cuda.synchronize()
    lay = [eng.mask_native_layout(h, w) for h, w in SHAPES]
    return dict(eng=eng, table=table, dets=dets, counts=counts, xyxy=xyxy, proto=proto_d, masks=masks, off=off, bases=bases,
                uniform=uniform, lay=lay, cnt=counts.cpu().tolist())


def _slots(c, masks, b, n=None):
    n = c["cnt"][b] if n is None else n
    return c["eng"].frame_masks(masks, c["table"], b, int(c["bases"][b]), n)


@pytest.mark.parametrize("mode", ["logit", "sigmoid"])
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_ragged_slots_equal_the_uniform_call_per_frame(dtype, mode):
    need_gpu()
    import vti_amd
    c = _case(dtype, mode)
    cnt, lay = c["cnt"], c["lay"]
    assert cnt[EMPTY] == 0 and all(n >= 20 for b, n in enumerate(cnt) if b != EMPTY), cnt
    want_off = np.concatenate(([0], np.cumsum(cnt)))
    want_bases = np.concatenate(([0], np.cumsum([n * l["slot_bytes"] for n, l in zip(cnt, lay)])))
    assert c["off"].cpu().tolist() == want_off.tolist()
    assert c["bases"].dtype == torch.int64 and c["bases"].cpu().tolist() == want_bases.tolist()
    assert all(v % 8 == 0 for v in want_bases.tolist())
    assert c["masks"].numel() == want_bases[-1]                                       # capacity_bytes=None sizes the buffer exactly
    for b, (H0, W0) in enumerate(SHAPES):
        if b == EMPTY:
            continue
        ubits, uoff = c["uniform"][b]
        assert torch.equal(uoff, c["off"])
        mine, theirs = _slots(c, c["masks"], b), ubits[want_off[b]:want_off[b + 1]]
        assert mine.shape == theirs.shape == (cnt[b], H0, lay[b]["row_bytes"])
        diff = int((mine != theirs).sum())
        assert diff == 0, (b, (H0, W0), diff)
        assert int(mine.reshape(cnt[b], -1).amax(1).count_nonzero()) >= 1, b       # not a comparison of empty masks
        # the restatement, first on the uniform call's output, then on the ragged one: a miss names its side
        ref = process_mask_native(c["proto"][b].float().cpu().permute(2, 0, 1), c["dets"][b, :cnt[b], 6:].cpu(),
                                  c["xyxy"][b, :cnt[b]].cpu(), H0, W0, mode).numpy()
        assert ref.sum() > 0
        px = cnt[b] * H0 * W0
        for side, bits in (("uniform", theirs), ("ragged", mine)):
            full = vti_amd.unpack_bits(bits, lay[b]["row_bytes"] * 8).cpu().numpy()
            assert int(full[..., W0:].sum()) == 0, (side, b)                          # pad bits are 0
            got = full[..., :W0]
            worst = min(mask_iou(got[i], ref[i]) for i in range(cnt[b]))
            flips = int((got != ref).sum())
            print(dtype, mode, side, (H0, W0), "IoU min", worst, "flips", flips, "of", px)
            assert worst >= 0.999, (side, b, worst)
            assert flips <= 20 + 5e-7 * px, (side, b, flips, px)


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_capacity_in_bytes_cuts_inside_a_slot(dtype):
    need_gpu()
    c = _case(dtype, "logit")
    eng, cnt, lay = c["eng"], c["cnt"], c["lay"]
    bases = c["bases"].cpu().tolist()
    total = c["masks"].numel()
    cut_frame, fit = 2, 3                                                             # inside (640, 640)'s run, off a slot boundary
    assert cnt[cut_frame] > fit + 1
    end = bases[cut_frame] + fit * lay[cut_frame]["slot_bytes"]
    cap = end + 1000
    assert cap < bases[cut_frame] + (fit + 1) * lay[cut_frame]["slot_bytes"] and cap % lay[cut_frame]["slot_bytes"] != 0
    buf = torch.full((total,), 0xAB, dtype=torch.uint8, device="cuda")
    _, off, bs = eng.masks_native_frames(c["dets"], c["counts"], c["xyxy"], c["proto"], c["table"], "logit", masks=buf,
                                         capacity_bytes=cap)
    torch.cuda.synchronize()
    assert torch.equal(off, c["off"]) and torch.equal(bs, c["bases"])
    assert torch.equal(buf[:end], c["masks"][:end])                                   # every slot that fits, completely
    assert bool((buf[end:] == 0xAB).all())                                            # no byte of the slot that did not fit is written
    buf.fill_(0xAB)
    off.fill_(-1)
    bs.fill_(-1)
    eng.masks_native_frames(c["dets"], c["counts"], c["xyxy"], c["proto"], c["table"], "logit", masks=buf, capacity_bytes=0,
                            offsets=off, mask_bases=bs)
    torch.cuda.synchronize()
    assert torch.equal(off, c["off"]) and torch.equal(bs, c["bases"]) and bool((buf == 0xAB).all())


@pytest.mark.parametrize("dtype", ["h2", "fp32"])
def test_predict_frames_into_native_equals_the_stage_calls(dtype):
    need_gpu()
    from test_gpu_frames import engine, flat_buffer, frames_for
    eng, _ = engine(dtype)
    frames = frames_for([0, 6, 2, 3], seed=2)
    n, max_det, conf, iou = len(frames), 50, 0.25, 0.7
    table, _, _ = eng.pack_frames([f.shape for f in frames], "cuda")
    buf = flat_buffer(frames, table)
    plain = eng.alloc_outputs(n, max_det, n * max_det, "bits")
    eng.predict_frames_into(buf, table, plain, conf, iou, max_det)
    out = eng.alloc_outputs(n, max_det, 0, native_frames=table)
    out["masks"].fill_(0xAB)
    eng.predict_frames_into(buf, table, out, conf, iou, max_det, native=True)
    torch.cuda.synchronize()
    cnt = plain["counts"].cpu().tolist()
    assert min(cnt) >= 1, cnt
    for k in ("dets", "counts", "xyxy", "offsets"):
        assert out[k].cpu().numpy().tobytes() == plain[k].cpu().numpy().tobytes(), k
    masks, off, bases = eng.masks_native_frames(out["dets"], out["counts"], out["xyxy"], out["proto"], table, "logit")
    torch.cuda.synchronize()
    assert torch.equal(bases, out["mask_bases"]) and torch.equal(off, out["offsets"])
    live = int(bases[-1])
    assert live == masks.numel() > 0 and torch.equal(out["masks"][:live], masks)
    assert bool((out["masks"][live:] == 0xAB).all()) and int(masks.count_nonzero()) > 0
    with pytest.raises(ValueError):
        eng.predict_frames_into(buf, table, plain, conf, iou, max_det, native=True)
