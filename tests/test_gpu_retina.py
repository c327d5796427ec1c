"""predict(retina_masks=True): frame-resolution masks (Ultralytics process_mask_native, the 8.1/8.2 scale_masks form) from
vti_masks_native, held against a torch-CPU restatement of steps 2-5 below on the same prototypes and detections."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_util import frames_u8, mask_iou, need_gpu, synth_pred
from oracle.letterbox import letterbox
from oracle.model import OracleModel
from oracle.postproc import crop_mask, non_max_suppression, scale_boxes

pytestmark = pytest.mark.gpu


@torch.inference_mode()
def process_mask_native(proto, coeffs, boxes, H0, W0, mode="logit"):
    """proto f32 [nm,mh,mw], coeffs f32 [n,nm], boxes f32 [n,4] in FRAME px -> bool masks [n,H0,W0]."""
    proto, coeffs, boxes = (torch.as_tensor(np.asarray(t), dtype=torch.float32) for t in (proto, coeffs, boxes))
    nm, mh, mw = proto.shape
    m = (coeffs @ proto.reshape(nm, -1)).reshape(-1, mh, mw)                        # 2. coefficients x prototypes
    if mode == "sigmoid":
        m = m.sigmoid()
    gain = min(mh / H0, mw / W0)                                                     # 3. scale_masks (8.1/8.2)
    pad_w, pad_h = (mw - W0 * gain) / 2, (mh - H0 * gain) / 2
    top, left, bottom, right = int(pad_h), int(pad_w), int(mh - pad_h), int(mw - pad_w)
    m = F.interpolate(m[None, :, top:bottom, left:right], (H0, W0), mode="bilinear", align_corners=False)[0]
    m = crop_mask(m, boxes)                                                          # 4. crop in frame px
    return m > (0.5 if mode == "sigmoid" else 0.0)                                   # 5. threshold


_engines = {}


def _engine(H, W, dtype, nm=32):
    import vti_amd
    key = (H, W, dtype, nm)
    if key not in _engines:
        eng = vti_amd.Engine("n", 80, nm=nm, H=H, W=W, max_batch=2, dtype=dtype)
        eng.load_weights(vti_amd.random_weights(eng, seed=2), 0)
        _engines[key] = eng
    return _engines[key]


FRAMES = [(960, 1280, 960), (640, 640, 640), (719, 1277, 640), (90, 120, 640)]


@pytest.mark.parametrize("H0,W0,imgsz", FRAMES)
@pytest.mark.parametrize("mode", ["logit", "sigmoid"])
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_masks_native_vs_restatement(dtype, mode, H0, W0, imgsz):
    need_gpu()
    import vti_amd
    H, W = vti_amd.letterbox_shape(H0, W0, imgsz)
    eng = _engine(H, W, dtype)
    rng = np.random.default_rng(11)
    B = 2
    pred = synth_pred(rng, B, 80, 32, eng.num_anchors, H=H, W=W, n_inst=25)
    proto = rng.standard_normal((B, H // 4, W // 4, 32)).astype(np.float32)
    proto_d = torch.from_numpy(proto).to(torch.float16 if dtype == "fp16" else torch.float32).cuda()
    dets, counts = eng.nms(torch.from_numpy(pred).cuda(), 0.25, 0.7, 300)
    xyxy = eng.scale_boxes(dets, counts, H0, W0)
    bits, off = eng.masks_native(dets, counts, xyxy, proto_d, H0, W0, mode, "bits")
    u8, off2 = eng.masks_native(dets, counts, xyxy, proto_d, H0, W0, mode, "u8")
    torch.cuda.synchronize()
    rb = 8 * -(-W0 // 64)
    assert bits.shape[1:] == (H0, rb) and u8.shape[1:] == (H0, W0)
    full = vti_amd.unpack_bits(bits, rb * 8)
    assert torch.equal(full[..., :W0], u8) and torch.equal(off, off2)                # packings agree
    assert int(full[..., W0:].sum()) == 0                                            # pad bits are 0
    o = off.cpu().numpy()
    live = int(o[-1])
    assert live == int(counts.sum()) > 0
    worst, flips, px = 1.0, 0, 0
    for b in range(B):
        n = int(counts[b])
        d = dets[b, :n].cpu().numpy()
        ref = process_mask_native(proto_d[b].float().cpu().permute(2, 0, 1), d[:, 6:], xyxy[b, :n].cpu(), H0, W0, mode).numpy()
        got = u8[o[b]:o[b + 1]].cpu().numpy()
        assert set(np.unique(got)) <= {0, 1}
        for i in range(n):
            worst = min(worst, mask_iou(got[i], ref[i]))
            flips += int((got[i] != ref[i]).sum())
        px += n * H0 * W0
        assert ref.sum() > 0
    assert worst >= 0.999, worst
    assert flips <= 20 + 5e-7 * px, (flips, px)      # stray threshold-tie pixels, the rate test_masks_vs_process_mask allows

    # slots at and beyond offsets[B] are not touched; a smaller capacity writes exactly that many slots
    for cap, extra in ((live, 3), (live - 3, 2)):
        buf = torch.full((cap + extra, H0, rb), 0xAB, dtype=torch.uint8, device="cuda")
        _, offc = eng.masks_native(dets, counts, xyxy, proto_d, H0, W0, mode, "bits", capacity=cap, masks=buf)
        torch.cuda.synchronize()
        assert torch.equal(offc, off)
        assert torch.equal(buf[:cap], bits[:cap]) and bool((buf[cap:] == 0xAB).all())


def test_masks_native_other_coefficient_count():
    need_gpu()
    import vti_amd
    eng = _engine(320, 320, "fp32", nm=16)
    dets = torch.zeros((1, 4, 6 + 16), device="cuda")
    counts = torch.ones((1,), dtype=torch.int32, device="cuda")
    xyxy = eng.scale_boxes(dets, counts, 320, 320)
    proto = torch.zeros((1, 80, 80, 16), device="cuda")
    with pytest.raises(vti_amd.VtiError) as ei:
        eng.masks_native(dets, counts, xyxy, proto, 320, 320, "logit", "bits", capacity=1)
    assert ei.value.code == -6


def _oracle_native(blob, frame, imgsz, conf, iou, max_det, nc):
    """The CPU oracle's own prototypes and detections for one frame -> (det rows, frame-px boxes, native masks)."""
    lb, g = letterbox(frame, imgsz)
    pred, proto = OracleModel(blob, g["H"], g["W"], "fp32").forward_u8(lb[None], swap_rb=True)
    det = non_max_suppression(pred.numpy(), conf, iou, max_det, nc=nc)[0]
    boxes = scale_boxes((g["H"], g["W"]), det[:, :4], frame.shape[:2])
    return det, boxes, process_mask_native(proto[0], det[:, 6:], boxes, *frame.shape[:2]).numpy()


@pytest.mark.parametrize("dtype", ["h2", "fp32"])
def test_predict_retina_reference_call(dtype):
    """measurement.py:208-210 with retina_masks=True: masks at the 960x1280 frame, everything else as without it."""
    need_gpu()
    import vti_amd
    from test_gpu_predict import _calibrated_model
    frame = frames_u8(1, 960, 1280, seed=21)[0]
    model = _calibrated_model(vti_amd, 2, dtype, frame, 960, 0.20)
    kw = dict(verbose=False, conf=0.20, iou=0.25, max_det=200, imgsz=960)
    r = model.predict(frame, retina_masks=True, **kw)[0]
    plain = model.predict(frame, **kw)[0]
    n = len(r.boxes)
    assert n > 0 and r.masks.data.shape == (n, 960, 1280) and r.masks.data.dtype == torch.float32
    assert torch.equal(r.boxes.data, plain.boxes.data)                             # boxes, confidences, classes
    assert plain.masks.data.shape == (n, 736, 960)
    det, boxes, omasks = _oracle_native(model._blob, frame, 960, 0.20, 0.25, 200, 2)
    assert n == len(det) and np.array_equal(r.boxes.cls.cpu().numpy(), det[:, 5])
    got = r.masks.data_u8.cpu().numpy()
    assert min(mask_iou(got[i], omasks[i]) for i in range(n)) >= 0.999
    eng = model._engine(736, 960, 1)
    for idx in range(min(n, 5)):
        bm = vti_amd.consumer.get_instance_mask_as_bitmap(eng, r, idx, 960, 1280)
        if bm is None:
            assert int(r.masks.data_u8[idx].sum()) == 0
        else:
            assert torch.equal(bm, r.masks.data_u8[idx])
    bms, nz = vti_amd.consumer.instance_bitmaps(eng, r, 960, 1280)
    assert torch.equal(bms, r.masks.data_u8) and torch.equal(nz.long(), r.masks.data_u8.flatten(1).sum(1))
    assert len(r.masks.xy) == n


def test_predict_retina_drop_reuse_layout():
    need_gpu()
    import vti_amd
    from test_gpu_predict import _calibrated_model
    frames = frames_u8(2, 719, 1277, seed=5)
    model = _calibrated_model(vti_amd, 2, "h2", frames[0], 640, 0.25)
    kw = dict(conf=0.25, iou=0.7, max_det=100, imgsz=640)
    keep_all = model.predict(frames[0], retina_masks=True, **kw)[0]
    model.drop_empty_masks = True
    dropped = model.predict(frames[0], retina_masks=True, **kw)[0]
    model.drop_empty_masks = False
    nonempty = keep_all.masks.data_u8.flatten(1).amax(1) > 0
    assert torch.equal(dropped.boxes.data, keep_all.boxes.data[nonempty])
    if dropped.masks is not None:
        assert torch.equal(dropped.masks.data_u8, keep_all.masks.data_u8[nonempty])
    # a second call on another frame leaves the first call's Results as they were
    first_boxes, first_masks = keep_all.boxes.data.clone(), keep_all.masks.bits.clone()
    second = model.predict(frames[1], retina_masks=True, **kw)[0]
    assert not torch.equal(second.boxes.data, first_boxes)
    assert torch.equal(keep_all.boxes.data, first_boxes) and torch.equal(keep_all.masks.bits, first_masks)
    # a plain call after a retina one: letterbox-size masks again
    plain = model.predict(frames[1], **kw)[0]
    H, W = vti_amd.letterbox_shape(719, 1277, 640)
    assert plain.masks.data.shape == (len(plain.boxes), H, W) and second.masks.data.shape == (len(second.boxes), 719, 1277)
