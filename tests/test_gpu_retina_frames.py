"""-m gpu: YOLO.predict(list of differing shapes, retina_masks=True, mixed=True) -- every frame's masks at that frame's own size,
boxes as without retina_masks, polygons from the frame's own rows, drop_empty_masks per frame, JPEG sources alike."""
import numpy as np
import pytest
import torch

from gpu_util import need_gpu

pytestmark = pytest.mark.gpu

KW = dict(conf=0.25, iou=0.7, max_det=50, imgsz=640)


def _frames(shapes, seed=4):
    return [np.random.Generator(np.random.PCG64(seed * 100 + k)).integers(0, 256, (h, w, 3), dtype=np.uint8)
            for k, (h, w) in enumerate(shapes)]


def _model(**kw):
    import vti_amd
    return vti_amd.YOLO(None, scale="n", nc=2, seed=3, cls_bias=-1.0, dtype="h2", **kw)


def test_predict_mixed_retina_masks_at_every_frames_own_size():
    need_gpu()
    from vti_amd import polygons
    shapes = [(480, 640), (481, 333), (135, 241)]
    frames = _frames(shapes)
    model = _model()
    with pytest.raises(ValueError, match="retina_masks"):
        model.predict(frames, retina_masks=True, **KW)                                # without mixed=True: as before
    res = model.predict(frames, retina_masks=True, mixed=True, **KW)
    plain = model.predict(frames, **KW)
    assert sum(len(r) for r in res) >= 3
    eng = model._engines[(640, 640)]
    for b, (r, p, (H0, W0)) in enumerate(zip(res, plain, shapes)):
        n = len(r)
        assert r.orig_shape == (H0, W0) and n == len(p)
        assert r.boxes.data.cpu().numpy().tobytes() == p.boxes.data.cpu().numpy().tobytes(), b   # boxes, conf, cls
        if not n:
            assert r.masks is None
            continue
        rb = 8 * -(-W0 // 64)
        assert tuple(r.masks.bits.shape) == (n, H0, rb) and tuple(r.masks.data.shape) == (n, H0, W0)
        assert r.masks.data.dtype == torch.float32 and r.masks.orig_shape == (H0, W0)
        # the same detections through the uniform retina call on this frame alone (its own rect canvas differs, so compare with
        # the stage call at this frame's size on the mixed call's canvas instead)
        xy = eng.scale_boxes(r.dets[None], torch.tensor([n], dtype=torch.int32, device="cuda"), H0, W0)
        assert xy[0, :n].cpu().numpy().tobytes() == r.boxes.xyxy.cpu().numpy().tobytes()
        m_host = r.masks.data_u8.cpu().numpy()
        assert set(np.unique(m_host)) <= {0, 1}
        segs = r.masks.xy
        assert len(segs) == n and len(r.masks.xyn) == n
        for i in range(n):
            exp = polygons.scale_coords((H0, W0), polygons.masks2segments(m_host[i:i + 1])[0], (H0, W0))
            assert segs[i].dtype == np.float32 and segs[i].tobytes() == np.asarray(exp, np.float32).tobytes(), (b, i)
    assert any(r.masks is not None and int(r.masks.data_u8.sum()) > 0 for r in res)
    # equal shapes, or mixed without retina_masks: today's paths and results
    same = model.predict(frames, mixed=True, **KW)
    for x, y in zip(same, plain):
        assert x.boxes.data.cpu().numpy().tobytes() == y.boxes.data.cpu().numpy().tobytes()
        assert (x.masks is None) == (y.masks is None)
        assert x.masks is None or x.masks.bits.cpu().numpy().tobytes() == y.masks.bits.cpu().numpy().tobytes()
    stack = [frames[0], frames[0][::-1].copy()]
    a = model.predict(stack, retina_masks=True, mixed=True, **KW)
    c = model.predict(np.stack(stack), retina_masks=True, **KW)
    for x, y in zip(a, c):
        assert x.boxes.data.cpu().numpy().tobytes() == y.boxes.data.cpu().numpy().tobytes()
        assert x.masks is None or x.masks.bits.cpu().numpy().tobytes() == y.masks.bits.cpu().numpy().tobytes()


def test_the_masks_are_the_stage_calls_on_the_same_outputs():
    need_gpu()
    shapes = [(481, 333), (480, 640), (135, 241)]
    frames = _frames(shapes, seed=6)
    model = _model()
    res = model.predict(frames, retina_masks=True, mixed=True, **KW)
    eng = model._engines[(640, 640)]
    o = next(iter(model._outs.values()))
    cnt = o["counts"].cpu().tolist()
    for b, (r, (H0, W0)) in enumerate(zip(res, shapes)):
        if not cnt[b]:
            continue
        bits, off = eng.masks_native(o["dets"], o["counts"], o["xyxy"], o["proto"], H0, W0, model.mask_mode, "bits")
        want = bits[int(off[b]):int(off[b]) + cnt[b]]
        assert r.masks.bits.cpu().numpy().tobytes() == want.cpu().numpy().tobytes(), b


def test_drop_empty_masks_drops_exactly_the_all_zero_masks():
    """The tiny frames are there so that all-zero masks occur (asserted at the end): a box narrower than one frame pixel can keep no
    column (x1 <= col < x2)."""
    need_gpu()
    shapes = [(480, 640), (24, 32), (481, 333), (30, 20), (135, 241)]
    frames = _frames(shapes)
    keep_all = _model().predict(frames, retina_masks=True, mixed=True, **KW)
    dropped = _model(drop_empty_masks=True).predict(frames, retina_masks=True, mixed=True, **KW)
    n_dropped = n_kept = 0
    for a, d in zip(keep_all, dropped):
        if a.masks is None:
            assert len(d) == 0 and d.masks is None
            continue
        nonempty = a.masks.data_u8.flatten(1).amax(1) > 0
        n_dropped += int((~nonempty).sum())
        n_kept += int(nonempty.sum())
        assert d.boxes.data.cpu().numpy().tobytes() == a.boxes.data[nonempty].cpu().numpy().tobytes()
        if int(nonempty.sum()):
            assert torch.equal(d.masks.data_u8, a.masks.data_u8[nonempty])
        else:
            assert d.masks is None
    print("dropped", n_dropped, "kept", n_kept)
    assert n_dropped >= 1 and n_kept >= 1                                             # the rule was exercised both ways


def test_jpeg_sources_of_two_sizes_take_the_same_path():
    need_gpu()
    from test_gpu_jpeg_decode import _file, _want_of
    files = [_file("smooth", 480, 640, 95, "420"), _file("noise", 135, 241, 95, "422"), _file("checker", 480, 640, 95, "444")]
    model = _model()
    got = model.predict(files, retina_masks=True, mixed=True, **KW)
    want = model.predict([_want_of(f) for f in files], swap_rb=False, retina_masks=True, mixed=True, **KW)
    assert [r.orig_shape for r in got] == [(480, 640), (135, 241), (480, 640)] and sum(len(r) for r in got) >= 1
    for x, y in zip(got, want):
        assert x.boxes.data.cpu().numpy().tobytes() == y.boxes.data.cpu().numpy().tobytes()
        assert (x.masks is None) == (y.masks is None)
        if x.masks is not None:
            assert tuple(x.masks.data.shape[1:]) == x.orig_shape
            assert x.masks.bits.cpu().numpy().tobytes() == y.masks.bits.cpu().numpy().tobytes()
    with pytest.raises(ValueError, match="retina_masks"):
        model.predict(files, retina_masks=True, **KW)
