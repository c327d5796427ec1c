"""-m gpu: a batch whose frames differ in size through vti_letterbox_frames, vti_predict_frames and YOLO.predict(list).  Every
comparison is on raw bytes: against oracle/letterbox.py, against vti_letterbox on each frame alone, and against the composition of
the existing per-stage entry points on the same batch."""
import numpy as np
import pytest
import torch

from gpu_util import need_gpu
from oracle.letterbox import letterbox

pytestmark = pytest.mark.gpu

SIZES = [(960, 1280), (640, 640), (480, 640), (1080, 1920), (1920, 1920), (960, 960), (481, 333), (1200, 1600)]
ORDERS = [list(range(8)), [7, 6, 5, 4, 3, 2, 1, 0], [3, 6, 0, 5, 1, 7, 2, 4]]
_cache = {}


def frames_for(order, seed=0):
    """One random frame per size (the same content for a size whatever its batch position)."""
    out = []
    for k in order:
        h, w = SIZES[k]
        out.append(np.random.Generator(np.random.PCG64(seed * 100 + k)).integers(0, 256, (h, w, 3), dtype=np.uint8))
    return out


def flat_buffer(frames, table):
    host = np.full(table.total_bytes, 0xEE, np.uint8)
    for f, off in zip(frames, table.byte_offsets):
        host[off:off + f.size] = f.reshape(-1)
    return torch.from_numpy(host).cuda()


def engine(dtype, cls_bias=-1.0):
    import vti_amd
    key = (dtype, cls_bias)
    if key not in _cache:
        eng = vti_amd.Engine("n", 2, H=960, W=960, max_batch=8, dtype=dtype)
        blob = vti_amd.random_weights(eng, seed=3, cls_bias=cls_bias)
        eng.load_weights(blob, 0)
        _cache[key] = (eng, blob)
    return _cache[key]


@pytest.mark.parametrize("order", ORDERS, ids=["as_listed", "reversed", "shuffled"])
def test_letterbox_frames_equals_the_oracle_and_vti_letterbox_per_frame(order):
    need_gpu()
    eng, _ = engine("h2")
    frames = frames_for(order)
    table, _, _ = eng.pack_frames([f.shape for f in frames], "cuda")
    buf = flat_buffer(frames, table)
    out = torch.full((8, 960, 960, 3), 0xA5, dtype=torch.uint8, device="cuda")      # poisoned: every byte must be written
    got = eng.letterbox_frames(buf, table, out=out).cpu().numpy()
    for b, f in enumerate(frames):
        want, g = letterbox(f, (960, 960), auto=False)
        assert want.shape == (960, 960, 3)
        r = table.row(b)
        assert (r["new_h"], r["new_w"], r["top"], r["left"]) == (g["new_h"], g["new_w"], g["top"], g["left"])
        diff = np.argwhere(got[b] != want)
        assert diff.size == 0, (b, f.shape, len(diff), diff[:5].tolist())
        alone = eng.letterbox(torch.from_numpy(f[None]).cuda())[0].cpu().numpy()
        assert alone.tobytes() == got[b].tobytes(), (b, f.shape)


def test_letterbox_frames_on_a_rectangular_canvas_and_an_unaligned_uniform_source():
    """imgsz=(h, w) likewise; and vti_letterbox keeps taking frames at any byte address (its wide loads are alignment-gated)."""
    need_gpu()
    import vti_amd
    eng = vti_amd.Engine("n", 2, H=736, W=960, max_batch=8, dtype="fp16")
    frames = frames_for(list(range(8)), seed=1) + [np.random.default_rng(5).integers(0, 256, (1472, 1920, 3), dtype=np.uint8)]
    frames = frames[1:]                                                               # 8 frames, the last an exact 2x of 736x960
    table, _, _ = eng.pack_frames([f.shape for f in frames], "cuda")
    got = eng.letterbox_frames(flat_buffer(frames, table), table).cpu().numpy()
    for b, f in enumerate(frames):
        want, _ = letterbox(f, (736, 960), auto=False)
        assert got[b].tobytes() == want.tobytes(), (b, f.shape)
    through = np.random.default_rng(6).integers(0, 256, (736, 960, 3), dtype=np.uint8)
    for f in (frames[0], through, frames[7]):                                         # bilinear, copy through, exact 2x
        raw = torch.zeros(f.size + 1, dtype=torch.uint8, device="cuda")
        raw[1:] = torch.from_numpy(f.reshape(-1)).cuda()
        odd = raw[1:].view(1, *f.shape)
        assert odd.data_ptr() % 2 == 1
        want, _ = letterbox(f, (736, 960), auto=False)
        assert eng.letterbox(odd)[0].cpu().numpy().tobytes() == want.tobytes(), f.shape


def composition(eng, frames, conf, iou, max_det):
    """The existing entry points on the same batch: vti_letterbox per frame into one canvas batch, then the scored forward, NMS
    and masks on the whole batch, then vti_scale_boxes per frame."""
    B = len(frames)
    inp = torch.cat([eng.letterbox(torch.from_numpy(f[None]).cuda()) for f in frames])
    best = eng.alloc_best(B)
    pred, proto = eng.forward(inp, swap_rb=True, best=best)
    dets, counts = eng.nms(pred, conf, iou, max_det, best=best)
    cap = B * max_det
    masks, offsets = eng.masks(dets, counts, proto, "logit", "bits", capacity=cap)
    xyxy = torch.zeros((B, max_det, 4), dtype=torch.float32, device="cuda")
    for b, f in enumerate(frames):
        xyxy[b] = eng.scale_boxes(dets[b:b + 1], counts[b:b + 1], f.shape[0], f.shape[1])[0]
    return dict(input=inp, dets=dets, counts=counts, masks=masks, offsets=offsets, xyxy=xyxy)


def assert_same_outputs(got, want, B, max_det):
    cnt = want["counts"].cpu().tolist()
    off = want["offsets"].cpu().tolist()
    assert min(cnt) >= 1, cnt                                    # the comparison cannot pass on empty outputs
    assert got["input"].cpu().numpy().tobytes() == want["input"].cpu().numpy().tobytes()
    assert got["counts"].cpu().tolist() == cnt and got["offsets"].cpu().tolist() == off
    assert got["dets"].cpu().numpy().tobytes() == want["dets"].cpu().numpy().tobytes()
    live = off[-1]
    assert got["masks"][:live].cpu().numpy().tobytes() == want["masks"][:live].cpu().numpy().tobytes()
    for b in range(B):
        assert got["xyxy"][b, :cnt[b]].cpu().numpy().tobytes() == want["xyxy"][b, :cnt[b]].cpu().numpy().tobytes(), b
    return cnt, off


@pytest.mark.parametrize("dtype", ["h2", "fp32"])
def test_predict_frames_equals_the_composition_of_stage_calls(dtype):
    need_gpu()
    eng, _ = engine(dtype)
    frames = frames_for(ORDERS[2], seed=2)
    B, max_det, conf, iou = len(frames), 50, 0.25, 0.7
    table, _, _ = eng.pack_frames([f.shape for f in frames], "cuda")
    out = eng.alloc_outputs(B, max_det, B * max_det, "bits")
    out["xyxy"].fill_(-3.0)
    eng.predict_frames_into(flat_buffer(frames, table), table, out, conf, iou, max_det)
    want = composition(eng, frames, conf, iou, max_det)
    cnt, _ = assert_same_outputs(out, want, B, max_det)
    print(dtype, "detections per frame", cnt)
    # and scale_boxes(frames=) on its own is the per-frame call, rows beyond the counts zeroed alike
    xy = eng.scale_boxes(out["dets"], out["counts"], frames=table)
    assert xy.cpu().numpy().tobytes() == want["xyxy"].cpu().numpy().tobytes()


@pytest.mark.parametrize("drop_empty", [False, True])
def test_yolo_predict_takes_a_list_of_differing_shapes(drop_empty):
    need_gpu()
    import vti_amd
    from vti_amd import polygons
    model = vti_amd.YOLO(None, scale="n", nc=2, seed=3, cls_bias=-1.0, dtype="h2", drop_empty_masks=drop_empty)
    frames = frames_for(ORDERS[0], seed=2)
    max_det, conf, iou = 50, 0.25, 0.7
    res = model.predict(frames, conf=conf, iou=iou, max_det=max_det, imgsz=960)
    eng = model._engines[(960, 960)]
    want = composition(eng, frames, conf, iou, max_det)
    cnt, off = want["counts"].cpu().tolist(), want["offsets"].cpu().tolist()
    assert len(res) == 8 and min(cnt) >= 1
    for b, (r, f) in enumerate(zip(res, frames)):
        assert r.orig_shape == f.shape[:2] and r.boxes.orig_shape == f.shape[:2]
        n = cnt[b]
        data = torch.cat((want["xyxy"][b, :n], want["dets"][b, :n, 4:6]), 1)
        bits = want["masks"][off[b]:off[b] + n]
        if drop_empty:
            keep = bits.reshape(n, -1).amax(1) > 0
            data, bits = data[keep], bits[keep]
        assert r.boxes.data.cpu().numpy().tobytes() == data.cpu().numpy().tobytes(), b
        assert len(r) == data.shape[0]
        if not len(r):
            assert r.masks is None
            continue
        md = vti_amd.unpack_bits(bits, 960).float()
        assert tuple(r.masks.data.shape) == (len(r), 960, 960) and r.masks.orig_shape == f.shape[:2]
        assert r.masks.data.cpu().numpy().tobytes() == md.cpu().numpy().tobytes(), b
        if b in (0, 6):                                           # the host restatement is slow: the reference's frame and the odd one
            m_host = r.masks.data_u8.cpu().numpy()
            xy = r.masks.xy
            for i in range(min(len(xy), 4)):
                seg = xy[i]
                exp = polygons.scale_coords((960, 960), polygons.masks2segments(m_host[i:i + 1])[0], f.shape[:2])
                assert seg.dtype == np.float32 and seg.tobytes() == np.asarray(exp, np.float32).tobytes(), (b, i)
                assert seg.size == 0 or (seg[:, 0].max() <= f.shape[1] and seg[:, 1].max() <= f.shape[0])


def test_a_list_of_equal_shapes_keeps_the_stacked_path():
    need_gpu()
    import vti_amd
    model = vti_amd.YOLO(None, scale="n", nc=2, seed=3, cls_bias=-1.0, dtype="h2")
    stack = np.random.Generator(np.random.PCG64(9)).integers(0, 256, (8, 480, 640, 3), dtype=np.uint8)
    a = model.predict(stack, max_det=50, imgsz=640)
    b = model.predict([f for f in stack], max_det=50, imgsz=640)
    assert (480, 640) in model._engines and not model._frame_tables           # rect letterbox, no frame table
    assert sum(len(r) for r in a) >= 8
    for x, y in zip(a, b):
        assert x.orig_shape == y.orig_shape == (480, 640)
        assert x.boxes.data.cpu().numpy().tobytes() == y.boxes.data.cpu().numpy().tobytes()
        assert (x.masks is None) == (y.masks is None)
        if x.masks is not None:
            assert x.masks.bits.cpu().numpy().tobytes() == y.masks.bits.cpu().numpy().tobytes()
