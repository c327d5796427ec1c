"""-m gpu: predict on a window of each frame.  Every comparison is tobytes() equality against today's calls on the contiguous
crops frame[y0:y0+h, x0:x0+w]: the canvas against vti_letterbox_frames, the mask stage against vti_masks_native_frames on the
crops' table pasted into the full frames' ragged layout by the host, vti_predict_windows against vti_predict_frames_native, and
YOLO.predict(window=) / process_frames(window=) against the public calls on the crops."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

from gpu_util import need_gpu

pytestmark = pytest.mark.gpu


def _flat(frames, table, poison=0xEE):
    host = np.full(table.total_bytes, poison, np.uint8)
    for f, off in zip(frames, table.byte_offsets):
        host[off:off + f.size] = f.reshape(-1)
    return torch.from_numpy(host).cuda()


def _crops(frames, windows):
    return [np.ascontiguousarray(f[y0:y0 + h, x0:x0 + w]) for f, (x0, y0, w, h) in zip(frames, windows)]


def _rand_frames(shapes, seed):
    return [np.random.Generator(np.random.PCG64(seed * 100 + k)).integers(0, 256, (h, w, 3), dtype=np.uint8)
            for k, (h, w) in enumerate(shapes)]


def _row_bytes(w0):
    return 8 * -(-w0 // 64)


def _paste(crop_bits, window, shape):
    """Bit-packed crop masks u8 [n, h, 8*ceil(w/64)] (LSB first) -> the frame's rows u8 [n, H0, 8*ceil(W0/64)]: bit (y, x) is the
    crop's bit (y - y0, x - x0) inside the window and 0 elsewhere."""
    (x0, y0, w, h), (H0, W0) = window, shape
    n = crop_bits.shape[0]
    px = np.unpackbits(np.ascontiguousarray(crop_bits), axis=-1, bitorder="little")[..., :w]
    full = np.zeros((n, H0, _row_bytes(W0) * 8), np.uint8)
    full[:, y0:y0 + h, x0:x0 + w] = px
    return np.packbits(full, axis=-1, bitorder="little")


def _shift(xyxy_crop, counts, windows):
    """xyxy_window + (float)(x0, y0, x0, y0), one f32 add per coordinate; rows at or past counts[b] stay zero."""
    out = np.zeros_like(xyxy_crop)
    for b, (x0, y0, _, _) in enumerate(windows):
        n = counts[b]
        out[b, :n] = xyxy_crop[b, :n] + np.array([x0, y0, x0, y0], np.float32).astype(np.float32)
    assert out.dtype == np.float32
    return out


# ---- letterbox ------------------------------------------------------------------------------------------------------------------
LB_SHAPE = (140, 200)
LB_WINDOWS = [(1, 1, 96, 64),          # copy branch
              (7, 11, 192, 128),       # exact 2x branch, odd start
              (3, 5, 131, 97),         # bilinear branch
              (163, 111, 37, 29),      # bottom-right corner, upscaled
              (199, 139, 1, 1),        # single pixel at the frame's last byte
              (0, 0, 200, 140)]        # whole frame


@pytest.mark.parametrize("first", range(len(LB_WINDOWS)))
def test_letterbox_windows_is_letterbox_frames_of_the_crops(first):
    """Two 140 x 200 frames on a 64 x 96 canvas; frame 0 takes window `first`, frame 1 the next one, so every window meets both
    batch positions (the second frame starts at byte 84000, the first at 0) and every branch meets every other in one launch."""
    need_gpu()
    import vti_amd
    eng = vti_amd.Engine("n", 2, H=64, W=96, max_batch=2)
    frames = _rand_frames([LB_SHAPE] * 2, seed=7)
    windows = [LB_WINDOWS[first], LB_WINDOWS[(first + 1) % len(LB_WINDOWS)]]
    wt = eng.pack_windows([LB_SHAPE] * 2, windows, "cuda")
    # the frame buffer sits between poisoned guards: nothing outside a frame may weigh on a canvas byte
    guard = 4096
    big = torch.full((guard + wt.total_bytes + guard,), 0xEE, dtype=torch.uint8, device="cuda")
    buf = big[guard:guard + wt.total_bytes]
    buf.copy_(_flat(frames, wt.frames))
    out = torch.full((2, 64, 96, 3), 0xA5, dtype=torch.uint8, device="cuda")      # poisoned: every canvas byte must be written
    got = eng.letterbox_windows(buf, wt, out=out).cpu().numpy()
    crops = _crops(frames, windows)
    ct, _, _ = eng.pack_frames([c.shape for c in crops], "cuda")
    want = eng.letterbox_frames(_flat(crops, ct), ct).cpu().numpy()
    for b in range(2):
        r, c = wt.row(b), ct.row(b)
        assert all(r[k] == c[k] for k in c if k != "offset"), (r, c)
        diff = np.argwhere(got[b] != want[b])
        assert diff.size == 0, (b, windows[b], len(diff), diff[:5].tolist())
    assert got.tobytes() == want.tobytes()
    branch = lambda r: "copy" if (r["new_h"], r["new_w"]) == (r["H0"], r["W0"]) else \
        "area2" if (r["H0"], r["W0"]) == (2 * r["new_h"], 2 * r["new_w"]) else "bilinear"
    want_branch = ["copy", "area2", "bilinear", "bilinear", "bilinear", "bilinear"]
    assert [branch(wt.row(b)) for b in range(2)] == [want_branch[first], want_branch[(first + 1) % 6]]
    assert bool((big[:guard] == 0xEE).all()) and bool((big[guard + wt.total_bytes:] == 0xEE).all())


# ---- the mask stage on synthetic inputs -------------------------------------------------------------------------------------------
MS_SHAPES = [(135, 241), (480, 640)]
# frame 0 (135 x 241) | frame 1 (480 x 640), one pair per call
MS_WINDOWS = [[(0, 0, 241, 135), (64, 100, 192, 380)],       # whole frame | x0 % 64 == 0, exactly three words, y0 > 0 and y0 + h == H0
              [(70, 3, 20, 50), (129, 7, 300, 200)],         # inside a single word | x0 % 64 == 1
              [(1, 10, 240, 125), (191, 0, 449, 480)],       # x0 % 64 == 1, ends at the 241-wide frame's right edge (pad bits stay 0),
                                                             # y0 + h == H0 | x0 % 64 == 63, ends at the right edge
              [(63, 0, 130, 100), (0, 0, 640, 480)]]         # x0 % 64 == 63, words 0..3 | whole frame
MS_MAX_DET = 8


def _ms_boxes(row, H, W):
    """Hand-placed boxes in canvas px for one frame whose crop has letterbox row `row`: covering the window, one touching each window
    edge, one narrower and one lower than a frame pixel, one in the middle."""
    l, t, nw, nh, g = row["left"], row["top"], row["new_w"], row["new_h"], row["gain"]
    r, b = l + nw, t + nh
    return [(0, 0, W, H),                                              # covers the window: clipped to it on all four sides
            (0, t + nh * 0.2, l + nw * 0.3, t + nh * 0.7),             # touches the left edge
            (l + nw * 0.6, t + nh * 0.1, W, t + nh * 0.5),             # the right edge
            (l + nw * 0.2, 0, l + nw * 0.8, t + nh * 0.3),             # the top edge
            (l + nw * 0.3, t + nh * 0.6, l + nw * 0.7, H),             # the bottom edge
            (l + nw * 0.5, t + nh * 0.1, l + nw * 0.5 + 0.3 * g, b),   # narrower than a pixel
            (l + nw * 0.1, t + nh * 0.5, r, t + nh * 0.5 + 0.4 * g)]   # lower than a pixel


@functools.lru_cache(maxsize=None)
def _ms_engine(dtype):
    import vti_amd
    eng = vti_amd.Engine("n", 2, H=160, W=160, max_batch=2, dtype=dtype)
    eng.load_weights(vti_amd.random_weights(eng, seed=2), 0)
    return eng


@pytest.mark.parametrize("call", range(len(MS_WINDOWS)))
@pytest.mark.parametrize("dtype", ["h2", "fp16"])
def test_masks_native_windows_places_the_crop_masks_in_the_frame(dtype, call):
    need_gpu()
    eng = _ms_engine(dtype)
    windows = MS_WINDOWS[call]
    wt = eng.pack_windows(MS_SHAPES, windows, "cuda")
    crop_shapes = [(h, w) for _, _, w, h in windows]
    ct, _, _ = eng.pack_frames(crop_shapes, "cuda")
    rng = np.random.default_rng(100 + call)
    dets = np.zeros((2, MS_MAX_DET, 38), np.float32)
    counts = np.array([7, 7], np.int32)
    for b in range(2):
        boxes = _ms_boxes(ct.row(b), 160, 160)
        dets[b, :7, :4] = np.array(boxes, np.float32)
        dets[b, :7, 4] = np.linspace(0.9, 0.3, 7)
        dets[b, :7, 5] = [0, 1, 0, 1, 0, 1, 0]
        dets[b, :7, 6:] = rng.standard_normal((7, 32))
    dets[:, 7] = 123.0                                                     # a row past the count: never read
    proto = torch.from_numpy(rng.standard_normal((2, 40, 40, 32)).astype(np.float32)).to(eng.torch_dtype).cuda()
    d_dets, d_counts = torch.from_numpy(dets).cuda(), torch.from_numpy(counts).cuda()
    # the crop path, today's calls
    xy_c = eng.scale_boxes(d_dets, d_counts, frames=ct)
    m_c, off_c, bases_c = eng.masks_native_frames(d_dets, d_counts, xy_c, proto, ct, "logit")
    # boxes: the window call is the crop call plus the origin
    xy_w = eng.scale_boxes_windows(d_dets, d_counts, wt)
    assert xy_w.cpu().numpy().tobytes() == _shift(xy_c.cpu().numpy(), counts, windows).tobytes()
    # offsets, bases and the slot layout are those of the full frames
    _, off_f, bases_f = eng.masks_native_frames(d_dets, d_counts, xy_w, proto, wt.frames, "logit", masks=torch.empty(0, dtype=torch.uint8,
                                                                                                                  device="cuda"), capacity_bytes=0)
    slot = [h * _row_bytes(w) for h, w in MS_SHAPES]
    total = 7 * slot[0] + 7 * slot[1]
    assert bases_f.cpu().tolist() == [0, 7 * slot[0], total] and eng.mask_native_windows_bytes(wt, MS_MAX_DET) == MS_MAX_DET * sum(slot)
    want = np.zeros(total, np.uint8)
    m_c_h, bc = m_c.cpu().numpy(), bases_c.cpu().tolist()
    nonempty = 0
    for b in range(2):
        (x0, y0, w, h) = windows[b]
        cs = h * _row_bytes(w)
        bits = m_c_h[bc[b]:bc[b] + 7 * cs].reshape(7, h, _row_bytes(w))
        nonempty += int((bits.reshape(7, -1).max(1) > 0).sum())
        base = 0 if b == 0 else 7 * slot[0]
        want[base:base + 7 * slot[b]] = _paste(bits, windows[b], MS_SHAPES[b]).reshape(-1)
    print(dtype, windows, "non-empty crop masks", nonempty, "of 14")
    assert nonempty >= 8, nonempty                                         # not a comparison of empty masks (two boxes per frame are sub-pixel)
    poison = 0xAB
    buf = torch.full((total + 4096,), poison, dtype=torch.uint8, device="cuda")
    _, off_w, bases_w = eng.masks_native_windows(d_dets, d_counts, proto, wt, "logit", masks=buf)
    torch.cuda.synchronize()
    assert torch.equal(off_w, off_f) and torch.equal(bases_w, bases_f) and torch.equal(off_w, off_c)
    got = buf.cpu().numpy()
    for b in range(2):
        base = 0 if b == 0 else 7 * slot[0]
        for i in range(7):
            a, e = got[base + i * slot[b]:base + (i + 1) * slot[b]], want[base + i * slot[b]:base + (i + 1) * slot[b]]
            assert a.tobytes() == e.tobytes(), (dtype, windows[b], b, i, int((a != e).sum()))
    assert got[:total].tobytes() == want.tobytes()
    assert bool((got[total:] == poison).all())                             # no byte after the last live slot is touched
    # the pad bits right of column W0 = 241 stay 0
    rows0 = np.unpackbits(got[:7 * slot[0]].reshape(7, 135, _row_bytes(241)), axis=-1, bitorder="little")
    assert int(rows0[..., 241:].sum()) == 0
    # capacity_bytes cuts inside the second frame's slots: the live prefix is as specified, the bytes after it are intact
    fit = 2
    end = 7 * slot[0] + fit * slot[1]
    cap = end + 1000
    assert cap < end + slot[1]
    buf.fill_(poison)
    _, off_k, bases_k = eng.masks_native_windows(d_dets, d_counts, proto, wt, "logit", masks=buf, capacity_bytes=cap)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert torch.equal(off_k, off_f) and torch.equal(bases_k, bases_f)
    assert got[:end].tobytes() == want[:end].tobytes() and bool((got[end:] == poison).all())
    buf.fill_(poison)
    eng.masks_native_windows(d_dets, d_counts, proto, wt, "logit", masks=buf, capacity_bytes=0)
    torch.cuda.synchronize()
    assert bool((buf == poison).all())
    if call in (0, 3):                                                     # the whole-frame window is vti_masks_native_frames itself
        b = 0 if call == 0 else 1
        m_f, _, _ = eng.masks_native_frames(d_dets, d_counts, xy_w, proto, wt.frames, "logit")
        base = 0 if b == 0 else 7 * slot[0]
        assert m_f.cpu().numpy()[base:base + 7 * slot[b]].tobytes() == want[base:base + 7 * slot[b]].tobytes()


# ---- end to end -------------------------------------------------------------------------------------------------------------------
E2E_SEED = 3                     # picked on the GPU: the crop path alone gives >= 3 instances with non-empty masks
E2E_SHAPES = [(240, 320), (135, 241), (240, 320), (300, 200)]
E2E_WINDOWS = [(17, 31, 200, 150), (0, 0, 241, 135), (64, 0, 256, 240), (63, 100, 137, 200)]
E2E_KW = dict(conf=0.25, iou=0.7, max_det=40)


@functools.lru_cache(maxsize=None)
def _e2e_engine(dtype="h2"):
    import vti_amd
    eng = vti_amd.Engine("n", 2, H=320, W=320, max_batch=4, dtype=dtype)
    eng.load_weights(vti_amd.random_weights(eng, seed=E2E_SEED, cls_bias=-1.0), 0)
    return eng


def _compare_with_the_crop_path(eng, frames, shapes, windows, nms=None):
    B, max_det = len(shapes), E2E_KW["max_det"]
    wt = eng.pack_windows(shapes, windows, "cuda")
    out = eng.alloc_outputs(B, max_det, 0, native_frames=wt.frames)
    out["masks"].fill_(0xAB)
    out["xyxy"].fill_(-3.0)
    eng.predict_windows_into(_flat(frames, wt.frames), wt, out, nms=nms, **E2E_KW)
    crops = _crops(frames, windows)
    ct, _, _ = eng.pack_frames([c.shape for c in crops], "cuda")
    ref = eng.alloc_outputs(B, max_det, 0, native_frames=ct)
    eng.predict_frames_into(_flat(crops, ct), ct, ref, native=True, nms=nms, **E2E_KW)
    torch.cuda.synchronize()
    h = lambda t: t.cpu().numpy()
    for k in ("input", "pred", "proto", "dets", "counts", "offsets"):                  # Specification item 1
        assert h(out[k]).tobytes() == h(ref[k]).tobytes(), k
    cnt = h(ref["counts"]).tolist()
    assert h(out["xyxy"]).tobytes() == _shift(h(ref["xyxy"]), cnt, windows).tobytes()  # item 2
    slot = [hh * _row_bytes(ww) for hh, ww in shapes]
    bases = np.concatenate(([0], np.cumsum([n * s for n, s in zip(cnt, slot)]))).tolist()
    assert h(out["mask_bases"]).tolist() == bases                                       # item 3
    rb, got = h(ref["mask_bases"]).tolist(), h(out["masks"])
    ref_m = h(ref["masks"])
    nonempty = 0
    for b, (x0, y0, w, hh) in enumerate(windows):
        cs = hh * _row_bytes(w)
        bits = ref_m[rb[b]:rb[b] + cnt[b] * cs].reshape(cnt[b], hh, _row_bytes(w))
        nonempty += int((bits.reshape(cnt[b], -1).max(1) > 0).sum()) if cnt[b] else 0
        want = _paste(bits, windows[b], shapes[b]).reshape(-1)
        assert got[bases[b]:bases[b + 1]].tobytes() == want.tobytes(), (b, windows[b])
    assert bool((got[bases[-1]:] == 0xAB).all())
    return out, ref, cnt, nonempty


def test_predict_windows_is_predict_frames_native_on_the_crops():
    need_gpu()
    eng = _e2e_engine()
    frames = _rand_frames(E2E_SHAPES, seed=5)
    out, ref, cnt, nonempty = _compare_with_the_crop_path(eng, frames, E2E_SHAPES, E2E_WINDOWS)
    print("detections per frame", cnt, "non-empty masks", nonempty)
    assert nonempty >= 3                                                   # a condition of the test, met by the crop path alone
    # the stage calls on the same outputs give the same bytes
    wt = eng.pack_windows(E2E_SHAPES, E2E_WINDOWS, "cuda")
    assert eng.letterbox_windows(_flat(frames, wt.frames), wt).cpu().numpy().tobytes() == out["input"].cpu().numpy().tobytes()
    assert eng.scale_boxes_windows(out["dets"], out["counts"], wt).cpu().numpy().tobytes() == out["xyxy"].cpu().numpy().tobytes()
    m, off, bases = eng.masks_native_windows(out["dets"], out["counts"], out["proto"], wt, "logit")
    live = int(bases[-1])
    assert torch.equal(bases, out["mask_bases"]) and torch.equal(m[:live], out["masks"][:live])
    # Specification item 4: with the whole frame as every window, every output byte is vti_predict_frames_native's
    whole = [(0, 0, w, h) for h, w in E2E_SHAPES]
    wt = eng.pack_windows(E2E_SHAPES, whole, "cuda")
    a = eng.alloc_outputs(4, 40, 0, native_frames=wt.frames)
    b = eng.alloc_outputs(4, 40, 0, native_frames=wt.frames)
    for o in (a, b):
        o["masks"].fill_(0xAB)
        o["xyxy"].fill_(-3.0)
    buf = _flat(frames, wt.frames)
    eng.predict_windows_into(buf, wt, a, **E2E_KW)
    eng.predict_frames_into(buf, wt.frames, b, native=True, **E2E_KW)
    torch.cuda.synchronize()
    for k in ("input", "pred", "proto", "dets", "counts", "offsets", "xyxy", "mask_bases", "masks"):
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
    assert int(a["counts"].sum()) >= 3 and int(a["masks"][:int(a["mask_bases"][-1])].count_nonzero()) > 0


def test_a_set_nms_table_applies_as_it_does_on_the_crops():
    need_gpu()
    import vti_amd
    eng = _e2e_engine()
    frames = _rand_frames(E2E_SHAPES, seed=5)
    table = eng.pack_nms_table([vti_amd.NmsParams(0.25, 0.7, 40), vti_amd.NmsParams(0.3, 0.5, 5, True, (1,))], "cuda")
    _, ref, cnt, _ = _compare_with_the_crop_path(eng, frames, E2E_SHAPES, E2E_WINDOWS, nms=(table, [0, 1, 1, 0]))
    assert max(cnt[1], cnt[2]) <= 5 and sum(cnt) >= 3, cnt
    for b in (1, 2):
        assert bool((ref["dets"][b, :cnt[b], 5] == 1).all())


def _model(**kw):
    import vti_amd
    return vti_amd.YOLO(None, scale="n", nc=2, seed=E2E_SEED, cls_bias=-1.0, dtype="h2", **kw)


def _same_as_crop_results(got, ref, windows, shapes):
    n_masks = 0
    for b, (g, r) in enumerate(zip(got, ref)):
        x0, y0, w, h = windows[b]
        assert g.orig_shape == tuple(shapes[b]) and g.boxes.orig_shape == tuple(shapes[b]) and r.orig_shape == (h, w)
        want = r.boxes.data.cpu().numpy().copy()
        want[:, :4] = want[:, :4] + np.array([x0, y0, x0, y0], np.float32)
        assert g.boxes.data.cpu().numpy().tobytes() == want.tobytes(), b
        assert g.dets.cpu().numpy().tobytes() == r.dets.cpu().numpy().tobytes()
        assert (g.masks is None) == (r.masks is None) and len(g) == len(r)
        if g.masks is None:
            continue
        H0, W0 = shapes[b]
        assert tuple(g.masks.bits.shape) == (len(r), H0, _row_bytes(W0)) and g.masks.orig_shape == (H0, W0)
        assert g.masks.bits.cpu().numpy().tobytes() == _paste(r.masks.bits.cpu().numpy(), windows[b], shapes[b]).tobytes(), b
        assert tuple(g.masks.data.shape) == (len(r), H0, W0)
        n_masks += int((g.masks.bits.reshape(len(r), -1).amax(1) > 0).sum())
    return n_masks


def test_yolo_predict_window_on_a_stacked_batch_with_classes_and_polygons():
    need_gpu()
    from vti_amd import polygons
    model = _model()
    stack = np.stack(_rand_frames([(240, 320)] * 3, seed=6))
    window = (17, 31, 217, 181)                                            # x1, y1 exclusive: the 150 x 200 crop
    wins = [(17, 31, 200, 150)] * 3
    kw = dict(conf=0.25, iou=0.7, max_det=40, imgsz=320)
    crops = np.ascontiguousarray(stack[:, 31:181, 17:217])
    got = model.predict(stack, window=window, **kw)
    ref = model.predict(crops, retina_masks=True, mixed=True, **kw)
    assert sum(len(r) for r in ref) >= 3
    assert _same_as_crop_results(got, ref, wins, [(240, 320)] * 3) >= 1
    # retina_masks / mixed change nothing: masks are always frame-resolution with window=
    again = model.predict(stack, window=window, retina_masks=False, **kw)
    assert [a.masks.bits.cpu().numpy().tobytes() if a.masks is not None else b"" for a in again] == \
           [a.masks.bits.cpu().numpy().tobytes() if a.masks is not None else b"" for a in got]
    # classes=: the one-row NMS table applies as on the crops
    got_c = model.predict(stack, window=window, classes=[1], **kw)
    ref_c = model.predict(crops, retina_masks=True, mixed=True, classes=[1], **kw)
    _same_as_crop_results(got_c, ref_c, wins, [(240, 320)] * 3)
    assert sum(len(r) for r in ref_c) >= 1 and all(bool((r.boxes.cls == 1).all()) for r in got_c)
    # polygons=True: the native polygon path on the frame rows; lazily made .xy gives the same values
    got_p = model.predict(stack, window=window, polygons=True, **kw)
    for gp, g in zip(got_p, got):
        if g.masks is None:
            continue
        assert gp.masks._xy is not None
        lazy = g.masks.xy
        assert len(lazy) == len(gp.masks.xy) and all(a.tobytes() == b.tobytes() for a, b in zip(gp.masks.xy, lazy))
        m_host = g.masks.data_u8.cpu().numpy()
        for i in range(min(len(lazy), 3)):                               # ... and the host restatement on the pasted mask
            exp = polygons.scale_coords((240, 320), polygons.masks2segments(m_host[i:i + 1])[0], (240, 320))
            assert lazy[i].tobytes() == np.asarray(exp, np.float32).tobytes(), i
            if lazy[i].size:
                assert lazy[i][:, 0].min() >= 17 and lazy[i][:, 0].max() <= 217 and lazy[i][:, 1].min() >= 31 and lazy[i][:, 1].max() <= 181


def test_yolo_predict_window_on_a_list_of_two_sizes():
    need_gpu()
    model = _model()
    shapes = [(240, 320), (135, 241), (240, 320)]
    frames = _rand_frames(shapes, seed=5)
    window = [(17, 31, 217, 181), None, (64, 0, 320, 240)]
    wins = [(17, 31, 200, 150), (0, 0, 241, 135), (64, 0, 256, 240)]
    kw = dict(conf=0.25, iou=0.7, max_det=40, imgsz=320)
    got = model.predict(frames, window=window, **kw)
    ref = model.predict(_crops(frames, wins), retina_masks=True, mixed=True, **kw)
    assert sum(len(r) for r in ref) >= 3
    assert _same_as_crop_results(got, ref, wins, shapes) >= 1
    got_p = model.predict(frames, window=window, polygons=True, **kw)
    for gp, g in zip(got_p, got):
        if g.masks is not None:
            assert all(a.tobytes() == b.tobytes() for a, b in zip(gp.masks.xy, g.masks.xy))


# ---- the measurers ----------------------------------------------------------------------------------------------------------------
def _params(**kw):
    import vti_amd
    from test_oracle_geometry import load_calib
    return vti_amd.MeasureParams(*load_calib(), **dict(dict(roi=(40, 60, 280, 200), min_stitches=1, drop_empty=False), **kw))


def _strip(rec):
    return {k: v for k, v in rec.items() if k not in ("timestamp", "camera")}


def _crop_set(model, stack, wins, kw):
    """The output set a windowed predict must give, built by the host from the public crop path: shifted boxes, pasted masks."""
    B, H0, W0 = stack.shape[:3]
    (x0, y0, w, h), = set(wins)
    crops = np.ascontiguousarray(stack[:, y0:y0 + h, x0:x0 + w])
    eng, o, _, _ = model._predict_outputs(crops, kw["conf"], kw["iou"], kw["max_det"], kw["imgsz"], False, False, True)
    torch.cuda.synchronize()
    cnt, off = o["counts"].cpu().tolist(), o["offsets"].cpu().tolist()
    masks = np.zeros((B * kw["max_det"], H0, _row_bytes(W0)), np.uint8)
    live = off[-1]
    masks[:live] = _paste(o["masks"][:live].cpu().numpy(), wins[0], (H0, W0))
    view = dict(dets=o["dets"].clone(), counts=o["counts"].clone(), offsets=o["offsets"].clone(),
                xyxy=torch.from_numpy(_shift(o["xyxy"].cpu().numpy(), cnt, wins)).cuda(), masks=torch.from_numpy(masks).cuda())
    return eng, view, cnt


@pytest.mark.parametrize("window", ["proper", "roi"])
def test_stitch_measurer_window_measures_the_crop_paths_outputs(window):
    need_gpu()
    import vti_amd
    from vti_amd.measure import CameraStream
    model = _model()
    p = _params()
    stack = np.stack(_rand_frames([(240, 320)] * 3, seed=6))
    kw = dict(conf=0.20, iou=0.25, max_det=40, imgsz=320)
    if window == "proper":
        arg, win = dict(window=(17, 31, 217, 181)), (17, 31, 200, 150)
    else:                                                                  # ROI (40, 60)..(280, 200) inclusive, grown by 16 px
        arg, win = dict(window="roi", window_margin=16), (24, 44, 273, 173)
    sm = vti_amd.StitchMeasurer(model, p, frame_buffer=8)
    annotated, got = sm.process_frames(stack, annotate="all", **arg, **kw)
    eng, view, cnt = _crop_set(model, stack, [win] * 3, kw)
    print(window, "detections per frame", cnt)
    assert sum(cnt) >= 3
    r = eng.measure(view, sm.params, 240, 320, native=True, stitch_rows=True)
    f64, i32 = r["frame_f64"].cpu().numpy(), r["frame_i32"].cpu().numpy()
    stream = CameraStream(8)
    assert [_strip(g) for g in got] == [_strip(stream.record(f64[b], i32[b])) for b in range(3)]
    # annotate="all" on one frame size: byte-identical to Engine.annotate on that set
    pics = eng.annotate(torch.from_numpy(stack).cuda(), view, r, sm.params, [0, 1, 2], native=True)["frames"].cpu().numpy()
    assert [a[0] for a in annotated] == [0, 1, 2]
    for k, (_, pic, _) in enumerate(annotated):
        assert pic.shape == (240, 320, 3) and pic.tobytes() == pics[k].tobytes(), k
    assert any(pics[k].tobytes() != stack[k].tobytes() for k in range(3))          # something was drawn


def test_a_whole_frame_window_is_retina_masks_and_the_rig_takes_windows_per_camera():
    need_gpu()
    import vti_amd
    from vti_amd.measure import CameraStream
    model = _model()
    p = [_params(), _params(roi=(10, 20, 300, 230))]
    stack = np.stack(_rand_frames([(240, 320)] * 4, seed=6))
    kw = dict(conf=0.20, iou=0.25, max_det=40, imgsz=320)
    a = vti_amd.StitchMeasurer(model, p[0], frame_buffer=8).process_frames(stack, window=(0, 0, 320, 240), **kw)
    b = vti_amd.StitchMeasurer(model, p[0], frame_buffer=8).process_frames(stack, retina_masks=True, **kw)
    assert [_strip(x) for x in a] == [_strip(x) for x in b]
    off = vti_amd.StitchMeasurer(model, dataclasses.replace(p[0], roi_enabled=False), frame_buffer=8)
    c = off.process_frames(stack, window="roi", **kw)                      # a disabled ROI means the whole frame
    d = vti_amd.StitchMeasurer(model, dataclasses.replace(p[0], roi_enabled=False), frame_buffer=8).process_frames(stack, retina_masks=True, **kw)
    assert [_strip(x) for x in c] == [_strip(x) for x in d]
    cams = [0, 1, 1, 0]
    rig = vti_amd.MultiCameraMeasurer(model, p, frame_buffer=8)
    whole = rig.process_frames(stack, cams, windows=[None, (0, 0, 320, 240)], **kw)
    want = vti_amd.MultiCameraMeasurer(model, p, frame_buffer=8).process_frames(stack, cams, retina_masks=True, **kw)
    assert [g["camera"] for g in whole] == cams and [_strip(x) for x in whole] == [_strip(x) for x in want]
    # one window for both cameras ("roi" of two cameras with one ROI size would do as well): the crop path's set, measured per camera
    win = (24, 44, 273, 173)
    rig = vti_amd.MultiCameraMeasurer(model, p, frame_buffer=8)
    got = rig.process_frames(stack, cams, windows=[(24, 44, 297, 217)] * 2, **kw)
    eng, view, cnt = _crop_set(model, stack, [win] * 4, kw)
    assert sum(cnt) >= 3
    r = eng.measure(view, rig.params, 240, 320, native=True, stitch_rows=False, cameras=cams)
    f64, i32 = r["frame_f64"].cpu().numpy(), r["frame_i32"].cpu().numpy()
    streams = [CameraStream(8), CameraStream(8)]
    assert [_strip(g) for g in got] == [_strip(streams[c].record(f64[k], i32[k])) for k, c in enumerate(cams)]
    # "roi" per camera gives windows of two sizes here: the records are those of the explicit windows
    rois = [(24, 44, 297, 217), (0, 4, 317, 240)]
    e = vti_amd.MultiCameraMeasurer(model, p, frame_buffer=8).process_frames(stack, cams, windows="roi", window_margin=16, **kw)
    f = vti_amd.MultiCameraMeasurer(model, p, frame_buffer=8).process_frames(stack, cams, windows=rois, **kw)
    assert [_strip(x) for x in e] == [_strip(x) for x in f]
