"""vti_convert_raw / vti_convert_raw_frames on the device against rawframes.to_bgr, byte for byte, on seeded random bytes (every
byte string is a frame, so both clamps are exercised): the uniform call for every format, channel order and the shapes that move
frame starts and row ends off the vector sizes, with guard bands and with both pointers one byte off; the ragged call in three
orders on a poisoned buffer; and RawFrames sources through predict, process_frames and FrameFeeder against the BGR frames."""
import functools

import numpy as np
import pytest
import torch

from gpu_util import need_gpu
from vti_amd import rawframes as R

pytestmark = pytest.mark.gpu
POISON = 0xA5
GUARD = 64
FMTS = sorted(R.FORMATS, key=R.FORMATS.get)
SHAPES = [(2, 2), (2, 4), (4, 6), (6, 10), (18, 34), (34, 66), (64, 130)]
B = 3
RAGGED = [(6, 10, "yuyv"), (34, 66, "nv12"), (2, 2, "i420"), (18, 34, "uyvy"), (64, 130, "yv12")]


@functools.lru_cache(maxsize=None)
def _engine():
    import vti_amd
    return vti_amd.Engine("n", 2, H=64, W=64, max_batch=8)          # no weights: the conversion needs none


@functools.lru_cache(maxsize=None)
def _raw(fmt, H0, W0, n=B):
    """Seeded random frames and their host conversion, computed once and shared (read only)."""
    rng = np.random.Generator(np.random.PCG64(1000 * R.FORMATS[fmt] + 7 * H0 + W0))
    raw = rng.integers(0, 256, n * R.frame_bytes(fmt, H0, W0), dtype=np.uint8)
    raw.setflags(write=False)
    want = {rgb: R.to_bgr(raw, fmt, H0, W0, rgb) for rgb in (False, True)}
    for w in want.values():
        w.setflags(write=False)
    return raw, want


def _guarded(nbytes, shift=0):
    flat = torch.full((GUARD + shift + nbytes + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    return flat, flat[GUARD + shift:GUARD + shift + nbytes]


@pytest.mark.parametrize("rgb", (False, True), ids=("bgr", "rgb"))
@pytest.mark.parametrize("fmt", FMTS)
def test_uniform_call_every_shape_with_guards_and_with_both_pointers_one_byte_off(fmt, rgb):
    need_gpu()
    eng = _engine()
    for H0, W0 in SHAPES:
        raw, want = _raw(fmt, H0, W0)
        for shift in (0, 1):
            src = torch.zeros(raw.size + 16, dtype=torch.uint8, device="cuda")
            src[shift:shift + raw.size] = torch.from_numpy(raw.copy()).cuda()
            flat, out = _guarded(B * H0 * W0 * 3, shift)
            assert out.data_ptr() % 16 == shift and src.data_ptr() % 16 == 0
            got = eng.convert_raw(src[shift:shift + raw.size], fmt, H0, W0, rgb=rgb, out=out.view(B, H0, W0, 3))
            host = flat.cpu().numpy()
            assert np.array_equal(got.cpu().numpy(), want[rgb]), (fmt, H0, W0, rgb, shift)
            assert (host[:GUARD + shift] == POISON).all() and (host[-GUARD:] == POISON).all(), (fmt, H0, W0, rgb, shift)
            assert np.array_equal(src[shift:shift + raw.size].cpu().numpy(), raw)          # the input is never written
    # the wrapper's other inputs: host bytes in any shape, and an output it allocates
    raw, want = _raw(fmt, 6, 10)
    assert np.array_equal(eng.convert_raw(raw.tobytes(), R.FORMATS[fmt], 6, 10, rgb=rgb).cpu().numpy(), want[rgb])


@pytest.mark.parametrize("order", ((0, 1, 2, 3, 4), (4, 3, 2, 1, 0), (2, 4, 0, 3, 1)), ids=("as-listed", "reversed", "shuffled"))
def test_ragged_call_equals_the_uniform_calls_and_leaves_the_gaps(order):
    need_gpu()
    eng = _engine()
    members = [RAGGED[k] for k in order]
    shapes, fmts = [(h, w) for h, w, _ in members], [f for _, _, f in members]
    rt = eng.pack_raw_frames(shapes, fmts, "cuda")
    table = eng.pack_frames(shapes, "cuda")[0]
    assert all(o % 16 == 0 for o in rt.raw_offsets) and rt.raw_bytes >= rt.raw_offsets[-1] + rt.frame_bytes[-1]
    host_raw = np.full(rt.raw_bytes, 0x5A, np.uint8)
    for (h, w, f), off, fb in zip(members, rt.raw_offsets, rt.frame_bytes):
        host_raw[off:off + fb] = _raw(f, h, w)[0][:fb]                                     # frame 0 of the shared batch
    buf = torch.from_numpy(host_raw).cuda()
    for rgb in (False, True):
        out = torch.full((table.total_bytes + GUARD,), POISON, dtype=torch.uint8, device="cuda")
        assert eng.convert_raw_frames(buf, rt, table, rgb=rgb, out=out) is out
        got = out.cpu().numpy()
        written = np.zeros(got.size, bool)
        for (h, w, f), at in zip(members, table.byte_offsets):
            uniform = eng.convert_raw(torch.from_numpy(_raw(f, h, w)[0][:R.frame_bytes(f, h, w)].copy()).cuda(), f, h, w, rgb=rgb)
            assert np.array_equal(uniform.cpu().numpy()[0], _raw(f, h, w)[1][rgb][0])
            assert np.array_equal(got[at:at + 3 * h * w].reshape(h, w, 3), uniform.cpu().numpy()[0]), (f, h, w, rgb)
            written[at:at + 3 * h * w] = True
        assert not written.all() and (got[~written] == POISON).all()                     # the gaps and the guard band
        assert np.array_equal(buf.cpu().numpy(), host_raw)
    assert eng.convert_raw_frames(buf, rt, table).numel() == table.total_bytes             # an output it allocates


def _model():
    import vti_amd
    return vti_amd.YOLO(None, scale="n", nc=2, seed=3, cls_bias=-1.0, dtype="h2")


def _same_results(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.orig_shape == y.orig_shape and len(x) == len(y)
        assert x.boxes.data.cpu().numpy().tobytes() == y.boxes.data.cpu().numpy().tobytes()
        assert x.dets.cpu().numpy().tobytes() == y.dets.cpu().numpy().tobytes()
        assert (x.masks is None) == (y.masks is None)
        if x.masks is not None:
            assert x.masks.bits.cpu().numpy().tobytes() == y.masks.bits.cpu().numpy().tobytes()


def test_predict_takes_raw_frames():
    need_gpu()
    import vti_amd
    model = _model()
    kw = dict(conf=0.05, max_det=50, imgsz=64)
    raw, want = _raw("yuyv", 48, 64)
    bgr = want[False]
    for data in (raw, raw.reshape(B, 48, 64, 2), raw.tobytes(), torch.from_numpy(raw.copy()), torch.from_numpy(raw.copy()).cuda()):
        got = model.predict(vti_amd.RawFrames(data, "yuyv", 48, 64), **kw)
        ref = model.predict(np.array(bgr), **kw)
        assert all(r.orig_shape == (48, 64) for r in got) and len(got) == B
        _same_results(got, ref)
    print("detections per frame (uniform):", [len(r) for r in ref])
    _same_results(model.predict(vti_amd.RawFrames(raw, "yuyv", 48, 64), swap_rb=False, **kw), model.predict(np.array(bgr), swap_rb=False, **kw))
    # members of one size keep the stacked path, whatever their formats
    nv, nv_want = _raw("nv12", 48, 64)
    got = model.predict([vti_amd.RawFrames(raw, "yuyv", 48, 64), vti_amd.RawFrames(nv, "nv12", 48, 64)], **kw)
    _same_results(got, model.predict(np.concatenate((bgr, nv_want[False])), **kw))
    # two sizes and two formats: the frame table
    small, small_want = _raw("i420", 34, 66)
    members = [vti_amd.RawFrames(raw[:R.frame_bytes("yuyv", 48, 64)], "yuyv", 48, 64), vti_amd.RawFrames(small, 4, 34, 66)]
    frames = [np.array(bgr[0])] + [np.array(f) for f in small_want[False]]
    for extra in ({}, dict(retina_masks=True, mixed=True)):
        got = model.predict(members, **kw, **extra)
        ref = model.predict(frames, **kw, **extra)
        assert [r.orig_shape for r in got] == [(48, 64)] + [(34, 66)] * B
        _same_results(got, ref)
        print("detections per frame (two sizes):", [len(r) for r in ref], extra)
    assert sum(len(r) for r in ref) >= 1


def _strip(rec):
    return {k: v for k, v in rec.items() if k != "timestamp"}


def test_process_frames_takes_raw_frames():
    need_gpu()
    import vti_amd
    from test_gpu_annotate import _params
    h, w = 48, 64
    kw = dict(conf=0.05, iou=0.25, max_det=50, imgsz=64)
    raw, want = _raw("yuyv", h, w)
    bgr = np.array(want[False])
    model = _model()
    base = _params(h, w, "kmeans")
    got = vti_amd.StitchMeasurer(model, base).process_frames(vti_amd.RawFrames(raw, "yuyv", h, w), **kw)
    ref = vti_amd.StitchMeasurer(model, base).process_frames(bgr, **kw)
    assert [_strip(r) for r in got] == [_strip(r) for r in ref] and len(got) == B
    (ga, gr), (ra, rr) = (vti_amd.StitchMeasurer(model, base).process_frames(src, annotate="all", encode="jpeg", **kw)
                          for src in (vti_amd.RawFrames(raw, "yuyv", h, w), bgr))
    assert [_strip(r) for r in gr] == [_strip(r) for r in rr]
    assert [(b, data, items) for b, data, items in ga] == [(b, data, items) for b, data, items in ra] and len(ga) == B
    assert all(isinstance(data, bytes) and data[:2] == b"\xff\xd8" for _, data, _ in ga)
    plist = [_params(h, w, "kmeans", k) for k in range(2)]
    got = vti_amd.MultiCameraMeasurer(model, plist).process_frames(vti_amd.RawFrames(raw, "yuyv", h, w), [1, 0, 1], **kw)
    ref = vti_amd.MultiCameraMeasurer(model, plist).process_frames(bgr, [1, 0, 1], **kw)
    assert [_strip(r) for r in got] == [_strip(r) for r in ref]
    # two sizes and two formats, drawn and encoded at each frame's own size
    small, small_want = _raw("nv21", 34, 66)
    members = [vti_amd.RawFrames(raw, "yuyv", h, w), vti_amd.RawFrames(small[:R.frame_bytes("nv21", 34, 66)], "nv21", 34, 66)]
    frames = [np.array(f) for f in bgr] + [np.array(small_want[False][0])]
    (ga, gr), (ra, rr) = (vti_amd.StitchMeasurer(model, base).process_frames(src, annotate="all", encode="jpeg", mixed=True, **kw)
                          for src in (members, frames))
    assert [_strip(r) for r in gr] == [_strip(r) for r in rr] and len(gr) == B + 1
    assert [(b, data, items) for b, data, items in ga] == [(b, data, items) for b, data, items in ra]


def test_frame_feeder_with_raw_slots():
    need_gpu()
    import vti_amd
    h, w, depth, nb = 48, 64, 3, 2
    eng = vti_amd.Engine("n", 2, H=64, W=64, max_batch=nb, dtype="h2")
    eng.load_weights(vti_amd.random_weights(eng, seed=3, cls_bias=-1.0), 0)
    feeder = vti_amd.FrameFeeder(nb, h, w, depth=depth, device=0, fmt="yuyv")
    fb = R.frame_bytes("yuyv", h, w)
    assert feeder.host_view(0).shape == (nb, fb) and feeder.frame_bytes == fb
    rng = np.random.Generator(np.random.PCG64(77))
    out, ref = (eng.alloc_outputs(nb, 20, nb * 20, "bits", "cuda") for _ in range(2))
    for k in range(2 * depth):
        n = nb if k % 3 else 1                  # a partly filled slot too
        raw = rng.integers(0, 256, (n, fb), dtype=np.uint8)
        want = R.to_bgr(raw, "yuyv", h, w)
        if k % 2:
            slot = feeder.put(raw.reshape(n, h, w, 2))
        else:
            slot = feeder.next_slot()
            feeder.host_view(slot)[:n] = raw
            feeder.submit(slot, n)
        got = feeder.frames(slot)
        assert tuple(got.shape) == (n, h, w, 3) and np.array_equal(got.cpu().numpy(), want), k
        if n == nb:
            feeder.predict_into(eng, slot, out, conf=0.05, max_det=20)
            eng.predict_into(torch.from_numpy(want).cuda(), ref, conf=0.05, max_det=20)
            for key in ("counts", "offsets"):
                assert out[key].cpu().numpy().tobytes() == ref[key].cpu().numpy().tobytes(), (k, key)
            for b, c in enumerate(ref["counts"].cpu().tolist()):
                for key in ("dets", "xyxy"):
                    assert out[key][b, :c].cpu().numpy().tobytes() == ref[key][b, :c].cpu().numpy().tobytes(), (k, key, b)
            live = int(ref["offsets"][-1])
            assert out["masks"][:live].cpu().numpy().tobytes() == ref["masks"][:live].cpu().numpy().tobytes(), k
        else:
            feeder.release(slot)
    with pytest.raises(ValueError, match="raw bytes"):
        feeder.put(np.zeros(fb + 1, np.uint8))
