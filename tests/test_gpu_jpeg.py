"""-m gpu: vti_encode_jpeg (the saved JPEG on the device) against the restatement in jpeg.py, byte for byte.  jpeg.py itself is held
to libjpeg's bytes on the CPU (tests/test_jpeg.py), and that file asserts that these contents reach ZRL, EOB, size-11 DC, size-10 AC
and stuffed bytes."""
import ctypes as C
import functools
import io

import numpy as np
import pytest
import torch

import jpeg_util as J
from gpu_util import frames_u8, need_gpu
from vti_amd import jpeg

pytestmark = pytest.mark.gpu
POISON = 0xA5
GUARD = 4096
SIZES = J.SIZES + [(480, 640)]
TRIPLES = (("noise", "ramp", "zrl"), ("tiles", "checker", "flat"))      # n = 3 different contents per call
QUALITIES = (95, 100, 10)


@functools.lru_cache(maxsize=None)
def _engine():
    import vti_amd
    return vti_amd.Engine("n", 2, H=64, W=64, max_batch=1)


@functools.lru_cache(maxsize=None)
def _batch(h, w, contents):
    return np.stack([J.frame(c, h, w) for c in contents])


@functools.lru_cache(maxsize=None)
def _want(h, w, content, q):
    return jpeg.encode(J.frame(content, h, w), q)


def _raw(eng, dframes, quality, rgb=0, max_bytes=None):
    """vti_encode_jpeg through the C ABI with the scratch and the output poisoned -> (out with its guard band, offsets, room)."""
    import vti_amd
    L = vti_amd.lib()
    n, h, w, _ = dframes.shape
    need = eng.encode_jpeg_scratch_bytes(n, h, w)
    room = int(L.vti_encode_jpeg_max_bytes(n, h, w)) if max_bytes is None else max_bytes
    ws = torch.full((need,), POISON, dtype=torch.uint8, device="cuda")
    out = torch.full((room + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    off = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    rc = L.vti_encode_jpeg(eng._ctx, C.c_void_p(dframes.data_ptr()), n, h, w, rgb, quality, C.c_void_p(ws.data_ptr()), need,
                           C.c_void_p(off.data_ptr()), C.c_void_p(out.data_ptr()), room, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.vti_last_error(eng._ctx)
    torch.cuda.synchronize()
    return out.cpu().numpy(), off.cpu().numpy(), room


def _files(out, off):
    return [out[off[k]:off[k + 1]].tobytes() for k in range(len(off) - 1)]


@pytest.mark.parametrize("contents", TRIPLES, ids=["-".join(t) for t in TRIPLES])
@pytest.mark.parametrize("h,w", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_every_file_equals_the_restatement(h, w, contents):
    need_gpu()
    eng = _engine()
    frames = _batch(h, w, contents)
    dframes = torch.from_numpy(frames).cuda()            # 17 x 33 and 135 x 241: rows and frame bases at odd addresses
    before = dframes.clone()
    for q in QUALITIES:
        out, off, room = _raw(eng, dframes, q)
        want = [_want(h, w, c, q) for c in contents]
        sizes = [len(b) for b in want]
        print(f"{h}x{w} {contents} q={q}: device sizes {np.diff(off).tolist()} restatement {sizes}")
        assert off.tolist() == [0] + np.cumsum(sizes).tolist()                     # the exclusive scan of the file sizes
        for k, b in enumerate(_files(out, off)):
            first = next((i for i, (x, y) in enumerate(zip(b, want[k])) if x != y), None)
            assert b == want[k], (contents[k], q, len(b), len(want[k]), first)
        assert (out[off[-1]:] == POISON).all()                                      # nothing at and beyond offsets[n]
        assert off[-1] <= room
    assert torch.equal(dframes, before)                                             # dev_frames is read only


def test_a_files_bytes_do_not_depend_on_its_batch_position_and_rgb_is_the_flip():
    need_gpu()
    eng = _engine()
    h, w = 50, 70
    a, b = J.frame("noise", h, w), J.frame("ramp", h, w)
    out, off, _ = _raw(eng, torch.from_numpy(np.stack([a, b, a])).cuda(), 95)
    f = _files(out, off)
    assert f[0] == f[2] == _want(h, w, "noise", 95) and f[1] == _want(h, w, "ramp", 95)
    flipped = np.ascontiguousarray(np.stack([a, b, a])[..., ::-1])
    out2, off2, _ = _raw(eng, torch.from_numpy(flipped).cuda(), 95, rgb=1)
    assert off2.tolist() == off.tolist() and _files(out2, off2) == f
    out3, off3, _ = _raw(eng, torch.from_numpy(flipped).cuda(), 95, rgb=0)          # ... and without the flag it is another picture
    assert _files(out3, off3)[0] != f[0]


def test_a_buffer_one_byte_short_gets_the_offsets_and_nothing_else():
    need_gpu()
    eng = _engine()
    h, w = 135, 241
    frames = _batch(h, w, TRIPLES[0])
    dframes = torch.from_numpy(frames).cuda()
    out, off, _ = _raw(eng, dframes, 95)
    total = int(off[-1])
    short, off_short, _ = _raw(eng, dframes, 95, max_bytes=total - 1)
    assert off_short.tolist() == off.tolist()
    assert (short == POISON).all()                                                  # dev_out is still entirely poison
    exact, off_exact, _ = _raw(eng, dframes, 95, max_bytes=total)
    assert off_exact.tolist() == off.tolist() and exact[:total].tobytes() == out[:total].tobytes() and (exact[total:] == POISON).all()
    # the Engine wrapper calls again by itself, with exactly the room the files need
    for room in (0, 1000, total - 1):
        data, o = eng.encode_jpeg(dframes, quality=95, max_bytes=room)
        assert data.numel() == total and o.cpu().numpy().tolist() == off.tolist()
        assert data.cpu().numpy().tobytes() == out[:total].tobytes()
    data, o = eng.encode_jpeg(dframes)                                              # the default room: no second call needed
    assert data.numel() == 3 * 3 * h * w + 1024 * 3 and data[:total].cpu().numpy().tobytes() == out[:total].tobytes()
    assert o.dtype == torch.int64 and o.cpu().numpy().tolist() == off.tolist()


def test_pillow_opens_the_device_files():
    pytest.importorskip("PIL")
    from PIL import Image
    need_gpu()
    eng = _engine()
    for (h, w) in ((17, 33), (135, 241)):
        data, off = eng.encode_jpeg(torch.from_numpy(_batch(h, w, TRIPLES[0])).cuda(), quality=95)
        data, off = data.cpu().numpy(), off.cpu().numpy()
        for k, b in enumerate(_files(data, off)):
            im = Image.open(io.BytesIO(b))
            im.load()
            assert im.size == (w, h) and im.mode == "RGB", k


def _strip(rec):
    return {k: v for k, v in rec.items() if k != "timestamp"}


def test_measurers_return_the_jpeg_of_the_annotated_frame():
    """process_frames(..., annotate=[...], encode="jpeg"): every returned file is jpeg.encode of the picture a second identical call
    without encode returns; text_items and records are the same."""
    need_gpu()
    import vti_amd
    from test_gpu_annotate import _params
    h, w = 480, 640
    kw = dict(conf=0.20, iou=0.25, max_det=200, imgsz=640)
    frames = frames_u8(3, h, w, 0)
    model = vti_amd.YOLO(None, scale="n", nc=2, seed=3, cls_bias=-1.0, dtype="h2")
    base = _params(h, w, "kmeans")
    sel = [2, 0]
    pics, recs = vti_amd.StitchMeasurer(model, base).process_frames(frames, annotate=sel, **kw)
    files, recs_j = vti_amd.StitchMeasurer(model, base).process_frames(frames, annotate=sel, encode="jpeg", jpeg_quality=90, **kw)
    assert [_strip(r) for r in recs_j] == [_strip(r) for r in recs]
    assert [f[0] for f in files] == sel and model._last_frames is None
    for (b, pic, items), (bj, data, items_j) in zip(pics, files):
        assert b == bj and isinstance(data, bytes) and items_j == items
        assert not np.array_equal(pic, frames[b])                                   # the overlay is in the picture
        assert data == jpeg.encode(pic, 90), (b, len(data))
    # MultiCameraMeasurer: a duplicated and reordered selection, the default quality
    cams, sel = [1, 0, 1], [2, 0, 2, 1]
    plist = [_params(h, w, "kmeans", k) for k in range(2)]
    pics, recs = vti_amd.MultiCameraMeasurer(model, plist).process_frames(frames, cams, annotate=sel, **kw)
    files, recs_j = vti_amd.MultiCameraMeasurer(model, plist).process_frames(frames, cams, annotate=sel, encode="jpeg", **kw)
    assert [_strip(r) for r in recs_j] == [_strip(r) for r in recs] and [f[0] for f in files] == sel
    want = {}
    for (b, pic, items), (bj, data, items_j) in zip(pics, files):
        if b not in want:
            want[b] = jpeg.encode(pic, 95)
        assert b == bj and items_j == items and data == want[b], (b, len(data), len(want[b]))
    assert files[0][1] == files[2][1]
