"""-m gpu: vti_encode_jpeg_frames -- the JPEG files of a batch whose frames differ in size, byte for byte the restatement jpeg.py
and vti_encode_jpeg of each frame alone; then the whole mixed-size pipeline (predict, measure, annotate, encode) through
MultiCameraMeasurer.process_frames(..., mixed=True)."""
import ctypes as C
import dataclasses
import functools
import io

import numpy as np
import pytest
import torch

import jpeg_util as J
from gpu_util import need_gpu
from test_gpu_jpeg import GUARD, POISON, SIZES, _engine, _files, _raw, _want
from vti_amd import jpeg

pytestmark = pytest.mark.gpu
CONTENTS = ("noise", "ramp", "zrl", "tiles", "checker", "flat", "noise")   # one per size of SIZES: mixed contents in one call
QUALITIES = (95, 100, 10)


def _flat(frames, table):
    flat = np.zeros(table.total_bytes, np.uint8)
    for f, at in zip(frames, table.byte_offsets):
        flat[at:at + f.size] = f.reshape(-1)
    return torch.from_numpy(flat).cuda()


def _raw_frames(eng, dflat, table, quality, rgb=0, max_bytes=None):
    """vti_encode_jpeg_frames through the C ABI with the scratch and the output poisoned -> (out with its guard band, offsets, room)."""
    import vti_amd
    L = vti_amd.lib()
    n = table.B
    hp = C.c_void_p(table.host.data_ptr())
    need = int(L.vti_encode_jpeg_frames_scratch_bytes(eng._ctx, hp))
    room = int(L.vti_encode_jpeg_frames_max_bytes(hp)) if max_bytes is None else max_bytes
    ws = torch.full((need,), POISON, dtype=torch.uint8, device="cuda")
    out = torch.full((room + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    off = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    rc = L.vti_encode_jpeg_frames(eng._ctx, C.c_void_p(dflat.data_ptr()), hp, C.c_void_p(table.dev.data_ptr()), n, rgb, quality,
                                  C.c_void_p(ws.data_ptr()), need, C.c_void_p(off.data_ptr()), C.c_void_p(out.data_ptr()), room,
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.vti_last_error(eng._ctx)
    torch.cuda.synchronize()
    return out.cpu().numpy(), off.cpu().numpy(), room


@functools.lru_cache(maxsize=None)
def _batch():
    eng = _engine()
    frames = [J.frame(c, h, w) for c, (h, w) in zip(CONTENTS, SIZES)]
    table, _, _ = eng.pack_frames(SIZES, "cuda")
    return eng, frames, table, _flat(frames, table)


def test_every_file_equals_the_restatement_and_the_frame_encoded_alone():
    need_gpu()
    eng, frames, table, dflat = _batch()
    assert len(SIZES) == 7 and (1, 1) in SIZES and (480, 640) in SIZES and len(set(CONTENTS)) == 6
    before = dflat.clone()
    for q in QUALITIES:
        out, off, room = _raw_frames(eng, dflat, table, q)
        got = _files(out, off)
        want = [_want(h, w, c, q) for c, (h, w) in zip(CONTENTS, SIZES)]
        print(f"q={q}: device sizes {np.diff(off).tolist()} restatement {[len(b) for b in want]}")
        assert off.tolist() == [0] + np.cumsum([len(b) for b in want]).tolist()     # back to back and unpadded
        for k, (b, f) in enumerate(zip(got, frames)):
            first = next((i for i, (x, y) in enumerate(zip(b, want[k])) if x != y), None)
            assert b == want[k], (SIZES[k], q, len(b), len(want[k]), first)
            alone, off1, _ = _raw(eng, torch.from_numpy(f[None]).cuda(), q)            # vti_encode_jpeg, n = 1, this frame's size
            assert b == _files(alone, off1)[0], (SIZES[k], q)
            assert b[163:167] == bytes([f.shape[0] >> 8, f.shape[0] & 255, f.shape[1] >> 8, f.shape[1] & 255])      # SOF0: its own size
        assert (out[off[-1]:] == POISON).all() and off[-1] <= room
    assert torch.equal(dflat, before)                                               # dev_frames is read only


def test_a_files_bytes_do_not_depend_on_its_position_and_rgb_is_the_flip():
    need_gpu()
    eng, frames, table, dflat = _batch()
    out, off, _ = _raw_frames(eng, dflat, table, 95)
    f = _files(out, off)
    rev_table, _, _ = eng.pack_frames(SIZES[::-1], "cuda")
    out_r, off_r, _ = _raw_frames(eng, _flat(frames[::-1], rev_table), rev_table, 95)
    assert _files(out_r, off_r) == f[::-1]
    flipped = [np.ascontiguousarray(x[..., ::-1]) for x in frames]
    out2, off2, _ = _raw_frames(eng, _flat(flipped, table), table, 95, rgb=1)
    assert off2.tolist() == off.tolist() and _files(out2, off2) == f
    out3, off3, _ = _raw_frames(eng, _flat(flipped, table), table, 95, rgb=0)       # ... and without the flag it is another picture
    assert _files(out3, off3)[0] != f[0]


def test_a_buffer_one_byte_short_gets_the_offsets_and_nothing_else():
    need_gpu()
    eng, frames, table, dflat = _batch()
    out, off, _ = _raw_frames(eng, dflat, table, 95)
    total = int(off[-1])
    short, off_short, _ = _raw_frames(eng, dflat, table, 95, max_bytes=total - 1)
    assert off_short.tolist() == off.tolist() and (short == POISON).all()           # exact offsets, dev_out still entirely poison
    exact, off_exact, _ = _raw_frames(eng, dflat, table, 95, max_bytes=total)
    assert off_exact.tolist() == off.tolist() and exact[:total].tobytes() == out[:total].tobytes() and (exact[total:] == POISON).all()
    # the Engine wrapper calls again by itself, with exactly the room the files need; its default room is the sum over the frames
    for room in (0, total - 1):
        data, o = eng.encode_jpeg(dflat, quality=95, max_bytes=room, table=table)
        assert data.numel() == total and o.cpu().numpy().tolist() == off.tolist() and data.cpu().numpy().tobytes() == out[:total].tobytes()
    data, o = eng.encode_jpeg(dflat, table=table)
    assert data.numel() == sum(3 * h * w + 1024 for h, w in SIZES) and data[:total].cpu().numpy().tobytes() == out[:total].tobytes()


def test_the_annotated_buffer_and_its_table_are_encoded_directly():
    """vti_annotate_frames' (buf, table) -> vti_encode_jpeg_frames, for the four large sizes: each file is vti_encode_jpeg of the dense
    picture (Pillow: the next test)."""
    need_gpu()
    from test_gpu_annotate_frames import _every, _pictures
    s = _every()
    eng = s["eng"]
    sel = [s["shapes"].index(hw) for hw in ((481, 333), (720, 960), (960, 1280), (1080, 1920))]
    ann = eng.annotate(s["dflat"], s["dev"], s["meas"], s["cams"], sel, cameras=s["idx"], table=s["table"])
    data, off = eng.encode_jpeg(ann["buf"], quality=90, table=ann["table"])
    off = off.cpu().numpy()
    files = _files(data.cpu().numpy(), off)
    pics = _pictures(ann["buf"], ann["shapes"], ann["byte_offsets"])
    for k, (b, pic) in enumerate(zip(sel, pics)):
        assert np.array_equal(pic, s["pics"][b])
        d1, o1 = eng.encode_jpeg(torch.from_numpy(np.ascontiguousarray(pic[None])).cuda(), quality=90)
        assert files[k] == d1[:int(o1[1])].cpu().numpy().tobytes(), (b, len(files[k]))


def test_pillow_opens_the_files_of_the_annotated_buffer():
    pytest.importorskip("PIL")
    from PIL import Image
    need_gpu()
    from test_gpu_annotate_frames import _every
    s = _every()
    eng = s["eng"]
    sel = [s["shapes"].index(hw) for hw in ((481, 333), (720, 960), (960, 1280), (1080, 1920))]
    ann = eng.annotate(s["dflat"], s["dev"], s["meas"], s["cams"], sel, cameras=s["idx"], table=s["table"])
    data, off = eng.encode_jpeg(ann["buf"], quality=90, table=ann["table"])
    for k, (b, f) in enumerate(zip(sel, _files(data.cpu().numpy(), off.cpu().numpy()))):
        im = Image.open(io.BytesIO(f))
        im.load()
        assert im.size == s["shapes"][b][::-1] and im.mode == "RGB", b


# ---- the pipeline: mixed-size frames in, annotated JPEG files out -----------------------------------------------------------
PIPE_SIZES = [(960, 1280), (640, 640), (480, 640), (1080, 1920), (1920, 1920), (960, 960), (481, 333), (1200, 1600)]
PIPE_CAMS = [0, 1, 0, 1, 1, 0, 0, 1]
PIPE_KW = dict(conf=0.20, iou=0.25, max_det=200, imgsz=960)


def _strip(rec):
    return {k: v for k, v in rec.items() if k != "timestamp"}


@functools.lru_cache(maxsize=None)
def _model():
    import vti_amd
    from test_gpu_measure_frames import _params
    model = vti_amd.YOLO(None, scale="n", nc=2, seed=3, cls_bias=-1.0)
    return model, [dataclasses.replace(_params(c), drop_empty=False) for c in range(2)]


def _uniform_file(mc, model, frames, b, quality):
    """eng.encode_jpeg of eng.annotate at frame b's size, on the output set the mixed call left behind."""
    (eng, table), = mc._tables.values()
    o, = model._outs.values()
    h, w = frames[b].shape[:2]
    B = len(frames)
    idx = torch.tensor(PIPE_CAMS, dtype=torch.int32, device="cuda")
    uni = dict(o, xyxy=eng.scale_boxes(o["dets"], o["counts"], h, w))
    meas = eng.measure(uni, table, h, w, cameras=idx)
    dense = torch.zeros((B, h, w, 3), dtype=torch.uint8, device="cuda")
    dense[b] = torch.from_numpy(frames[b]).cuda()
    ann = eng.annotate(dense, uni, meas, table, [b], cameras=idx)
    data, off = eng.encode_jpeg(ann["frames"], quality=quality)
    return data[:int(off[1])].cpu().numpy().tobytes(), ann["frames"][0].cpu().numpy()


def test_multi_camera_measurer_annotates_and_encodes_the_mixed_list():
    need_gpu()
    import vti_amd
    model, params = _model()
    frames = [np.random.Generator(np.random.PCG64(k)).integers(0, 256, (h, w, 3), dtype=np.uint8) for k, (h, w) in enumerate(PIPE_SIZES)]
    plain = vti_amd.MultiCameraMeasurer(model, params).process_frames(frames, PIPE_CAMS, **PIPE_KW)
    with pytest.raises(ValueError, match="annotate needs frames of one size"):
        vti_amd.MultiCameraMeasurer(model, params).process_frames(frames, PIPE_CAMS, annotate="all", encode="jpeg", **PIPE_KW)
    mc = vti_amd.MultiCameraMeasurer(model, params)
    annotated, records = mc.process_frames(frames, PIPE_CAMS, annotate="all", encode="jpeg", mixed=True, **PIPE_KW)
    assert [_strip(r) for r in records] == [_strip(r) for r in plain]               # the records are those of the call without annotate
    assert [a[0] for a in annotated] == list(range(8)) and all(isinstance(a[1], bytes) for a in annotated) and model._last_frames is None
    drawn = 0
    for b in range(8):              # every file: 1080 x 1920, 1920 x 1920 and 1200 x 1600 take the global-image tracer, 481 x 333 is the odd one
        want, pic = _uniform_file(mc, model, frames, b, 95)
        assert annotated[b][1] == want, (b, len(annotated[b][1]), len(want))
        assert annotated[b][1][163:167] == bytes([PIPE_SIZES[b][0] >> 8, PIPE_SIZES[b][0] & 255, PIPE_SIZES[b][1] >> 8, PIPE_SIZES[b][1] & 255])
        drawn += int(not np.array_equal(pic, frames[b]))
    print("frames with an overlay:", drawn)
    assert drawn >= 1
    # the bottom line of the text sits at each frame's own H0 - 10
    heights = set()
    for b, _, items in annotated:
        if items and items[-1][0].startswith("Stitches:"):
            assert items[-1][1] == (10, PIPE_SIZES[b][0] - 10), (b, items[-1])
            heights.add(PIPE_SIZES[b][0])
    print("frames with the whole text, by height:", sorted(heights))
    assert len(heights) >= 2, heights
    # without encode: the pictures, each the [H0, W0, 3] array of its frame; a reordered selection with a duplicate
    sel = [6, 2, 6]
    pics, recs2 = vti_amd.MultiCameraMeasurer(model, params).process_frames(frames, PIPE_CAMS, annotate=sel, mixed=True, **PIPE_KW)
    assert [_strip(r) for r in recs2] == [_strip(r) for r in plain] and [p[0] for p in pics] == sel
    for b, pic, items in pics:
        assert pic.shape == frames[b].shape and pic.dtype == np.uint8 and items == annotated[b][2]
        assert jpeg.encode(pic, 95) == annotated[b][1], b                           # 481 x 333 and 480 x 640: cheap on the host
    # mixed=True on frames of one size is mixed=False
    same = [frames[2], frames[2][::-1].copy()]
    a1, r1 = vti_amd.MultiCameraMeasurer(model, params).process_frames(same, [0, 1], annotate="all", encode="jpeg", mixed=True, **PIPE_KW)
    a2, r2 = vti_amd.MultiCameraMeasurer(model, params).process_frames(same, [0, 1], annotate="all", encode="jpeg", **PIPE_KW)
    assert [_strip(r) for r in r1] == [_strip(r) for r in r2] and a1 == a2


def test_the_mixed_list_as_jpeg_files():
    """The same sizes as motion-JPEG input (jpeg.encode at quality 95 makes the files; blocky pictures, which the host encodes quickly):
    the returned files are those of the decoded frames given as arrays."""
    need_gpu()
    import vti_amd
    model, params = _model()
    frames = []
    for k, (h, w) in enumerate(PIPE_SIZES):
        t = np.random.Generator(np.random.PCG64(50 + k)).integers(0, 256, (-(-h // 32), -(-w // 32), 3), dtype=np.uint8)
        frames.append(np.repeat(np.repeat(t, 32, axis=0), 32, axis=1)[:h, :w].copy())
    files = [jpeg.encode(f, 95) for f in frames]
    sel = [4, 6, 1]
    got, recs = vti_amd.MultiCameraMeasurer(model, params).process_frames(files, PIPE_CAMS, annotate=sel, encode="jpeg", mixed=True, **PIPE_KW)
    with torch.inference_mode():                                                    # the decoder's buffers were made under it
        dec, info = model._decode_jpeg(files, rgb=False)
    assert int(info[:, 0].abs().sum()) == 0 and list(dec.shapes) == PIPE_SIZES
    host = dec.buf.cpu().numpy()
    decoded = [host[at:at + 3 * h * w].reshape(h, w, 3).copy() for (h, w), at in zip(dec.shapes, dec.byte_offsets)]
    assert np.array_equal(decoded[6], jpeg.decode(files[6], rgb=False))             # the frames cap.read() would have delivered
    want, recs_w = vti_amd.MultiCameraMeasurer(model, params).process_frames(decoded, PIPE_CAMS, annotate=sel, encode="jpeg", mixed=True,
                                                                             **PIPE_KW)
    assert [_strip(r) for r in recs] == [_strip(r) for r in recs_w]
    assert [g[0] for g in got] == sel and [(g[0], g[2]) for g in got] == [(x[0], x[2]) for x in want]
    for g, x in zip(got, want):
        assert isinstance(g[1], bytes) and g[1] == x[1] and g[1][:2] == b"\xff\xd8", g[0]
        assert g[1][163:167] == bytes([PIPE_SIZES[g[0]][0] >> 8, PIPE_SIZES[g[0]][0] & 255, PIPE_SIZES[g[0]][1] >> 8, PIPE_SIZES[g[0]][1] & 255])
    with pytest.raises(ValueError, match="annotate needs frames of one size"):
        vti_amd.MultiCameraMeasurer(model, params).process_frames(files, PIPE_CAMS, annotate=sel, encode="jpeg", **PIPE_KW)
