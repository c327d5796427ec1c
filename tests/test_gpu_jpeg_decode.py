"""-m gpu: vti_decode_jpeg (JPEG files -> frames on the device) against the host specification jpeg.decode, byte for byte.
jpeg.decode itself is held to libjpeg's pixels on the CPU (tests/test_jpeg_decode.py).  Every comparison runs with dev_out and the
scratch poisoned, a guard band after dev_out and in the alignment gaps, and dev_files compared afterwards."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import jpeg_decode_util as U
import jpeg_util as J
from gpu_util import need_gpu
from vti_amd import jpeg

pytestmark = pytest.mark.gpu
POISON = 0xA5
GUARD = 4096
SIZES = J.SIZES + [(480, 640)]
QUALITIES = (95, 100, 10)
CORRUPT = 1


def _contents(h, w):
    # n = 3 different contents per call; the one large shape takes contents whose host reference decodes quickly
    return ("flat", "smooth", "checker") if h * w > 135 * 241 else ("noise", "ramp", "tiles")


def _frame(content, h, w):
    if content == "smooth":
        yy, xx = np.mgrid[:h, :w]
        return np.stack([(xx // 3 + yy // 5) % 256, (xx // 4) % 256, (255 - yy // 2) % 256], axis=2).astype(np.uint8)
    return J.frame(content, h, w)


@functools.lru_cache(maxsize=None)
def _file(content, h, w, q, ss, restart=0, with_dht=True):
    return U.own_file(_frame(content, h, w), q, ss, restart, with_dht)


@functools.lru_cache(maxsize=None)
def _want_of(data):
    a = jpeg.decode(data)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _engine():
    import vti_amd
    return vti_amd.Engine("n", 2, H=64, W=64, max_batch=1)


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_decode_pillow.npz")) as z:
        return {k: z[k] for k in z.files if k != "pillow_version"}


def _raw(files, segment_bytes=0, rgb=1, layout=0, dev_files=None):
    """vti_decode_jpeg through the C ABI -> (frames [u8 H0 x W0 x 3], info [n, 4]); checks the guard bands and dev_files."""
    import vti_amd
    L = vti_amd.lib()
    eng = _engine()
    rc, p = U.plan(vti_amd, list(files), segment_bytes, layout, ctx=eng._ctx)
    assert rc == 0, p["error"]
    n, total, need = len(files), int(p["out_off"][-1]), p["scratch_bytes"]
    dfiles = torch.from_numpy(p["blob"]).cuda() if dev_files is None else dev_files
    before = dfiles.clone()
    dtable = torch.from_numpy(p["table"]).cuda()
    ws = torch.full((need + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    out = torch.full((total + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    info = torch.full((n, 4), -7, dtype=torch.int32, device="cuda")
    rc = L.vti_decode_jpeg(eng._ctx, C.c_void_p(dfiles.data_ptr()), C.c_void_p(p["table"].ctypes.data), C.c_void_p(dtable.data_ptr()), n, rgb,
                           C.c_void_p(out.data_ptr()), total, C.c_void_p(info.data_ptr()), C.c_void_p(ws.data_ptr()), need,
                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.vti_last_error(eng._ctx)
    torch.cuda.synchronize()
    assert torch.equal(dfiles, before)                               # dev_files is read only
    out, ws = out.cpu().numpy(), ws.cpu().numpy()
    assert (out[total:] == POISON).all() and (ws[need:] == POISON).all()
    frames, written = [], np.zeros(total, bool)
    for k in range(n):
        a, m = int(p["out_off"][k]), 3 * int(p["H0"][k]) * int(p["W0"][k])
        frames.append(out[a:a + m].reshape(p["H0"][k], p["W0"][k], 3))
        written[a:a + m] = True
    assert (out[:total][~written] == POISON).all()                   # the alignment gaps of layout 0
    return frames, info.cpu().numpy()


def _check(files, frames, info, rgb=1, label=""):
    for k, (f, got) in enumerate(zip(files, frames)):
        want = _want_of(f) if rgb else _want_of(f)[..., ::-1]
        assert info[k, 0] == 0 and info[k, 3] == jpeg.parse(f)["n_blocks"], (label, k, info[k])
        bad = np.argwhere((got != want).any(-1))
        assert got.shape == want.shape and not len(bad), (label, k, len(bad), bad[:4].tolist(), info[k].tolist())


@pytest.mark.parametrize("ss", list(U.SAMPLINGS))
@pytest.mark.parametrize("h,w", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_every_frame_equals_the_host_specification(h, w, ss):
    need_gpu()
    for q in QUALITIES:
        files = [_file(c, h, w, q, ss) for c in _contents(h, w)]
        frames, info = _raw(files)                                   # layout 0: frames at multiples of 16 bytes
        print(f"{h}x{w} {ss} q={q}: bytes {[len(f) for f in files]} segments {info[:, 1].tolist()} rounds {info[:, 2].tolist()}")
        _check(files, frames, info, label=(h, w, ss, q))
        dense, info = _raw(files, layout=1, rgb=0)                   # dense, BGR
        _check(files, dense, info, rgb=0, label=(h, w, ss, q, "dense bgr"))


def test_one_call_mixes_sizes_and_samplings():
    need_gpu()
    files = [_file("noise", 135, 241, 95, "422"), _file("ramp", 1, 1, 95, "444"), _file("tiles", 17, 33, 10, "420"),
             _file("smooth", 480, 640, 95, "420"), _file("ramp", 50, 70, 100, "444", 3), _file("noise", 8, 8, 95, "422", 0, False),
             _file("checker", 16, 16, 95, "420")]
    for rgb in (1, 0):
        frames, info = _raw(files, rgb=rgb)
        _check(files, frames, info, rgb=rgb, label=("mixed", rgb))


def _hard_files():
    g = _golden()
    return {
        # blocks several segments long: nearly every 16-byte segment starts mid-block, the entry states travel many rounds
        "noise 135x241 q100": _file("noise", 135, 241, 100, "444"),
        # hundreds of blocks per segment: the block-count scan
        "flat 480x640": _file("flat", 480, 640, 95, "420"),
        "smooth 480x640": _file("smooth", 480, 640, 95, "422"),
        "restart every MCU": _file("ramp", 50, 70, 95, "420", 1),
        "restart every 7 MCUs, no DHT": _file("noise", 50, 70, 95, "444", 7, False),
        "Pillow restart rows (RSTn wraps)": g["file_checker_135x241_420_q50_rr1"].tobytes(),
        "Pillow restart blocks": g["file_noise_17x33_422_q95_rb2"].tobytes(),
        "Pillow optimised tables": g["file_ramp_50x70_422_q95_opt"].tobytes(),
        "Pillow optimised tables, noise q100": g["file_noise_17x33_444_q100_opt"].tobytes(),
        "Pillow file without DHT": g["file_ramp_50x70_444_q95_nodht"].tobytes(),
        "scan shorter than one segment": _file("flat", 1, 1, 95, "420"),
    }


@pytest.mark.parametrize("segment_bytes", [16, 0])
def test_segment_sizes_on_the_hard_inputs(segment_bytes):
    need_gpu()
    hard = _hard_files()
    files = list(hard.values())
    assert len(files[-1]) - jpeg.parse(files[-1])["scan_start"] - 2 < 16
    frames, info = _raw(files, segment_bytes)
    for name, row in zip(hard, info):
        print(f"segment_bytes {segment_bytes or 256}: {name}: segments {row[1]} rounds {row[2]} blocks {row[3]}")
    _check(files, frames, info, label=segment_bytes)
    if segment_bytes == 16:
        assert info[0, 1] > 1000 and info[0, 2] > 100          # the states did travel
        assert info[1, 1] * 16 < jpeg.parse(files[1])["n_blocks"]     # many blocks per segment


def test_a_files_pixels_do_not_depend_on_its_batch_position():
    need_gpu()
    a, b = _file("noise", 50, 70, 95, "420"), _file("ramp", 135, 241, 95, "422", 4)
    frames, info = _raw([a, b, a])
    assert np.array_equal(frames[0], frames[2])
    _check([a, b, a], frames, info)


def test_damaged_scans_set_the_status_and_stay_inside_their_frame():
    """Inputs the decoder must survive: the scan ends, stays in its buffers (the guard bands are checked by _raw) and reports."""
    need_gpu()
    good, rst = _file("ramp", 50, 70, 95, "420"), _file("noise", 50, 70, 95, "422", 2)
    hdr = jpeg.parse(good)
    mid = (hdr["scan_start"] + hdr["scan_end"]) // 2
    junk = bytes(np.random.Generator(np.random.PCG64(3)).integers(1, 255, 60, dtype=np.uint8))
    at = rst.index(b"\xff\xd2", jpeg.parse(rst)["scan_start"])
    damaged = [good[:mid], good[:mid] + junk + good[mid + 60:], good[:mid] + bytes(40) + good[mid + 40:], rst[:at + 1] + b"\xd5" + rst[at + 2:],
               rst[:at] + rst[at + 2:]]
    for seg in (16, 0):
        files = [good, damaged[0], rst, damaged[1], damaged[2], damaged[3], damaged[4], good]
        frames, info = _raw(files, seg)
        assert info[:, 0].tolist() == [0, CORRUPT, 0, CORRUPT, CORRUPT, CORRUPT, CORRUPT, 0], (seg, info.tolist())
        for k in (0, 2, 7):                                           # the other files of the same batch are still exact
            assert np.array_equal(frames[k], _want_of(files[k])), (seg, k)


def test_round_trip_of_the_devices_own_files():
    need_gpu()
    import vti_amd
    eng = _engine()
    h, w = 135, 241
    batch = np.stack([J.frame(c, h, w) for c in ("noise", "ramp", "tiles")])
    data, off = eng.encode_jpeg(torch.from_numpy(batch).cuda(), quality=90)
    off = off.cpu().numpy()
    host = data[:off[-1]].cpu().numpy().tobytes()
    files = [host[off[k]:off[k + 1]] for k in range(3)]
    assert files == [jpeg.encode(f, 90) for f in batch]
    frames, info = _raw(files, rgb=0, dev_files=data[:off[-1] + 1])  # the encoder's device buffer feeds the decoder directly
    _check(files, frames, info, rgb=0)
    # ... and through the Engine wrappers
    dec, info = eng.decode_jpeg(files, rgb=False)
    assert tuple(dec.shape) == (3, h, w, 3) and dec.is_cuda and int(info[:, 0].abs().sum()) == 0
    for k in range(3):
        assert np.array_equal(dec[k].cpu().numpy(), _want_of(files[k])[..., ::-1])
    buf, shapes, offs, info = eng.decode_jpeg([files[0], _file("ramp", 17, 33, 95, "444")], rgb=True)
    assert shapes == [(h, w), (17, 33)] and offs == [0, (3 * h * w + 15) & ~15] and buf.dim() == 1
    assert np.array_equal(buf[offs[1]:offs[1] + 3 * 17 * 33].cpu().numpy().reshape(17, 33, 3), _want_of(_file("ramp", 17, 33, 95, "444")))


def _same_results(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.orig_shape == y.orig_shape and len(x) == len(y)
        assert x.boxes.data.cpu().numpy().tobytes() == y.boxes.data.cpu().numpy().tobytes()
        assert (x.masks is None) == (y.masks is None)
        if x.masks is not None:
            assert x.masks.bits.cpu().numpy().tobytes() == y.masks.bits.cpu().numpy().tobytes()


def test_predict_takes_jpeg_bytes_and_paths(tmp_path):
    need_gpu()
    import vti_amd
    model = vti_amd.YOLO(None, scale="n", nc=2, seed=3, cls_bias=-1.0, dtype="h2")
    kw = dict(max_det=50, imgsz=640)
    equal = [_file("smooth", 480, 640, 95, "420"), _file("checker", 480, 640, 95, "422"), _file("flat", 480, 640, 95, "444")]
    got = model.predict(equal, **kw)
    want = model.predict(np.stack([_want_of(f) for f in equal]), swap_rb=False, **kw)
    assert all(r.orig_shape == (480, 640) for r in got) and sum(len(r) for r in got) >= 1
    _same_results(got, want)
    path = tmp_path / "frame.jpg"
    path.write_bytes(equal[1])
    _same_results(model.predict(str(path), **kw), want[1:2])
    _same_results(model.predict(equal[0], **kw), want[:1])
    mixed = [equal[0], _file("noise", 135, 241, 95, "422"), _file("ramp", 50, 70, 95, "444", 3), path]
    got = model.predict(mixed, **kw)
    want = model.predict([_want_of(f) for f in mixed[:3]] + [_want_of(equal[1])], swap_rb=False, **kw)
    assert [r.orig_shape for r in got] == [(480, 640), (135, 241), (50, 70), (480, 640)]
    _same_results(got, want)
    # a refused file raises before any launch, a damaged one after the call, naming its index
    with pytest.raises(vti_amd.VtiError, match="file 1"):
        model.predict([equal[0], b"\xff\xd8 not a jpeg"], **kw)
    hdr = jpeg.parse(equal[0])
    with pytest.raises(ValueError, match="file 1 is damaged"):
        model.predict([equal[1], equal[0][:(hdr["scan_start"] + hdr["scan_end"]) // 2]], **kw)


def _strip(rec):
    return {k: v for k, v in rec.items() if k != "timestamp"}


def test_stitch_measurer_takes_jpeg_bytes():
    need_gpu()
    import vti_amd
    from test_gpu_annotate import _params
    h, w = 480, 640
    kw = dict(conf=0.20, iou=0.25, max_det=200, imgsz=640)
    files = [_file("smooth", h, w, 95, "420"), _file("checker", h, w, 95, "422"), _file("flat", h, w, 95, "444")]
    model = vti_amd.YOLO(None, scale="n", nc=2, seed=3, cls_bias=-1.0, dtype="h2")
    base = _params(h, w, "kmeans")
    got = vti_amd.StitchMeasurer(model, base).process_frames(files, **kw)
    want = vti_amd.StitchMeasurer(model, base).process_frames(np.stack([_want_of(f)[..., ::-1] for f in files]), **kw)
    assert [_strip(r) for r in got] == [_strip(r) for r in want] and len(got) == 3
    plist = [_params(h, w, "kmeans", k) for k in range(2)]
    got = vti_amd.MultiCameraMeasurer(model, plist).process_frames(files, [1, 0, 1], **kw)
    want = vti_amd.MultiCameraMeasurer(model, plist).process_frames(np.stack([_want_of(f)[..., ::-1] for f in files]), [1, 0, 1], **kw)
    assert [_strip(r) for r in got] == [_strip(r) for r in want]
