"""-m gpu: vti_stamp and vti_stamp_frames (the text of the annotated pictures, painted on the device) against the restatement
annotate.stamp, byte for byte; burn_text through the three process_frames; annotate -> stamp -> encode captured in one graph.
131 x 203 pictures: both dimensions odd, 26593 pixels = three whole 8192-pixel tiles and a part of a fourth, 40.35 rows per tile."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import stamp_util as S
from gpu_util import frames_u8, need_gpu
from vti_amd import annotate as A
from vti_amd import jpeg

pytestmark = pytest.mark.gpu
H, W = 131, 203
POISON = 0xA5
GUARD = 4096


@functools.lru_cache(maxsize=None)
def _engine():
    import vti_amd
    return vti_amd.Engine("n", 2, H=64, W=96, max_batch=4)


@functools.lru_cache(maxsize=None)
def _pictures():
    return frames_u8(3, H, W, 11)


def _want(pictures, per):
    return [A.stamp(p.copy(), s) for p, s in zip(pictures, per)]


def _stamped(per, **pack):
    """vti_stamp on the three random pictures -> (the pictures that came back, the packed table); nothing past them is written."""
    eng = _engine()
    pics = _pictures()
    flat = torch.full((pics.size + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    dev = flat[:pics.size].view(3, H, W, 3)
    dev.copy_(torch.from_numpy(pics))
    packed = eng.pack_stamps(per, [(H, W)] * 3, "cuda", **pack)
    assert eng.stamp(dev, packed) is dev
    torch.cuda.synchronize()
    assert (flat[pics.size:] == POISON).all()
    return dev.cpu().numpy(), packed


def _cases():
    rng = np.random.default_rng(7)
    R = lambda *a, **k: S.random_stamp(rng, *a, **k)
    a, b = R(60, 50, 45, 30, colour=(255, 0, 0), ones=1), R(80, 65, 50, 28, colour=(0, 255, 0))
    dup = R(20, 100, 37, 9)
    small = []
    for i in range(1024):                       # four LDS chunks of 256 records; 30720 stamp pixels on 26593: overlaps everywhere
        small.append(R(int(rng.integers(0, W - 6)), int(rng.integers(0, H - 5)), 6, 5))
    for i in range(0, 1024, 64):                # and the same place again 256, 512 and 768 records later, in other colours
        x, y = small[i][0], small[i][1]
        for later in (256, 512, 768):
            small[(i + later) % 1024] = R(x, y, 6, 5, ones=(later != 512) or None)
    return {
        "corners": [[R(0, 0, 17, 9), R(W - 21, H - 7, 21, 7)], [], [R(0, H - 3, 9, 3), R(W - 5, 0, 5, 11)]],
        "widths": [[R(3 + 7 * k, 10 + 9 * k, w, 5) for k, w in enumerate((1, 31, 32, 33, 64))], [],
                   [R(W - w, 100 + 5 * k, w, 5) for k, w in enumerate((1, 31, 32, 33, 64))]],
        "three_tiles": [[R(30, 10, 90, 100)], [], [R(0, 0, W, H)]],        # rows 10 .. 109 lie in tiles 0, 1 and 2; every tile of a picture
        "overlap_ab": [[a, b], [], [b, a]],
        "overlap_ba": [[b, a], [], [a, b]],
        "duplicate": [[dup, dup], [], [dup, R(25, 102, 37, 9), dup]],
        "zeros_and_ones": [[R(10, 10, 70, 40, ones=0), R(100, 60, 64, 33, ones=1)], [], [R(0, 0, W, H, ones=1)]],
        "many": [small, [], small[::-1]],
        "one_row_one_column": [[R(0, 40, W, 1), R(100, 0, 1, H)], [], [R(W - 1, 0, 1, H), R(0, H - 1, W, 1)]],
    }


CASES = _cases()


@pytest.mark.parametrize("name", list(CASES))
def test_vti_stamp_equals_the_restatement(name):
    need_gpu()
    per = CASES[name]
    got, packed = _stamped(per)
    want = _want(_pictures(), per)
    for k in range(3):
        diff = np.argwhere((got[k] != want[k]).any(axis=-1))
        print(f"{name} picture {k}: {len(per[k])} stamps, {packed.n_words} words, differing pixels {len(diff)}"
              + (f", first at (y, x) {diff[0].tolist()}" if len(diff) else ""))
        assert len(diff) == 0, (name, k, len(diff), diff[:5].tolist())
    assert np.array_equal(got[1], _pictures()[1])                                  # the picture without stamps came back as it was
    assert not np.array_equal(got[0], _pictures()[0])


def test_the_order_of_two_overlapping_stamps_shows():
    need_gpu()
    ab, _ = _stamped(CASES["overlap_ab"])
    ba, _ = _stamped(CASES["overlap_ba"])
    (ax, ay, abits, acol), (bx, by, bbits, bcol) = CASES["overlap_ab"][0]
    both = np.zeros((H, W), bool)                                                   # the pixels that both stamps paint
    both[by:by + bbits.shape[0], bx:bx + bbits.shape[1]] = bbits
    mask = np.zeros((H, W), bool)
    mask[ay:ay + abits.shape[0], ax:ax + abits.shape[1]] = abits
    both &= mask
    assert both.sum() > 100 and acol != bcol
    for first_a, first_b in ((ab[0], ba[0]), (ba[2], ab[2])):                       # a then b shows b's colour there, b then a shows a's
        assert (first_a[both] == bcol).all() and (first_b[both] == acol).all()
        assert np.array_equal(first_a[~both], first_b[~both])


def test_a_wider_pitch_with_garbage_in_the_pad_bits_paints_the_same():
    need_gpu()
    per = CASES["widths"]
    plain, p0 = _stamped(per)
    for extra, fill in ((0, 0xFFFFFFFF), (2, 0xFFFFFFFF), (3, 0x9E3779B9)):
        got, p = _stamped(per, pitch_extra=extra, pad_fill=fill)
        assert p.n_words == p0.n_words + extra * sum(s[2].shape[0] for q in per for s in q)
        assert np.array_equal(got, plain), (extra, hex(fill))
    assert np.array_equal(plain, np.stack(_want(_pictures(), per)))


def test_a_table_without_stamps_changes_nothing():
    need_gpu()
    got, packed = _stamped([[], [], []])
    assert packed.n_stamps == 0 and packed.bits is None and np.array_equal(got, _pictures())


def test_vti_stamp_frames_equals_vti_stamp_per_picture_and_leaves_the_gaps():
    need_gpu()
    eng = _engine()
    shapes = [(37, 53), (64, 96), (8, 8)]
    rng = np.random.default_rng(9)
    R = lambda *a, **k: S.random_stamp(rng, *a, **k)
    per = [[R(0, 0, 33, 5), R(20, 30, 33, 7), R(10, 2, 40, 30), R(52, 0, 1, 37)],
           [R(0, 0, 96, 64, colour=(1, 2, 3)), R(31, 31, 65, 33), R(90, 60, 6, 4)],
           [R(0, 0, 8, 8), R(7, 7, 1, 1, ones=1), R(2, 1, 5, 6)]]
    pics = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    table, offsets, total = eng.pack_frames(shapes, "cuda")
    assert any(offsets[k] + 3 * h * w < (offsets + [total])[k + 1] for k, (h, w) in enumerate(shapes))      # there is a gap to guard
    buf = torch.full((total + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    inside = np.zeros(total + GUARD, bool)
    for (h, w), at, p in zip(shapes, offsets, pics):
        buf[at:at + 3 * h * w] = torch.from_numpy(p.reshape(-1)).cuda()
        inside[at:at + 3 * h * w] = True
    packed = eng.pack_stamps(per, shapes, "cuda")
    flat = buf[:total]
    assert eng.stamp(flat, packed, table=table) is flat
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[~inside] == POISON).all()                                         # the gaps and what lies past the end
    for k, ((h, w), at) in enumerate(zip(shapes, offsets)):
        got = host[at:at + 3 * h * w].reshape(h, w, 3)
        alone = torch.from_numpy(pics[k][None].copy()).cuda()                      # the same picture through vti_stamp at its own size
        eng.stamp(alone, eng.pack_stamps([per[k]], [(h, w)], "cuda"))
        assert np.array_equal(got, alone[0].cpu().numpy()), k
        assert np.array_equal(got, A.stamp(pics[k].copy(), per[k])), k


# ---- burn_text through process_frames ------------------------------------------------------------------------------------------------
def _strip(rec):
    return {k: v for k, v in rec.items() if k != "timestamp"}


@functools.lru_cache(maxsize=None)
def _model():
    import vti_amd
    return vti_amd.YOLO(None, scale="n", nc=2, seed=3, cls_bias=-1.0, dtype="h2")


def _extra(n, shapes):
    """The caller's own lines: one per frame (so that every frame has at least one stamp), the last one clipped by the border."""
    return {b: [S.item(f"status of frame {b}: 12.5 fps", (10, shapes[b][0] - 30), (0, 255, 255), 0.7, 2),
                S.item("frame 30 12", (shapes[b][1] - 20, 5 + b), (255, 255, 255))] for b in range(n)}


def _check_burned(plain, burned, files, extra, shapes, quality):
    """burned = the pictures of the call without burn_text with the returned items stamped on them; files = jpeg.encode of those."""
    painted = 0
    for (b, pic, items), (bb, got, items_b), (bf, data, items_f) in zip(plain, burned, files):
        assert b == bb == bf and items_b == items + extra[b] == items_f
        h, w = shapes[b]
        stamps = A.text_stamps(items_b, h, w, S.rasterise)
        assert len(stamps) >= 2
        want = A.stamp(pic.copy(), stamps)
        diff = int((got != want).any(axis=-1).sum())
        print(f"frame {b} {h}x{w}: {len(items_b)} items, {len(stamps)} stamps, differing pixels {diff}")
        assert got.shape == (h, w, 3) and diff == 0, (b, diff)
        assert isinstance(data, bytes) and data == jpeg.encode(want, quality), (b, len(data))
        painted += int(not np.array_equal(want, pic))
    assert painted == len(plain)


def test_stitch_measurer_burns_the_text_into_pictures_and_files():
    need_gpu()
    import vti_amd
    from test_gpu_annotate import _params
    h, w = 240, 320
    kw = dict(conf=0.20, iou=0.25, max_det=200, imgsz=320, annotate="all")
    frames = frames_u8(3, h, w, 0)
    shapes = [(h, w)] * 3
    extra = _extra(3, shapes)
    base = _params(h, w, "kmeans")
    new = lambda: vti_amd.StitchMeasurer(_model(), base)
    plain, recs = new().process_frames(frames, **kw)
    burned, recs_b = new().process_frames(frames, burn_text=True, extra_text=extra, rasterise=S.rasterise, **kw)
    files, recs_f = new().process_frames(frames, burn_text=True, extra_text=extra, rasterise=S.rasterise, encode="jpeg", jpeg_quality=90, **kw)
    assert [_strip(r) for r in recs] == [_strip(r) for r in recs_b] == [_strip(r) for r in recs_f]
    assert _model()._last_frames is None
    _check_burned(plain, burned, files, extra, shapes, 90)


def test_multi_camera_measurer_burns_the_text_into_frames_of_two_sizes():
    need_gpu()
    import vti_amd
    from test_gpu_annotate import _params
    shapes = [(240, 320), (180, 260), (240, 320)]
    frames = [frames_u8(1, h, w, 20 + k)[0] for k, (h, w) in enumerate(shapes)]
    cams, sel = [1, 0, 1], [2, 0, 1]
    extra = _extra(3, shapes)
    kw = dict(conf=0.20, iou=0.25, max_det=200, imgsz=320, annotate=sel, mixed=True)
    plist = [_params(240, 320, "kmeans", k) for k in range(2)]
    new = lambda: vti_amd.MultiCameraMeasurer(_model(), plist)
    plain, recs = new().process_frames(frames, cams, **kw)
    burned, recs_b = new().process_frames(frames, cams, burn_text=True, extra_text=extra, rasterise=S.rasterise, **kw)
    files, recs_f = new().process_frames(frames, cams, burn_text=True, extra_text=extra, rasterise=S.rasterise, encode="jpeg", **kw)
    assert [_strip(r) for r in recs] == [_strip(r) for r in recs_b] == [_strip(r) for r in recs_f]
    assert [a[0] for a in burned] == sel
    _check_burned(plain, burned, files, extra, shapes, 95)


def test_stitch_distance_checker_burns_the_text_into_pictures_and_files():
    need_gpu()
    import vti_amd
    from test_oracle_geometry import load_calib
    h, w = 240, 320
    frames = frames_u8(2, h, w, 5)
    shapes = [(h, w)] * 2
    extra = _extra(2, shapes)
    kw = dict(imgsz=320, annotate=[1, 0])
    new = lambda: vti_amd.StitchDistanceChecker(_model(), vti_amd.CheckerParams(*load_calib()))
    plain, recs = new().process_frames(frames, **kw)
    burned, recs_b = new().process_frames(frames, burn_text=True, extra_text=extra, rasterise=S.rasterise, **kw)
    seen = {}                                   # the callable form gets the record of the very call: it returns the same lines here
    files, recs_f, rows = new().process_frames(frames, burn_text=True, extra_text=lambda b, rec: seen.setdefault(b, rec) and extra[b],
                                               rasterise=S.rasterise, encode="jpeg", rows=True, **kw)
    assert {b: _strip(r) for b, r in seen.items()} == {b: _strip(recs_f[b]) for b in (0, 1)}
    assert [_strip(r) for r in recs] == [_strip(r) for r in recs_b] == [_strip(r) for r in recs_f] and len(rows) == 2
    _check_burned(plain, burned, files, extra, shapes, 95)


# ---- annotate -> stamp -> encode in one graph ----------------------------------------------------------------------------------------
def test_annotate_stamp_and_encode_replay_from_one_graph():
    """The three calls through the C ABI on preallocated buffers, once eagerly and once captured and replayed: the same pictures and
    the same files.  A capture fails on any synchronisation or allocation inside it."""
    need_gpu()
    import annotate_util as U
    from test_gpu_annotate import _batch, _params
    from test_gpu_measure import _engine as measure_engine
    import vti_amd
    L = vti_amd.lib()
    mode, h, w, mh, mw = U.MODES[2]                                                 # native rows, 481 x 333
    eng = measure_engine(736, 960, 16)
    native, dev, ref, offsets, cap, frames, dframes = _batch(U.scenes()[:4], mode, h, w, mh, mw, seed=8)
    B = len(ref)
    p = _params(h, w, "kmeans")
    meas = eng.measure(dev, p, h, w, native=native)
    sel = np.arange(B, dtype=np.int32)
    dsel = torch.from_numpy(sel).cuda()
    cams = eng.pack_cameras([p], "cuda")
    items = [[S.item(f"Edge Dist: {b}.25mm | Avg Width: 4.10mm", (10, 30), (0, 0, 255), 0.7, 2), S.item("rect 300 9", (w - 150, h - 12), (9, 9, 9))]
             for b in range(B)]
    packed = eng.pack_stamps([A.text_stamps(it, h, w, S.rasterise) for it in items], [(h, w)] * B, "cuda")
    a_need = eng.annotate_scratch_bytes(B, dev["dets"].shape[1], h, w, U.MAX_POINTS)
    j_need = eng.encode_jpeg_scratch_bytes(B, h, w)
    a_ws = torch.empty(a_need + 256, dtype=torch.uint8, device="cuda")
    j_ws = torch.empty(j_need + 256, dtype=torch.uint8, device="cuda")
    al = lambda t: C.c_void_p((t.data_ptr() + 255) & ~255)
    room = 3 * B * h * w + 1024 * B
    P = lambda t: C.c_void_p(t.data_ptr())

    def run(pics, status, files, off, stream):
        st = C.c_void_p(stream.cuda_stream)
        rc = L.vti_annotate(eng._ctx, P(dframes), B, h, w, P(cams), 1, None, P(dev["masks"]), int(native), P(dev["dets"]), P(dev["xyxy"]),
                            P(dev["counts"]), P(dev["offsets"]), dev["dets"].shape[1], dev["masks"].shape[0], P(meas["frame_i32"]),
                            P(meas["stitch_f64"]), P(meas["stitch_i32"]), C.c_void_p(sel.ctypes.data), P(dsel), B, U.MAX_POINTS, P(pics),
                            P(status), al(a_ws), a_need, st)
        rc = rc or L.vti_stamp(eng._ctx, P(pics), B, h, w, P(packed.host), P(packed.dev), P(packed.bits), packed.n_words, st)
        rc = rc or L.vti_encode_jpeg(eng._ctx, P(pics), B, h, w, 0, 95, al(j_ws), j_need, P(off), P(files), room, st)
        assert rc == 0, (rc, L.vti_last_error(eng._ctx))

    new = lambda: (torch.full((B, h, w, 3), POISON, dtype=torch.uint8, device="cuda"), torch.full((B,), -7, dtype=torch.int32, device="cuda"),
                   torch.full((room,), POISON, dtype=torch.uint8, device="cuda"), torch.zeros(B + 1, dtype=torch.int64, device="cuda"))
    eager, graphed = new(), new()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(*eager, s)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        run(*graphed, s)
    for t, v in zip(graphed, (POISON, -7, POISON, 0)):
        t.fill_(v)                                                                  # what the capture may have left is gone
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    for e, r in zip(eager, graphed):
        assert torch.equal(e, r)
    pics, status, files, off = (t.cpu().numpy() for t in graphed)
    assert status.tolist() == [0] * B and off[0] == 0 and off[-1] <= room
    plain = eng.annotate(dframes, dev, meas, p, sel.tolist(), native=native)["frames"].cpu().numpy()
    for b in range(B):
        want = A.stamp(plain[b].copy(), A.text_stamps(items[b], h, w, S.rasterise))
        assert not np.array_equal(want, plain[b]) and np.array_equal(pics[b], want), b
    assert bytes(files[off[0]:off[1]]) == jpeg.encode(pics[0], 95)
