"""-m gpu: vti_overlay_frames -- the model-check viewer's picture of the selected frames of a batch whose frames differ in size, each
at its own size.  The main oracle is vti_overlay itself: every picture and status word is compared byte for byte with vti_overlay
run at that frame's size on the same inputs (letterbox masks: the same output set; ragged native rows: that frame's live slots as a
uniform [n, H0, row_bytes] buffer), in DRAW, BLEND and BOTH.  The restatement overlay.render is the second oracle on the small frames
and on the 960 x 1280 one (the Python rasteriser costs about a second per full-size frame).

One selection holds: 40 x 50 (below one 8192-pixel raster tile: the tile grid of the largest frame has idle workgroups), 120 x 203
(a non-integer stretch on both axes, a width that is no multiple of 16 or 64, tiles split mid-row), 481 x 333 (3 * 481 * 333 is no
multiple of 16: the next picture starts at a padded offset behind a gap; row_bytes 48 against the 32 of a 203-wide frame),
960 x 1280 (the tracer's LDS form) and 1040 x 1280 (its global form: the call takes both contour launches)."""
import functools

import numpy as np
import pytest
import torch

import annotate_util as U
from gpu_util import need_gpu
from test_gpu_measure import scenes, unpack
from test_gpu_measure_frames_native import build_ragged
from test_gpu_overlay import MH, MW, _eng, _scene_list, overlap_scene
from vti_amd import jpeg
from vti_amd import overlay as O

pytestmark = pytest.mark.gpu
POISON = 0xA5
GUARD = 4096
TINY, SMALL, ODD, LDS, GLOBAL = (40, 50), (120, 203), (481, 333), (960, 1280), (1040, 1280)
MODES = ((O.DRAW, "draw"), (O.BLEND, "blend"), (O.BOTH, "both"))
DEAD = 3                                            # instances of the last frame without a mask (past the capacity / cut off)
FORMS = ["letterbox", "native"]


def plan():
    """(scene, (h, w)) per frame; the last frame's last DEAD instances have no mask."""
    s = scenes()
    some = _scene_list("some")
    return [(s[0], TINY), (overlap_scene(), SMALL), (s[4], ODD), (overlap_scene(), LDS), (some[6], SMALL), (overlap_scene(), GLOBAL),
            (s[11], TINY), (s[5], ODD)]


def _flat(frames, table):
    flat = np.zeros(table.total_bytes, np.uint8)
    for f, at in zip(frames, table.byte_offsets):
        flat[at:at + f.size] = f.reshape(-1)
    return flat


def _pictures(host, shapes, offsets):
    return [host[at:at + 3 * h * w].reshape(h, w, 3) for (h, w), at in zip(shapes, offsets)]


def _rand_frames(shapes, seed):
    return [np.random.Generator(np.random.PCG64(seed * 100 + b)).integers(0, 256, (h, w, 3), dtype=np.uint8) for b, (h, w) in enumerate(shapes)]


def build_letterbox(pl, dead):
    """annotate_util.host_batch per frame (each at its own size, all on the engine's 96 x 160 mask canvas), joined into one output set."""
    parts = [U.host_batch([scene], h, w, MH, MW, False, dead=0, seed=b + 1) for b, (scene, (h, w)) in enumerate(pl)]
    counts = np.array([len(scene) for scene, _ in pl], np.int32)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    cap = int(offsets[-1]) - dead
    arr = dict(dets=np.concatenate([p[0]["dets"] for p in parts]), xyxy=np.concatenate([p[0]["xyxy"] for p in parts]), counts=counts,
               offsets=offsets, masks=np.ascontiguousarray(np.concatenate([p[0]["masks"] for p in parts])[:cap]))
    ref = []
    for b, p in enumerate(parts):
        cls, boxes, ms = p[1][0]
        ref.append((cls, boxes, [m if offsets[b] + i < cap else None for i, m in enumerate(ms)]))
    return {k: torch.from_numpy(v).cuda() for k, v in arr.items()}, ref, offsets, cap


def _setup(form, pl, dead=DEAD, seed=5):
    """-> the batch: engine, output set, frame table, flat frames, per-frame reference (cls, boxes, masks or None), keyword arguments of
    the frames call and, per frame, the output set of the uniform call that serves as its oracle."""
    eng = _eng()
    shapes = [hw for _, hw in pl]
    B = len(pl)
    if form == "letterbox":
        dev, ref, offsets, cap = build_letterbox(pl, dead)
        table, _, _ = eng.pack_frames(shapes, "cuda")
        kw = dict(native=False)
        n_live = [max(0, min(len(ref[b][0]), cap - int(offsets[b]))) for b in range(B)]
        full = None
    else:
        last = len(pl[-1][0])
        cut = (B - 1, last - dead, 100)             # capacity_bytes ends inside the last frame's run, off a slot boundary
        dev, table, ref, offsets, bases, slot, capacity_bytes, live_slots = build_ragged(eng, [(s, hw, 0) for s, hw in pl], cut)
        kw = dict(native=True, capacity_bytes=capacity_bytes)
        n_live = [max(0, min(len(ref[b][0]), live_slots - int(offsets[b]))) for b in range(B)]
        full = dev["masks"]
        assert full.numel() > capacity_bytes and (full[capacity_bytes:] == 0xFF).all()      # the poisoned tail of the mask buffer
    frames = _rand_frames(shapes, seed)
    flat = _flat(frames, table)
    s = dict(eng=eng, form=form, shapes=shapes, dev=dev, ref=ref, offsets=offsets, table=table, kw=kw, frames=frames, flat=flat,
             dflat=torch.from_numpy(flat).cuda(), n_live=n_live, plan=pl, B=B)
    if form == "native":
        s.update(bases=bases, full=full)
    return s


def _uniform(s, b, mode, annotated=None, max_points=U.MAX_POINTS):
    """vti_overlay at frame b's size on the same inputs -> (picture, status word)."""
    eng, dev = s["eng"], s["dev"]
    h, w = s["shapes"][b]
    ann = torch.from_numpy(annotated[None].copy()).cuda() if annotated is not None else None
    if s["form"] == "letterbox":                    # the same output set; the other frames of the dense batch are never read
        dense = torch.zeros((s["B"], h, w, 3), dtype=torch.uint8, device="cuda")
        dense[b] = torch.from_numpy(s["frames"][b]).cuda()
        one = eng.overlay(dense, dev, [b], native=False, mode=mode, annotated=ann, max_points=max_points)
    else:                                           # frame b's live slots as a uniform [n, H0, row_bytes] buffer
        n = len(s["ref"][b][0])
        view = dict(dets=dev["dets"][b:b + 1], xyxy=dev["xyxy"][b:b + 1], counts=dev["counts"][b:b + 1],
                    offsets=torch.tensor([0, n], dtype=torch.int32, device="cuda"),
                    masks=s["eng"].frame_masks(s["full"], s["table"], b, int(s["bases"][b]), s["n_live"][b]))
        dense = torch.from_numpy(s["frames"][b][None].copy()).cuda()
        one = eng.overlay(dense, view, [0], native=True, mode=mode, annotated=ann, max_points=max_points)
    return one["frames"][0].cpu().numpy(), int(one["status"][0])


@functools.lru_cache(maxsize=None)
def _every(form):
    """The batch and the all-frames call in each mode on a poisoned output, guard and scratch: computed once, shared, never changed."""
    s = _setup(form, plan())
    eng, B = s["eng"], s["B"]
    sel = list(range(B))
    first = eng.overlay(s["dflat"], s["dev"], sel, table=s["table"], **s["kw"])             # allocates the scratch
    total = first["table"].total_bytes
    pictures = np.random.Generator(np.random.PCG64(77)).integers(0, 256, total, dtype=np.uint8)     # BLEND's dev_annotated: any picture
    dpictures = torch.from_numpy(pictures).cuda()
    s.update(sel=sel, total=total, pictures=pictures, dpictures=dpictures, out={}, pics={}, status={})
    for m, name in MODES:
        eng._overlay_ws.fill_(POISON)
        out = torch.full((total + GUARD,), POISON, dtype=torch.uint8, device="cuda")
        res = dict(buf=out[:total], status=torch.full((B,), -7, dtype=torch.int32, device="cuda"))
        got = eng.overlay(s["dflat"], s["dev"], sel, mode=name, annotated=dpictures if m == O.BLEND else None, max_points=U.MAX_POINTS,
                          table=s["table"], result=res, **s["kw"])
        torch.cuda.synchronize()
        assert got["buf"].data_ptr() == out.data_ptr() and got["shapes"] == s["shapes"]
        s["out"][m] = out.cpu().numpy()
        s["pics"][m] = _pictures(s["out"][m], got["shapes"], got["byte_offsets"])
        s["status"][m] = got["status"].cpu().tolist()
        s["byte_offsets"] = got["byte_offsets"]
    s["annotated"] = _pictures(pictures, s["shapes"], s["byte_offsets"])
    return s


def test_the_batch_crosses_every_per_frame_decision():
    need_gpu()
    s = _every("letterbox")
    assert sorted(set(s["shapes"])) == sorted([TINY, SMALL, ODD, LDS, GLOBAL])
    assert 3 * TINY[0] * TINY[1] < 3 * 8192 and (3 * 481 * 333) % 16 != 0
    offs = s["byte_offsets"]
    gaps = [offs[k + 1] - (offs[k] + 3 * h * w) for k, (h, w) in enumerate(s["shapes"][:-1])]
    assert max(gaps) > 0 and all(at % 16 == 0 for at in offs)
    assert 8 * 960 * -(-1280 // 64) <= 156 * 1024 < 8 * 1040 * -(-1280 // 64)      # the tracer's LDS image: fits / does not fit
    assert 8 * -(-333 // 64) == 48 and 8 * -(-203 // 64) == 32
    n = _every("native")
    assert n["n_live"][-1] == len(n["ref"][-1][0]) - DEAD and s["n_live"][-1] == len(s["ref"][-1][0]) - DEAD


@pytest.mark.parametrize("form", FORMS)
def test_every_picture_and_status_equals_vti_overlay_at_that_frames_size(form):
    need_gpu()
    s = _every(form)
    bad = 0
    for b, (h, w) in enumerate(s["shapes"]):
        for m, name in MODES:
            want, word = _uniform(s, b, name, annotated=s["annotated"][b] if m == O.BLEND else None)
            diff = int((s["pics"][m][b] != want).any(axis=-1).sum())
            print(f"{form} frame {b} {h}x{w} mode {name}: status {s['status'][m][b]} / {word}, differing pixels {diff}")
            bad += diff + (s["status"][m][b] != word)
        assert not np.array_equal(s["pics"][O.BOTH][b], s["frames"][b])                    # every frame is drawn on
    assert bad == 0
    assert all(st == [0] * s["B"] for st in s["status"].values())


@pytest.mark.parametrize("form", FORMS)
def test_the_small_frames_and_the_lds_frame_equal_the_restatement(form):
    need_gpu()
    s = _every(form)
    checked = set()
    for b, (h, w) in enumerate(s["shapes"]):
        if (h, w) == GLOBAL or ((h, w) == SMALL and len(s["ref"][b][0]) > 100):            # the 201-instance scene: device against device only
            continue
        cls, boxes, ms = s["ref"][b]
        draw, word = O.render(s["frames"][b], cls, boxes, ms, mode=O.DRAW, max_points=U.MAX_POINTS, with_status=True)
        blend = O.render(s["frames"][b], cls, boxes, ms, mode=O.BLEND, annotated=s["annotated"][b])
        both = O.render(s["frames"][b], cls, boxes, ms, mode=O.BLEND, annotated=draw)      # BOTH = BLEND of DRAW (test_overlay.py pins it)
        for m, want in ((O.DRAW, draw), (O.BLEND, blend), (O.BOTH, both)):
            diff = np.argwhere((s["pics"][m][b] != want).any(axis=-1))
            print(f"{form} frame {b} {h}x{w} mode {m}: differing pixels {len(diff)}" + (f" first at (y, x) {diff[0].tolist()}" if len(diff) else ""))
            assert len(diff) == 0 and word == s["status"][m][b] == 0, (b, m)
        checked.add((h, w))
    assert checked == {TINY, SMALL, ODD, LDS}
    # the last frame's DEAD instances have no mask: no tint, no contour (the restatement got None for them), their boxes are drawn;
    # with native rows whatever lies past capacity_bytes (0xFF all over) was not read
    cls, boxes, ms = s["ref"][-1]
    assert [m is None for m in ms][-DEAD:] == [True] * DEAD and ms[-DEAD - 1] is not None
    boxes_only = O.render(s["frames"][-1], cls[-DEAD:], boxes[-DEAD:], [None] * DEAD, mode=O.DRAW)
    assert not np.array_equal(boxes_only, s["frames"][-1])
    changed = (boxes_only != s["frames"][-1]).any(axis=-1)
    later = O.render(s["frames"][-1], cls, boxes, ms, mode=O.DRAW)
    assert np.array_equal(s["pics"][O.DRAW][-1][changed], later[changed])


@pytest.mark.parametrize("form", FORMS)
def test_only_the_pictures_are_written(form):
    need_gpu()
    s = _every(form)
    total, offs = s["total"], s["byte_offsets"]
    for m, _ in MODES:
        out = s["out"][m]
        assert (out[total:] == POISON).all() and len(out) == total + GUARD                 # the guard behind the last picture
        end = gap_bytes = 0
        for (h, w), at in zip(s["shapes"], offs):
            assert (out[end:at] == POISON).all(), (m, end, at)                              # the gap in front of this picture
            gap_bytes += at - end
            end = at + 3 * h * w
        assert (out[end:total] == POISON).all() and gap_bytes > 0
    assert np.array_equal(s["dflat"].cpu().numpy(), s["flat"])                              # dev_frames is read only
    assert np.array_equal(s["dpictures"].cpu().numpy(), s["pictures"])                      # and so is BLEND's picture


@pytest.mark.parametrize("form", FORMS)
def test_both_is_blend_of_draw_and_blend_may_write_over_its_picture(form):
    need_gpu()
    s = _every(form)
    eng, total = s["eng"], s["total"]
    draw = torch.from_numpy(s["out"][O.DRAW][:total].copy()).cuda()
    both = torch.from_numpy(s["out"][O.BOTH][:total].copy()).cuda()
    blend = eng.overlay(s["dflat"], s["dev"], s["sel"], mode="blend", annotated=draw, table=s["table"], **s["kw"])["buf"]
    for k, ((h, w), at) in enumerate(zip(s["shapes"], s["byte_offsets"])):                 # (the gaps of a fresh buffer hold anything)
        assert torch.equal(blend[at:at + 3 * h * w], both[at:at + 3 * h * w]), k
    assert not torch.equal(both, draw)
    # dev_out is the very buffer dev_annotated points to
    alias = draw.clone()
    out = eng.overlay(s["dflat"], s["dev"], s["sel"], mode="blend", annotated=alias, table=s["table"], result=dict(buf=alias), **s["kw"])
    assert out["buf"].data_ptr() == alias.data_ptr()
    for k, ((h, w), at) in enumerate(zip(s["shapes"], s["byte_offsets"])):
        assert torch.equal(alias[at:at + 3 * h * w], both[at:at + 3 * h * w]), k


@pytest.mark.parametrize("form", FORMS)
def test_any_selection_and_picture_k_depends_on_its_frame_only(form):
    need_gpu()
    s = _every(form)
    eng, B = s["eng"], s["B"]
    for sel in ([5, 1, 5, 0, 7, 3, 1], list(range(B))[::-1], [6], [4, 2]):
        eng._overlay_ws.fill_(POISON)
        got = eng.overlay(s["dflat"], s["dev"], sel, table=s["table"], **s["kw"])
        assert got["shapes"] == [s["shapes"][b] for b in sel] and got["status"].cpu().tolist() == [0] * len(sel)
        for k, pic in enumerate(_pictures(got["buf"].cpu().numpy(), got["shapes"], got["byte_offsets"])):
            assert np.array_equal(pic, s["pics"][O.BOTH][sel[k]]), (sel, k)
    # the out table of a selection seen before is the packed and uploaded one (the cache Engine.annotate(table=) uses)
    again = eng.overlay(s["dflat"], s["dev"], [6], table=s["table"], **s["kw"])
    assert again["table"] is eng._out_tables[((TINY,), str(s["dflat"].device))] and len(eng._out_tables) <= 16
    with pytest.raises(ValueError):
        eng.overlay(s["dflat"], s["dev"], [B], table=s["table"], **s["kw"])
    with pytest.raises(ValueError):
        eng.overlay(s["dflat"], s["dev"], [0, -1], table=s["table"], **s["kw"])


def test_the_cut_changes_the_cut_frame_only():
    """The same ragged buffer with every byte counted as capacity: the 0xFF tail then IS the masks of the last frame's last instances,
    which shows -- so the equality with the restatement above does mean that the tail was not read."""
    need_gpu()
    s = _every("native")
    eng, B = s["eng"], s["B"]
    got = eng.overlay(s["dflat"], s["dev"], s["sel"], table=s["table"], native=True, capacity_bytes=s["full"].numel())
    pics = _pictures(got["buf"].cpu().numpy(), got["shapes"], got["byte_offsets"])
    for b in range(B - 1):
        assert np.array_equal(pics[b], s["pics"][O.BOTH][b]), b
    assert not np.array_equal(pics[B - 1], s["pics"][O.BOTH][B - 1])


def test_native_slots_at_or_past_the_capacity_are_no_mask_either():
    """The other half of the rule for ragged rows: a slot whose INDEX is at or past `capacity` is not live although its bytes are
    there.  Engine.overlay always passes capacity = B * max_det for the ragged form, so this is a direct call of the C entry point."""
    need_gpu()
    import ctypes as C
    import vti_amd
    s = _every("native")
    eng, B, dev = s["eng"], s["B"], s["dev"]
    capacity = int(s["offsets"][2]) + 1             # frame 2 keeps the first of its two masks; every later frame has none
    assert len(s["ref"][2][0]) == 2
    out_table = eng._out_table(tuple(s["shapes"]), s["dflat"].device)
    buf = torch.full((s["total"] + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    status = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    sel = np.arange(B, dtype=np.int32)
    dsel = torch.from_numpy(sel).cuda()
    pal = np.ascontiguousarray(O.PALETTE, dtype=np.uint8)
    ws = eng._overlay_ws
    ws.fill_(POISON)
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = vti_amd.lib().vti_overlay_frames(
        eng._ctx, p(s["dflat"]), *s["table"]._ptrs(), B, p(s["full"]), 1, p(dev["mask_bases"]), s["kw"]["capacity_bytes"], p(dev["dets"]),
        p(dev["xyxy"]), p(dev["counts"]), p(dev["offsets"]), dev["dets"].shape[1], capacity, None, C.c_void_p(pal.ctypes.data), len(pal),
        0.30, 0.70, C.c_void_p(sel.ctypes.data), p(dsel), B, O.BOTH, None, U.MAX_POINTS, *out_table._ptrs(), p(buf), p(status), p(ws),
        ws.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, vti_amd.lib().vti_last_error(eng._ctx)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[s["total"]:] == POISON).all() and status.cpu().tolist() == [0] * B
    pics = _pictures(host, s["shapes"], s["byte_offsets"])
    live = [max(0, min(s["n_live"][b], capacity - int(s["offsets"][b]))) for b in range(B)]
    assert live[:3] == [s["n_live"][0], s["n_live"][1], 1] and live[3:] == [0] * (B - 3)
    for b in range(B):
        want, word = _uniform(dict(s, n_live=live), b, "both")
        assert word == 0 and np.array_equal(pics[b], want), b
        assert np.array_equal(pics[b], s["pics"][O.BOTH][b]) == (b < 2)                    # the capacity changed frames 2 .. B - 1
    cls, boxes, ms = s["ref"][2]                                                           # ... and the restatement agrees on frame 2
    assert np.array_equal(pics[2], O.render(s["frames"][2], cls, boxes, [ms[0], None], mode=O.BOTH, max_points=U.MAX_POINTS))


def test_contours_beyond_max_points_set_the_status_bit_of_that_frame_only():
    need_gpu()
    import vti_amd
    plain, comb, plain2 = U.jagged_scenes()
    s = _setup("native", [(plain, SMALL), (comb, (240, 1280)), (plain2, ODD)], dead=1, seed=7)
    eng = s["eng"]
    got = eng.overlay(s["dflat"], s["dev"], [0, 1, 2], mode="draw", max_points=U.SMALL_MAX_POINTS, table=s["table"], **s["kw"])
    status = got["status"].cpu().tolist()
    assert status == [0, vti_amd._lib.VTI_OVERLAY_OUTLINE_SKIPPED, 0]
    pics = _pictures(got["buf"].cpu().numpy(), got["shapes"], got["byte_offsets"])
    for b in range(3):
        want, word = _uniform(s, b, "draw", max_points=U.SMALL_MAX_POINTS)
        assert word == status[b] and np.array_equal(pics[b], want), b
    cls, boxes, ms = s["ref"][1]                    # the middle frame equals the restatement drawn without contours: boxes only
    assert np.array_equal(pics[1], O.render(s["frames"][1], cls, boxes, [None] * len(cls), mode=O.DRAW))
    cls, boxes, ms = s["ref"][0]                    # ... and its neighbour has its contours
    assert not np.array_equal(pics[0], O.render(s["frames"][0], cls, boxes, [None] * len(cls), mode=O.DRAW))
    full = eng.overlay(s["dflat"], s["dev"], [1], mode="draw", table=s["table"], **s["kw"])     # with room the frame gets them
    assert full["status"].cpu().tolist() == [0]
    assert not np.array_equal(_pictures(full["buf"].cpu().numpy(), full["shapes"], full["byte_offsets"])[0], pics[1])


def test_the_buffer_and_its_table_feed_encode_jpeg_unchanged():
    need_gpu()
    s = _every("letterbox")
    eng = s["eng"]
    sel = [2, 0, 1]                                 # 481 x 333, 40 x 50, 120 x 203: cheap to encode on the host
    got = eng.overlay(s["dflat"], s["dev"], sel, table=s["table"], **s["kw"])
    data, offs = eng.encode_jpeg(got["buf"], table=got["table"])
    data, offs = data.cpu().numpy(), offs.cpu().tolist()
    for k, b in enumerate(sel):
        assert bytes(data[offs[k]:offs[k + 1]].tobytes()) == jpeg.encode(s["pics"][O.BOTH][b]), (k, b)


# ---- overlay.annotate_results over YOLO.predict of a list of three sizes -----------------------------------------------------------
LIST_SIZES = [(120, 160), (96, 131), (75, 100)]
# on the 128 x 128 canvas of imgsz 128 the first frame has the canvas's own size and a width that is a multiple of 64: its letterbox
# masks [n, 128, 16] have the layout of frame-size rows too
CANVAS_SIZES = [(128, 128), (96, 131), (75, 100)]


@functools.lru_cache(maxsize=None)
def _predicted(retina, sizes=tuple(LIST_SIZES), imgsz=160):
    import vti_amd
    frames = _rand_frames(sizes, 9)
    model = vti_amd.YOLO(None, scale="n", nc=2, seed=3, cls_bias=-1.0, dtype="fp32")
    results = model.predict(frames, conf=0.20, iou=0.25, max_det=50, imgsz=imgsz, retina_masks=retina, mixed=True)
    return model, frames, results


@pytest.mark.parametrize("retina", [False, True])
def test_annotate_results_takes_a_frame_of_the_canvas_size_in_the_list(retina):
    need_gpu()
    model, frames, results = _predicted(retina, tuple(CANVAS_SIZES), 128)
    counts = [len(r) for r in results]
    print(f"canvas-sized first frame, retina={retina}: instances per frame {counts}")
    assert counts[0] >= 1 and sum(counts[1:]) >= 1, "the canvas-sized frame and another one must both have detections"
    bits = results[0].masks.bits
    assert tuple(bits.shape[1:]) == (128, 16) == (128, 8 * -(-128 // 64)) and results[0].masks._W == 128      # one layout, both forms
    other = next(r for r in results[1:] if len(r))
    assert (tuple(other.masks.bits.shape[1:]) == (128, 16)) == (not retina)
    for b, (frame, r, pic) in enumerate(zip(frames, results, O.annotate_results(frames, results, labels=False))):
        assert np.array_equal(pic, O.annotate_result(frame, r, labels=False)), b
    one = O.annotate_results(frames[:1], results[:1], labels=False)                        # alone it votes for neither form
    assert np.array_equal(one[0], O.annotate_result(frames[0], results[0], labels=False))


@pytest.mark.parametrize("retina", [False, True])
def test_the_labelled_path_with_stand_ins_for_the_two_cv2_calls(retina, monkeypatch):
    """DRAW, one copy out, put_labels per picture, one copy back, BLEND -- and the plate rows per slot index -- run here without
    OpenCV: overlay.plates and overlay.put_labels are replaced by deterministic stand-ins (a plate from the label's length, a block of
    pixels at the text's origin), which annotate_result and annotate_results both call."""
    need_gpu()

    def plates(items):
        out = np.zeros((len(items), 4), np.int32)
        for i, (text, org, *_) in enumerate(items):
            out[i] = (org[0] - 4, org[1] - 14, org[0] + 5 * len(text) + 4, org[1] + 6)
        return out

    def put_labels(img, items):
        h, w = img.shape[:2]
        for i, (text, org, *_) in enumerate(items):
            x, y = min(max(org[0], 0), w - 1), min(max(org[1] - 8, 0), h - 1)
            img[y:y + 6, x:x + 3 * len(text)] = (7 * i % 256, len(text), 200)
        return img
    monkeypatch.setattr(O, "plates", plates)
    monkeypatch.setattr(O, "put_labels", put_labels)
    model, frames, results = _predicted(retina)
    pics = O.annotate_results(frames, results, names=model.names, labels=True)
    plain = O.annotate_results(frames, results, labels=False)
    for b, (frame, r, pic) in enumerate(zip(frames, results, pics)):
        assert np.array_equal(pic, O.annotate_result(frame, r, names=model.names, labels=True)), b
        assert np.array_equal(pic, plain[b]) == (len(r) == 0)                              # plates and text do show


@pytest.mark.parametrize("retina", [False, True])
def test_annotate_results_is_annotate_result_frame_by_frame(retina):
    need_gpu()
    model, frames, results = _predicted(retina)
    counts = [len(r) for r in results]
    print(f"retina={retina}: instances per frame {counts}")
    assert sum(counts) >= 1, "the seeded model must detect something, or only bare copies were compared"
    pics = O.annotate_results(frames, results, labels=False)
    assert len(pics) == len(frames)
    for b, (frame, r, pic) in enumerate(zip(frames, results, pics)):
        assert pic.shape == frame.shape and pic.dtype == np.uint8
        want = O.annotate_result(frame, r, labels=False)
        assert np.array_equal(pic, want), b
        assert np.array_equal(pic, frame) == (counts[b] == 0)
        if counts[b]:
            ms = unpack(r.masks.bits.cpu().numpy(), r.masks._W)
            assert ms.shape[1:] == (frame.shape[:2] if retina else (160, 160))
    # the restatement on the first frame with detections (the frames are small)
    b = next(k for k, n in enumerate(counts) if n)
    data = results[b].boxes.data.cpu().numpy()
    want = O.render(frames[b], data[:, 5], data[:, :4], list(unpack(results[b].masks.bits.cpu().numpy(), results[b].masks._W)),
                    mode=O.BOTH, max_points=16384)
    assert np.array_equal(pics[b], want)
    # frames of one size go through the same path; a list without detections is the bare copies
    same = [frames[0], frames[0][::-1].copy()]
    res = model.predict(same, conf=0.20, iou=0.25, max_det=50, imgsz=160, retina_masks=retina)
    for f, r, pic in zip(same, res, O.annotate_results(same, res, labels=False)):
        assert np.array_equal(pic, O.annotate_result(f, r, labels=False))
    empty = model.predict(frames, conf=0.999999, iou=0.25, max_det=50, imgsz=160, retina_masks=retina, mixed=True)
    bare = O.annotate_results(frames, empty, labels=False)
    assert all(np.array_equal(p, f) and p is not f for p, f in zip(bare, frames))
    with pytest.raises(ValueError):
        O.annotate_results(frames[:2], results, labels=False)


@pytest.mark.parametrize("retina", [False, True])
def test_annotate_results_with_labels_is_annotate_result_with_labels(retina):
    pytest.importorskip("cv2")
    need_gpu()
    model, frames, results = _predicted(retina)
    pics = O.annotate_results(frames, results, names=model.names, labels=True)
    for b, (frame, r, pic) in enumerate(zip(frames, results, pics)):
        assert np.array_equal(pic, O.annotate_result(frame, r, names=model.names, labels=True)), b
