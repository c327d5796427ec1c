"""-m gpu: vti_overlay (the model-check viewer's picture on the device, Utils/check_model.py:155-256) against the restatement in
overlay.py, byte for byte.  tests/test_overlay.py pins the restatement itself on the CPU (the blend against exact arithmetic, the
tint's order, the filled rectangle, BOTH = BLEND of DRAW).

Shapes: letterbox 120 x 203 with 96 x 160 masks (a non-integer stretch on both axes, a width that is no multiple of 16 or 64, three
raster tiles split mid-row); native 481 x 333 (row_bytes 48); native 960 x 1280 (the tracer's LDS form: 153 600 bytes fit) and
native 1040 x 1280 (its global form: 166 400 bytes do not), one frame each because the Python rasteriser costs about a second per
full-size frame."""
import numpy as np
import pytest
import torch

import annotate_util as U
from gpu_util import frames_u8, need_gpu
from test_gpu_measure import _engine, _fabric, _stitch, scenes, unpack
from vti_amd import jpeg
from vti_amd import overlay as O

pytestmark = pytest.mark.gpu
POISON = 0xA5
MH, MW = 96, 160                                    # the letterbox canvas of the small engine
SMALL = ("letterbox", 120, 203, MH, MW)
ODD = ("native", 481, 333, 481, 333)
SHAPES = [SMALL + ("some",), ODD + ("some",), ("native", 960, 1280, 960, 1280, "one"), ("native", 1040, 1280, 1040, 1280, "one")]
SHAPE_IDS = ["letterbox_120x203", "native_481x333", "native_960x1280_lds", "native_1040x1280_global"]
PALETTE16 = tuple((17 * k % 256, 255 - 13 * k, (40 + 29 * k) % 256) for k in range(16))


def overlap_scene():
    """Two fabric masks that overlap, stitches listed before, between and after them (some of them inside the overlap)."""
    return ([_stitch(200 + 90 * k, 560) for k in range(4)] + [_fabric(60, 300, 900, 700, bottom=680)] + [_stitch(700, 500, w=60, h=40)] +
            [_fabric(500, 350, 1220, 720, bottom=700, amp=10.0)] + [_stitch(300 + 120 * k, 640) for k in range(5)] + [_stitch(760, 420, w=50, h=30)])


def _scene_list(which):
    s = scenes()
    if which == "one":
        return [overlap_scene()]
    return [s[0], overlap_scene(), s[4], s[5], s[9], s[11], s[8], s[3]]       # the last frame's last 3 slots are past the capacity


def _eng():
    return _engine(MH, MW, 16)


def _batch(scene_list, mode, h, w, mh, mw, seed=0, dead=3, recolour=False):
    native = mode == "native"
    arr, ref, offsets, cap = U.host_batch(scene_list, h, w, mh, mw, native, dead=dead)
    if recolour:                                    # classes 0 .. 22, so that a 16-colour palette is used all over
        for b, (cls, _, _) in enumerate(ref):
            cls[:] = (5 * np.arange(len(cls)) + b) % 23
            arr["dets"][b, :len(cls), 5] = cls
    dev = {k: torch.from_numpy(v).cuda() for k, v in arr.items()}
    frames = frames_u8(len(ref), h, w, seed)
    return native, dev, ref, offsets, cap, frames, torch.from_numpy(frames).cuda()


def _poisoned_result(n_sel, h, w, guard=4096):
    flat = torch.full((n_sel * h * w * 3 + guard,), POISON, dtype=torch.uint8, device="cuda")
    return flat, dict(frames=flat[:n_sel * h * w * 3].view(n_sel, h, w, 3), status=torch.full((n_sel,), -7, dtype=torch.int32, device="cuda"))


def _poison_scratch(eng):
    if getattr(eng, "_overlay_ws", None) is not None:
        eng._overlay_ws.fill_(POISON)


def _report(tag, got, want):
    diff = np.argwhere((got != want).any(axis=-1))
    print(f"{tag}: differing pixels {len(diff)}" + (f" first at (y, x) {diff[0].tolist()}" if len(diff) else ""))
    return len(diff)


def _render(frame, ref_b, mode, plates=None, annotated=None, max_points=U.MAX_POINTS, palette=O.PALETTE):
    cls, boxes, ms = ref_b
    return O.render(frame, cls, boxes, ms, plates, mode=mode, annotated=annotated, palette=palette, max_points=max_points,
                    with_status=True)


@pytest.mark.parametrize("mode,h,w,mh,mw,which", SHAPES, ids=SHAPE_IDS)
def test_every_selected_frame_equals_the_restatement_in_each_mode(mode, h, w, mh, mw, which):
    need_gpu()
    eng = _eng()
    native, dev, ref, offsets, cap, frames, dframes = _batch(_scene_list(which), mode, h, w, mh, mw)
    B = len(ref)
    sel = list(range(B))
    pictures = frames_u8(B, h, w, 77)                                           # BLEND's dev_annotated: any picture
    dpictures = torch.from_numpy(pictures).cuda()
    before, pic_before = dframes.clone(), dpictures.clone()
    got = {}
    for m, name in ((O.DRAW, "draw"), (O.BLEND, "blend"), (O.BOTH, "both")):
        ann = dpictures if m == O.BLEND else None
        eng.overlay(dframes, dev, sel, native=native, mode=name, annotated=ann)           # allocates the scratch ...
        _poison_scratch(eng)                                                               # ... which is then poisoned, as the output is
        flat, res = _poisoned_result(B, h, w)
        out = eng.overlay(dframes, dev, sel, native=native, mode=name, annotated=ann, max_points=U.MAX_POINTS, result=res)
        torch.cuda.synchronize()
        assert (flat[B * h * w * 3:] == POISON).all(), name                                # nothing past dev_out
        assert out["status"].cpu().tolist() == [0] * B, name
        got[m] = out["frames"].cpu().numpy()
    assert torch.equal(dframes, before) and torch.equal(dpictures, pic_before)             # dev_frames, dev_annotated are read only
    bad = tinted = drawn = 0
    for b in range(B):
        draw, word = _render(frames[b], ref[b], O.DRAW)
        assert word == 0
        blend, _ = _render(frames[b], ref[b], O.BLEND, annotated=pictures[b])
        # full size: BOTH as BLEND of DRAW's picture (the identity test_overlay.py pins), which saves a second rasterisation
        both = _render(frames[b], ref[b], O.BLEND, annotated=draw)[0] if which == "one" else _render(frames[b], ref[b], O.BOTH)[0]
        for m, want in ((O.DRAW, draw), (O.BLEND, blend), (O.BOTH, both)):
            bad += _report(f"{mode} {h}x{w} frame {b} mode {m} ({len(ref[b][0])} instances)", got[m][b], want)
        drawn += int((draw != frames[b]).any())
        tinted += int((O.tint(frames[b], ref[b][0], [O.instance_bitmap(x, h, w) for x in ref[b][2]]) != frames[b]).any())
    assert bad == 0
    assert drawn == B and tinted >= B - 1                                                  # the scenes do exercise both halves


def test_both_is_blend_of_draw_and_blend_may_write_over_its_picture():
    need_gpu()
    eng = _eng()
    mode, h, w, mh, mw = SMALL
    native, dev, ref, offsets, cap, frames, dframes = _batch(_scene_list("some"), mode, h, w, mh, mw, seed=1)
    sel = [1, 0, 5, 1]
    draw = eng.overlay(dframes, dev, sel, native=native, mode="draw")["frames"].clone()
    both = eng.overlay(dframes, dev, sel, native=native, mode="both")["frames"].clone()
    blend = eng.overlay(dframes, dev, sel, native=native, mode="blend", annotated=draw)["frames"].clone()
    assert torch.equal(both, blend) and not torch.equal(both, draw)
    # dev_out is the very buffer dev_annotated points to
    alias = draw.clone()
    out = eng.overlay(dframes, dev, sel, native=native, mode="blend", annotated=alias, result=dict(frames=alias))
    assert out["frames"].data_ptr() == alias.data_ptr() and torch.equal(alias, both)


def test_plates_inside_across_every_edge_outside_degenerate_and_for_a_dead_slot():
    need_gpu()
    eng = _eng()
    mode, h, w, mh, mw = SMALL
    native, dev, ref, offsets, cap, frames, dframes = _batch(_scene_list("some"), mode, h, w, mh, mw, seed=2, recolour=True)
    B = len(ref)
    kinds = [(20, 10, 60, 22), (-15, 30, 12, 41), (190, 50, 230, 60), (40, -9, 90, 6), (100, 110, 150, 140), (-5, -5, w + 5, 3),
             (-40, 10, -3, 20), (w + 1, 10, w + 30, 20), (10, -30, 40, -1), (10, h, 40, h + 9), (33, 44, 33, 44),
             (50, 30, 49, 40), (50, 40, 60, 39), (7, 70, 7, 90), (70000, -70000, 70010, 5)]
    total = int(offsets[-1])
    table = np.array([kinds[s % len(kinds)] for s in range(total)], np.int32)
    table[:, [0, 2]] += (np.arange(total) % 11)[:, None]                                   # not all alike
    assert total - cap == 3
    table[cap:] = (30, 60, 90, 80)                                                         # the dead slots' rows: visible if they were drawn
    dplates = torch.from_numpy(table).cuda()                                               # they follow the live ones in memory
    sel = list(range(B))
    out = eng.overlay(dframes, dev, sel, native=native, plates=dplates[:cap], mode="both", palette=PALETTE16)
    none = eng.overlay(dframes, dev, sel, native=native, plates=None, mode="both", palette=PALETTE16)["frames"].cpu().numpy()
    got = out["frames"].cpu().numpy()
    bad = 0
    for b in range(B):
        n = len(ref[b][0])
        rows = [tuple(table[offsets[b] + i]) if offsets[b] + i < cap else None for i in range(n)]
        bad += _report(f"plates frame {b}", got[b], _render(frames[b], ref[b], O.BOTH, plates=rows, palette=PALETTE16)[0])
        bad += _report(f"no plates frame {b}", none[b], _render(frames[b], ref[b], O.BOTH, palette=PALETTE16)[0])
    assert bad == 0 and not np.array_equal(got, none)
    assert [r is None for r in rows][-3:] == [True] * 3                                     # the last frame's dead slots


def test_any_selection_and_output_k_depends_only_on_its_frame():
    need_gpu()
    eng = _eng()
    mode, h, w, mh, mw = ODD
    native, dev, ref, offsets, cap, frames, dframes = _batch(_scene_list("some")[:5], mode, h, w, mh, mw, seed=3, dead=0)
    B = len(ref)
    before = dframes.clone()
    every = eng.overlay(dframes, dev, list(range(B)), native=native)["frames"].clone()
    assert not torch.equal(every, dframes)
    for sel in ([3], [4, 0, 3, 3, 2], list(range(B))[::-1], [1] * 4):
        _poison_scratch(eng)
        flat, res = _poisoned_result(len(sel), h, w)
        out = eng.overlay(dframes, dev, sel, native=native, result=res)
        torch.cuda.synchronize()
        assert (flat[len(sel) * h * w * 3:] == POISON).all()
        assert out["status"].cpu().tolist() == [0] * len(sel)
        for k, b in enumerate(sel):
            assert torch.equal(out["frames"][k], every[b]), (sel, k, b)
    assert torch.equal(dframes, before)
    with pytest.raises(ValueError):
        eng.overlay(dframes, dev, [B], native=native)
    with pytest.raises(ValueError):
        eng.overlay(dframes, dev, [0, -1], native=native)


def test_contours_beyond_max_points_set_the_status_bit_and_are_left_out():
    """The comb scene: 191 fabric instances, four vertices per tooth.  240 x 1280 keeps the teeth (two columns each) and makes the
    frames cheap to rasterise."""
    need_gpu()
    import vti_amd
    eng = _eng()
    h, w = 240, 1280
    native, dev, ref, offsets, cap, frames, dframes = _batch(U.jagged_scenes(), "native", h, w, h, w, seed=4, dead=0)
    out = eng.overlay(dframes, dev, [0, 1, 2], native=True, mode="draw", max_points=U.SMALL_MAX_POINTS)
    got, status = out["frames"].cpu().numpy(), out["status"].cpu().tolist()
    assert status == [0, vti_amd._lib.VTI_OVERLAY_OUTLINE_SKIPPED, 0]
    for b in range(3):
        want, word = _render(frames[b], ref[b], O.DRAW, max_points=U.SMALL_MAX_POINTS)
        assert word == status[b]
        assert _report(f"comb frame {b}", got[b], want) == 0
    # the middle frame equals the restatement drawn without contours: boxes only
    cls, boxes, ms = ref[1]
    assert np.array_equal(got[1], O.render(frames[1], cls, boxes, [None] * len(cls), mode=O.DRAW))
    # with room for them the same frame gets its contours
    full = eng.overlay(dframes, dev, [1], native=True, mode="draw")
    assert full["status"].cpu().tolist() == [0]
    want, word = _render(frames[1], ref[1], O.DRAW)
    assert word == 0 and not np.array_equal(want, got[1])
    assert _report("comb frame 1 with room", full["frames"][0].cpu().numpy(), want) == 0


def _hand_set(n, h, w, cls=2):
    """An output set of one frame with n instances whose native masks cover the whole frame."""
    rb = 8 * -(-w // 64)
    dets = torch.zeros((1, 4, 38), device="cuda")
    dets[0, :, 5] = cls
    return dict(dets=dets, xyxy=torch.zeros((1, 4, 4), device="cuda") - 100.0, counts=torch.tensor([n], dtype=torch.int32, device="cuda"),
                offsets=torch.tensor([0, n], dtype=torch.int32, device="cuda"),
                masks=torch.full((n, h, rb), 0xFF, dtype=torch.uint8, device="cuda"))


@pytest.mark.parametrize("alpha,beta", [(0.30, 0.70), (0.8125, 0.4)])
def test_the_blend_on_the_device_for_every_pair_of_bytes(alpha, beta):
    need_gpu()
    eng = _eng()
    y, x = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    frame, pic = np.repeat(y[:, :, None], 3, axis=2), np.repeat(x[:, :, None], 3, axis=2)
    dframe, dpic = torch.from_numpy(frame[None].copy()).cuda(), torch.from_numpy(pic[None].copy()).cuda()
    # no masks: a = the frame's byte, b = the picture's
    out = eng.overlay(dframe, _hand_set(0, 256, 256), [0], native=True, mode="blend", annotated=dpic, alpha=alpha, beta=beta)
    got = out["frames"][0].cpu().numpy()
    want = O.add_weighted(frame, pic, alpha, beta)
    assert _report(f"blend {alpha} {beta} frame bytes", got, want) == 0 and out["status"].cpu().tolist() == [0]
    # one full-frame mask: a = the palette colour's byte
    out = eng.overlay(dframe, _hand_set(1, 256, 256, cls=2), [0], native=True, mode="blend", annotated=dpic, alpha=alpha, beta=beta)
    got = out["frames"][0].cpu().numpy()
    tinted = np.broadcast_to(np.array(O.PALETTE[2], np.uint8), frame.shape)
    want = O.add_weighted(tinted, pic, alpha, beta)
    assert _report(f"blend {alpha} {beta} palette bytes", got, want) == 0
    assert np.array_equal(want, O.render(frame, [2], np.zeros((1, 4), np.float32) - 100.0, [np.ones((256, 256), np.uint8)],
                                         mode=O.BLEND, annotated=pic, alpha=alpha, beta=beta))


@pytest.mark.parametrize("retina", [False, True])
def test_annotate_result_is_a_drop_in_over_predict(retina):
    need_gpu()
    import vti_amd
    h, w = 120, 160
    frames = frames_u8(2, h, w, 5)
    model = vti_amd.YOLO(None, scale="n", nc=2, seed=3, cls_bias=-1.0, dtype="fp32")
    kw = dict(conf=0.20, iou=0.25, max_det=50, imgsz=160, retina_masks=retina)
    results = model.predict(frames, **kw)
    total = 0
    for frame, r in zip(frames, results):
        n = len(r)
        total += n
        pic = O.annotate_result(frame, r, labels=False)
        assert pic.shape == (h, w, 3) and pic.dtype == np.uint8
        if n == 0:
            assert np.array_equal(pic, frame)
            continue
        data = r.boxes.data.cpu().numpy()
        ms = list(unpack(r.masks.bits.cpu().numpy(), r.masks._W))
        assert ms[0].shape == ((h, w) if retina else tuple(r.masks.data.shape[1:]))
        want = O.render(frame, data[:, 5], data[:, :4], ms, mode=O.BOTH, max_points=16384)
        print(f"drop-in retina={retina}: {n} instances, {int(sum(m.any() for m in ms))} with a mask")
        assert _report(f"drop-in retina={retina}", pic, want) == 0
        assert not np.array_equal(pic, frame)
    assert total >= 1, "the seeded model must detect something, or only the bare copy was compared"
    # a result without detections is the bare copy
    empty = model.predict(frames[:1], conf=0.999999, iou=0.25, max_det=50, imgsz=160, retina_masks=retina)[0]
    assert len(empty) == 0
    pic = O.annotate_result(frames[0], empty, labels=False)
    assert np.array_equal(pic, frames[0]) and pic is not frames[0]
    # without the engine that made it there is no picture
    del results[0]._engine
    with pytest.raises(RuntimeError):
        O.annotate_result(frames[0], results[0], labels=False)


def test_the_picture_feeds_encode_jpeg_unchanged():
    need_gpu()
    eng = _eng()
    mode, h, w, mh, mw = SMALL
    native, dev, ref, offsets, cap, frames, dframes = _batch([overlap_scene()], mode, h, w, mh, mw, seed=6, dead=0)
    out = eng.overlay(dframes, dev, [0], native=native)
    data, offs = eng.encode_jpeg(out["frames"])
    offs = offs.cpu().tolist()
    got = bytes(data[offs[0]:offs[1]].cpu().numpy().tobytes())
    want = jpeg.encode(_render(frames[0], ref[0], O.BOTH)[0])
    assert got == want
