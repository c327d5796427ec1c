"""-m gpu: vti_annotate_checker (the stitch-distance checker's picture on the device) against the restatement
annotate.rasterise(frame, annotate.checker_display_list(...)), byte for byte.  The restatement is fed what the device produced
(vti_measure_checker's frame_i32 / stitch_f64 / stitch_i32 and the masks it read): the measurement itself is test_gpu_checker.py's
subject.  The scenes, batches and modes are test_gpu_checker's sixteen, with three slots past the capacity (dead = 3) so that a dead
fabric slot contributes its filled box.  tests/test_annotate_checker.py pins the restatement by hand-written lists on the CPU."""
import functools

import numpy as np
import pytest
import torch

import annotate_util as U
import test_gpu_checker as tc
import test_gpu_measure as tg
from gpu_util import frames_u8, need_gpu
from test_gpu_annotate import POISON, _host, _poison_scratch, _poisoned_result
from vti_amd import annotate as A

pytestmark = pytest.mark.gpu
MODE_IDS = ["letterbox", "native", "native_odd"]
DEAD = 3
NAMES = ("defaults", "drop_empty", "nb0_iters1")


def _engine():
    return tg._engine(736, 960, 16)


@functools.lru_cache(maxsize=None)
def _frames(h, w):
    frames = frames_u8(len(tc.scenes()), h, w, 5)
    return frames, torch.from_numpy(frames).cuda()


def _calib(h, w, mh, mw, native, calib_id):
    return tc.CALIB if calib_id == "real" else tc.degenerate_calib(h, w, mh, mw, native, DEAD)


@functools.lru_cache(maxsize=None)
def _measured(h, w, mh, mw, native, name, calib_id="real"):
    """One vti_measure_checker call on the sixteen scenes -> (params, the device dict, its host copy)."""
    params = tc._params(_calib(h, w, mh, mw, native, calib_id), **tc.SETTINGS[name])
    meas = _engine().measure_checker(tc.device_batch(h, w, mh, mw, native, DEAD), params, h, w, native=native)
    return params, meas, _host(meas)


@functools.lru_cache(maxsize=None)
def _expected(h, w, mh, mw, native, name, calib_id="real", max_points=U.MAX_POINTS):
    """The restatement of every frame, once per (shape, settings): [(picture, status word, primitives)]."""
    params, _, host = _measured(h, w, mh, mw, native, name, calib_id)
    _, ref, offsets, cap = tc.host_batch(h, w, mh, mw, native, DEAD)
    frames, _ = _frames(h, w)
    out = []
    for b, (cls, boxes, ms) in enumerate(ref):
        rows = U.device_rows(host, b, offsets, cap, len(cls))
        prims, word = A.checker_display_list(h, w, cls, boxes, ms, rows, params, max_points=max_points, with_status=True)
        out.append((A.rasterise(frames[b], prims), word, prims))
    return out


def _draw(h, w, mh, mw, native, name, sel, calib_id="real", **kw):
    params, meas, _ = _measured(h, w, mh, mw, native, name, calib_id)
    return _engine().annotate_checker(_frames(h, w)[1], tc.device_batch(h, w, mh, mw, native, DEAD), meas, params, sel, native=native, **kw)


def _kinds(prims):
    return {(q[0], tuple(q[3]) if q[0] != "polyline" else (bool(q[2]), tuple(q[3]))) for q in prims}


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("mode,h,w,mh,mw", tc.MODES, ids=MODE_IDS)
def test_every_frame_equals_the_restatement(mode, h, w, mh, mw, name):
    need_gpu()
    native = mode == "native"
    frames, _ = _frames(h, w)
    B = len(frames)
    out = _draw(h, w, mh, mw, native, name, list(range(B)))
    got, status = out["frames"].cpu().numpy(), out["status"].cpu().tolist()
    exp = _expected(h, w, mh, mw, native, name)
    seen = set()
    for b, (want, word, prims) in enumerate(exp):
        diff = np.argwhere((got[b] != want).any(axis=-1))
        print(f"{mode} {h}x{w} {name} frame {b}: primitives {len(prims)} status {status[b]} differing pixels {len(diff)}"
              + (f" first at (y, x) {diff[0].tolist()}" if len(diff) else ""))
        assert status[b] == word == 0 and len(diff) == 0, (b, status[b], word, len(diff), diff[:5].tolist())
        seen |= _kinds(prims)
    # the scenes draw every kind of primitive the checker has
    for kind in (("rect", A.STITCH_BOX_COLOUR), ("rect", A.FABRIC_BOX_COLOUR), ("polyline", (False, A.ENVELOPE_COLOUR)),
                 ("polyline", (True, A.ENVELOPE_COLOUR)), ("line", A.DIST_COLOUR), ("circle", A.EDGE_POINT_COLOUR),
                 ("circle", A.WIDTH_COLOUR), ("line", A.WIDTH_COLOUR), ("circle", A.CHECKER_CENTRE_COLOUR)):
        assert kind in seen, kind
    _, ref, offsets, cap = tc.host_batch(h, w, mh, mw, native, DEAD)
    # the dead fabric slot of I_DEAD (past the capacity): without drop_empty its filled box is all the fabric there is next to the
    # empty-mask instance's, and both are in the picture's envelope and outline; with drop_empty the frame stops after its boxes
    cls, boxes, ms = ref[tc.I_DEAD]
    assert ms[-1] is None and cls[-1] == 1
    dead_prims = exp[tc.I_DEAD][2]
    if name == "drop_empty":
        assert all(q[0] == "rect" for q in dead_prims) and len(dead_prims) == sum(m is not None and m.any() for m in ms)
    else:
        assert sum(q[0] == "rect" for q in dead_prims) == len(cls) and any(q[0] == "polyline" and q[2] for q in dead_prims)


@pytest.mark.parametrize("mode,h,w,mh,mw", tc.MODES, ids=MODE_IDS)
def test_every_output_byte_is_written_and_nothing_else(mode, h, w, mh, mw):
    need_gpu()
    native = mode == "native"
    eng = _engine()
    _, dframes = _frames(h, w)
    B = dframes.shape[0]
    sel = list(range(B))
    _draw(h, w, mh, mw, native, "defaults", sel)                # allocates the scratch ...
    _poison_scratch(eng)                                        # ... which is then poisoned, as the output is
    flat, res = _poisoned_result(B, h, w)
    before = dframes.clone()
    out = _draw(h, w, mh, mw, native, "defaults", sel, result=res)
    torch.cuda.synchronize()
    assert torch.equal(dframes, before)                         # dev_frames is read only
    assert (flat[B * h * w * 3:] == POISON).all()               # nothing past dev_out
    assert out["status"].cpu().tolist() == [0] * B
    got = out["frames"].cpu().numpy()
    for b, (want, _, _) in enumerate(_expected(h, w, mh, mw, native, "defaults")):
        assert np.array_equal(got[b], want), (b, int((got[b] != want).any(axis=-1).sum()))      # no poisoned byte is left either


def test_any_selection_and_output_k_depends_only_on_its_frame():
    need_gpu()
    mode, h, w, mh, mw = tc.MODES[0]
    eng = _engine()
    _, dframes = _frames(h, w)
    B = dframes.shape[0]
    every = _draw(h, w, mh, mw, False, "defaults", list(range(B)))["frames"].clone()
    assert not torch.equal(every, dframes)
    for sel in (list(range(B))[::-1], [11, 0, 5, 5, 2, 14, 14], [tc.I_BOXES]):
        _poison_scratch(eng)
        flat, res = _poisoned_result(len(sel), h, w)
        out = _draw(h, w, mh, mw, False, "defaults", sel, result=res)
        torch.cuda.synchronize()
        assert (flat[len(sel) * h * w * 3:] == POISON).all()
        assert out["status"].cpu().tolist() == [0] * len(sel)
        for k, b in enumerate(sel):
            assert torch.equal(out["frames"][k], every[b]), (sel, k, b)
    with pytest.raises(ValueError):
        _draw(h, w, mh, mw, False, "defaults", [B])
    with pytest.raises(ValueError):
        _draw(h, w, mh, mw, False, "defaults", [])


@pytest.mark.parametrize("mode,h,w,mh,mw", tc.MODES[:2], ids=MODE_IDS[:2])
def test_an_outline_beyond_max_points_sets_the_status_bit_and_is_left_out(mode, h, w, mh, mw):
    """Scene 8's fabric has a wavy edge: its outline needs hundreds of vertices, the plain scenes' a handful."""
    need_gpu()
    import vti_amd
    native = mode == "native"
    full = _expected(h, w, mh, mw, native, "defaults")
    need = [sum(len(q[1]) for q in prims if q[0] == "polyline" and q[2]) for _, _, prims in full]
    small = 40
    assert max(need) > small and 0 < min(n for n in need if n) <= small, need
    sel = [b for b in range(len(full)) if need[b]]
    out = _draw(h, w, mh, mw, native, "defaults", sel, max_points=small)
    got, status = out["frames"].cpu().numpy(), out["status"].cpu().tolist()
    exp = _expected(h, w, mh, mw, native, "defaults", "real", small)
    assert status == [vti_amd._lib.VTI_ANNOTATE_OUTLINE_SKIPPED if need[b] > small else 0 for b in sel]
    assert len(set(status)) == 2
    for k, b in enumerate(sel):
        want, word, prims = exp[b]
        assert word == status[k]
        assert any(q[0] == "polyline" and q[2] for q in prims) == (need[b] <= small)       # drawn without step f, everything else stands
        assert any(q[0] == "polyline" and not q[2] for q in prims)
        assert np.array_equal(got[k], want), (b, int((got[k] != want).any(axis=-1).sum()))


def test_the_width_estimate_on_the_degenerate_plane_draws_no_width_markers():
    """test_gpu_checker.degenerate_calib: denom is exactly 0 on the left column of the first final stitch of I_BELOW, so its width is
    the local-scale estimate: VTI_STITCH_WIDTH is set, the centroid is drawn, the width markers are not -- host and device agree on
    the 1e-9 test."""
    need_gpu()
    mode, h, w, mh, mw = tc.MODES[1]
    b = tc.I_BELOW
    _, _, host = _measured(h, w, mh, mw, True, "defaults", "degenerate")
    _, ref, offsets, cap = tc.host_batch(h, w, mh, mw, True, DEAD)
    rows = U.device_rows(host, b, offsets, cap, len(ref[b][0]))
    calib = tc.degenerate_calib(h, w, mh, mw, True, DEAD)
    final = [i for i in range(len(rows["flags"])) if rows["flags"][i] & A.WIDTH]
    est = [i for i in final if not (A.world_point_exists(rows["f64"][i, 2], rows["f64"][i, 1], *calib) and
                                    A.world_point_exists(rows["f64"][i, 3], rows["f64"][i, 1], *calib))]
    assert len(est) >= 1 and len(final) > len(est)
    want, word, prims = _expected(h, w, mh, mw, True, "defaults", "degenerate")[b]
    assert sum(q[0] == "circle" and q[3] == A.CHECKER_CENTRE_COLOUR for q in prims) == len(final)
    assert sum(q[0] == "line" and q[3] == A.WIDTH_COLOUR for q in prims) == len(final) - len(est)
    out = _draw(h, w, mh, mw, True, "defaults", [b, 0, tc.I_STRADDLE], "degenerate")
    got = out["frames"].cpu().numpy()
    exp = _expected(h, w, mh, mw, True, "defaults", "degenerate")
    for k, f in enumerate([b, 0, tc.I_STRADDLE]):
        assert np.array_equal(got[k], exp[f][0]), (f, int((got[k] != exp[f][0]).any(axis=-1).sum()))
    # the same frame with the real calibration has the markers the estimate leaves out
    real = _expected(h, w, mh, mw, True, "defaults")[b]
    assert sum(q[0] == "line" and q[3] == A.WIDTH_COLOUR for q in real[2]) > len(final) - len(est)
    assert not np.array_equal(real[0], want)


def test_the_picture_differs_from_vti_annotates_on_the_same_inputs():
    need_gpu()
    import vti_amd
    mode, h, w, mh, mw = tc.MODES[0]
    eng = _engine()
    _, dframes = _frames(h, w)
    dev = tc.device_batch(h, w, mh, mw, False, DEAD)
    sel = [tc.I_STRADDLE, tc.I_BOXES]
    ours = _draw(h, w, mh, mw, False, "defaults", sel)["frames"]
    p = vti_amd.MeasureParams(*tc.CALIB, roi_enabled=False, max_px_distance=150)
    theirs = eng.annotate(dframes, dev, eng.measure(dev, p, h, w), p, sel)["frames"]
    for k in range(len(sel)):
        differing = int((ours[k] != theirs[k]).any(dim=-1).sum())
        assert differing > 1000, (sel[k], differing)               # another edge, other markers, another outline colour
    # vti_annotate's own picture is what it was: its outline is still drawn in its own colour
    want = A.rasterise(_frames(h, w)[0][tc.I_BOXES], A.display_list(
        h, w, *tc.host_batch(h, w, mh, mw, False, DEAD)[1][tc.I_BOXES],
        U.device_rows(_host(eng.measure(dev, p, h, w)), tc.I_BOXES, *tc.host_batch(h, w, mh, mw, False, DEAD)[2:], len(tc.scenes()[tc.I_BOXES])),
        p, max_points=U.MAX_POINTS))
    assert np.array_equal(theirs[1].cpu().numpy(), want)
    assert (want == A.OUTLINE_COLOUR).all(axis=-1).any()


def _strip(rec):
    return {k: v for k, v in rec.items() if k != "timestamp"}


@pytest.mark.parametrize("retina", [False, True])
def test_stitch_distance_checker_returns_the_pictures_over_predict(retina):
    """process_frames(annotate="all"): the pictures equal the restatement fed with the same call's rows and the masks of the output
    set the call left behind; with encode="jpeg" the bytes are jpeg.encode(picture, 95); the records are those of a call without
    annotate."""
    need_gpu()
    import vti_amd
    from vti_amd import jpeg
    h, w = 960, 1280
    kw = dict(conf=0.20, iou=0.45, max_det=200, imgsz=640, retina_masks=retina)
    frames = frames_u8(2, h, w, 0)
    model = vti_amd.YOLO(None, scale="n", nc=2, seed=3, cls_bias=-1.0, dtype="h2")
    params = tc._params()
    plain = vti_amd.StitchDistanceChecker(model, params).process_frames(frames, **kw)
    ck = vti_amd.StitchDistanceChecker(model, params)
    annotated, records, rows = ck.process_frames(frames, annotate="all", rows=True, **kw)
    assert [_strip(r) for r in records] == [_strip(r) for r in plain]
    assert [a[0] for a in annotated] == [0, 1] and all(a[1].shape == (h, w, 3) and a[1].dtype == np.uint8 for a in annotated)
    assert model._last_frames is None                           # the model does not hold on to the device batch
    eng = next(iter(model._engines.values()))
    o = next(iter(model._outs.values()))
    cnt, off = o["counts"].cpu().numpy(), o["offsets"].cpu().numpy()
    dets, xyxy = o["dets"].cpu().numpy(), o["xyxy"].cpu().numpy()
    mw = w if retina else eng.W
    drawn = 0
    for b, pic, items in annotated:
        n = int(cnt[b])
        ms = [tg.unpack(s, mw) for s in o["masks"][off[b]:off[b] + n].cpu().numpy()]
        prims = A.checker_display_list(h, w, dets[b, :n, 5], xyxy[b, :n], ms, rows[b], ck.params, max_points=U.MAX_POINTS)
        want = A.rasterise(frames[b], prims)
        print(f"pipeline retina={retina} frame {b}: {n} instances, status {rows[b]['status']}, {len(prims)} primitives")
        assert np.array_equal(pic, want), (b, int((pic != want).any(axis=-1).sum()))
        assert items == vti_amd.checker_text_items(records[b], rows[b], h), b
        drawn += int(len(prims) > 0)
    assert drawn >= 1
    # the JPEG files of the same pictures, and a selection out of order
    enc, rec2 = vti_amd.StitchDistanceChecker(model, params).process_frames(frames, annotate=[1, 0], encode="jpeg", **kw)
    assert [_strip(r) for r in rec2] == [_strip(r) for r in plain] and [e[0] for e in enc] == [1, 0]
    by = {b: pic for b, pic, _ in annotated}
    for b, data, items in enc:
        assert isinstance(data, bytes) and data == jpeg.encode(by[b], 95), b
    # one frame, the checker's tuple
    alone = vti_amd.StitchDistanceChecker(model, params).process_frame(frames[1], **kw)
    pic, rec = vti_amd.StitchDistanceChecker(model, params).process_frame(frames[1], annotate=True, **kw)
    assert pic.shape == (h, w, 3) and _strip(rec) == _strip(alone)
    with pytest.raises(ValueError):
        ck.process_frames(frames, encode="jpeg", **kw)
    with pytest.raises(ValueError):
        ck.process_frames(frames, annotate="all", encode="png", **kw)
