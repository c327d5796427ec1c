"""-m gpu: vti_annotate (process_frame's annotated frame on the device) against the restatement in annotate.py, byte for byte.
The restatement is fed what the device produced (vti_measure's frame_i32 / stitch_f64 / stitch_i32 and the masks it read): the
measurement itself is test_gpu_measure.py's subject, not re-derived here.  tests/test_annotate.py asserts on the CPU that these
scenes exercise every part of the overlay."""
import dataclasses

import numpy as np
import pytest
import torch

import annotate_util as U
from gpu_util import frames_u8, need_gpu
from test_gpu_measure import _engine, unpack
from vti_amd import annotate as A

pytestmark = pytest.mark.gpu
MODE_IDS = ["letterbox", "native", "native_odd"]
POISON = 0xA5


def _params(h, w, name, k=0):
    import vti_amd
    return vti_amd.MeasureParams(*U.CALIB, **U.settings_for(name, h, w, k))


def _batch(scene_list, mode, h, w, mh, mw, seed=0):
    native = mode == "native"
    arr, ref, offsets, cap = U.host_batch(scene_list, h, w, mh, mw, native, dead=3)
    dev = {k: torch.from_numpy(v).cuda() for k, v in arr.items()}
    frames = frames_u8(len(ref), h, w, seed)
    return native, dev, ref, offsets, cap, frames, torch.from_numpy(frames).cuda()


def _host(meas):
    return {k: meas[k].cpu().numpy() for k in ("frame_i32", "stitch_f64", "stitch_i32")}


def _expected(frame, h, w, ref_b, rows, settings, max_points=U.MAX_POINTS):
    cls, boxes, ms = ref_b
    prims, word = A.display_list(h, w, cls, boxes, ms, rows, settings, max_points=max_points, with_status=True)
    return A.rasterise(frame, prims), word, prims


def _poisoned_result(n_sel, h, w, guard=4096):
    flat = torch.full((n_sel * h * w * 3 + guard,), POISON, dtype=torch.uint8, device="cuda")
    return flat, dict(frames=flat[:n_sel * h * w * 3].view(n_sel, h, w, 3), status=torch.full((n_sel,), -7, dtype=torch.int32, device="cuda"))


def _poison_scratch(eng):
    if getattr(eng, "_annotate_ws", None) is not None:
        eng._annotate_ws.fill_(POISON)


@pytest.mark.parametrize("name", U.SETTING_NAMES)
@pytest.mark.parametrize("mode,h,w,mh,mw", U.MODES, ids=MODE_IDS)
def test_every_frame_equals_the_restatement_with_four_cameras(mode, h, w, mh, mw, name):
    need_gpu()
    eng = _engine(736, 960, 16)
    native, dev, ref, offsets, cap, frames, dframes = _batch(U.scenes(), mode, h, w, mh, mw)
    B = len(ref)
    params = [_params(h, w, name, k) for k in range(4)]
    table = eng.pack_cameras(params, "cuda")
    rr = [b % 4 for b in range(B)]
    cams = torch.tensor(rr, dtype=torch.int32, device="cuda")
    meas = eng.measure(dev, table, h, w, native=native, cameras=cams)
    host = _host(meas)
    sel = list(range(B))
    eng.annotate(dframes, dev, meas, table, sel, cameras=cams, native=native)         # allocates the scratch ...
    _poison_scratch(eng)                                                               # ... which is then poisoned, as the output is
    flat, res = _poisoned_result(B, h, w)
    before = dframes.clone()
    out = eng.annotate(dframes, dev, meas, table, sel, cameras=cams, native=native, result=res)
    torch.cuda.synchronize()
    got, status = out["frames"].cpu().numpy(), out["status"].cpu().numpy()
    assert torch.equal(dframes, before)                                                # dev_frames is read only
    assert (flat[B * h * w * 3:] == POISON).all()                                      # nothing past dev_out
    assert status.tolist() == [0] * B
    drawn = 0
    for b in range(B):
        rows = U.device_rows(host, b, offsets, cap, len(ref[b][0]))
        want, word, prims = _expected(frames[b], h, w, ref[b], rows, U.settings_for(name, h, w, rr[b]))
        diff = np.argwhere((got[b] != want).any(axis=-1))
        print(f"{mode} {h}x{w} {name} frame {b}: status {rows['status']} primitives {len(prims)} differing pixels {len(diff)}"
              + (f" first at (y, x) {diff[0].tolist()}" if len(diff) else ""))
        assert word == 0 and len(diff) == 0, (b, len(diff), diff[:5].tolist())
        drawn += int((want != frames[b]).any())
    assert drawn == B                                                                  # every frame has at least its ROI


@pytest.mark.parametrize("mode,h,w,mh,mw", U.MODES, ids=MODE_IDS)
def test_one_camera_is_a_one_row_table_without_an_index(mode, h, w, mh, mw):
    need_gpu()
    eng = _engine(736, 960, 16)
    native, dev, ref, offsets, cap, frames, dframes = _batch(U.scenes(), mode, h, w, mh, mw, seed=1)
    p = _params(h, w, "kmeans")
    meas = eng.measure(dev, p, h, w, native=native)
    host = _host(meas)
    sel = [0, 3, 4, 8, 9, 11]
    out = eng.annotate(dframes, dev, meas, p, sel, native=native)                       # cameras=None: dev_camera_of_frame = NULL
    got = out["frames"].cpu().numpy()
    assert out["status"].cpu().tolist() == [0] * len(sel)
    for k, b in enumerate(sel):
        rows = U.device_rows(host, b, offsets, cap, len(ref[b][0]))
        want, _, _ = _expected(frames[b], h, w, ref[b], rows, U.settings_for("kmeans", h, w))
        assert np.array_equal(got[k], want), (b, int((got[k] != want).any(axis=-1).sum()))
    # the explicit one-row table with an all-zero index is the same call
    table = eng.pack_cameras([p], "cuda")
    again = eng.annotate(dframes, dev, meas, table, sel, cameras=torch.zeros(len(ref), dtype=torch.int32, device="cuda"), native=native)
    assert torch.equal(again["frames"], out["frames"])


def test_any_selection_and_output_k_depends_only_on_its_frame():
    need_gpu()
    mode, h, w, mh, mw = U.MODES[0]
    eng = _engine(736, 960, 16)
    native, dev, ref, offsets, cap, frames, dframes = _batch(U.scenes(), mode, h, w, mh, mw, seed=2)
    B = len(ref)
    p = _params(h, w, "kmeans")
    meas = eng.measure(dev, p, h, w, native=native)
    every = eng.annotate(dframes, dev, meas, p, list(range(B)), native=native)["frames"].clone()      # n_sel = B
    assert not torch.equal(every, dframes)
    for sel in ([5], [11, 0, 5, 5, 2], list(range(B))[::-1], [7] * 4, [8, 3]):
        _poison_scratch(eng)
        flat, res = _poisoned_result(len(sel), h, w)
        out = eng.annotate(dframes, dev, meas, p, sel, native=native, result=res)
        torch.cuda.synchronize()
        assert (flat[len(sel) * h * w * 3:] == POISON).all()
        for k, b in enumerate(sel):
            assert torch.equal(out["frames"][k], every[b]), (sel, k, b)
    with pytest.raises(ValueError):
        eng.annotate(dframes, dev, meas, p, [B], native=native)
    with pytest.raises(ValueError):
        eng.annotate(dframes, dev, meas, p, [0, -1], native=native)


@pytest.mark.parametrize("mode,h,w,mh,mw", U.MODES[:2], ids=MODE_IDS[:2])
def test_an_outline_beyond_max_points_sets_the_status_bit_and_is_left_out(mode, h, w, mh, mw):
    need_gpu()
    import vti_amd
    eng = _engine(736, 960, 16)
    native, dev, ref, offsets, cap, frames, dframes = _batch(U.jagged_scenes(), mode, h, w, mh, mw, seed=3)
    p = _params(h, w, "kmeans")
    meas = eng.measure(dev, p, h, w, native=native)
    host = _host(meas)
    out = eng.annotate(dframes, dev, meas, p, [0, 1, 2], native=native, max_points=U.SMALL_MAX_POINTS)
    got, status = out["frames"].cpu().numpy(), out["status"].cpu().tolist()
    assert status == [0, vti_amd._lib.VTI_ANNOTATE_OUTLINE_SKIPPED, 0]
    for b in range(3):
        rows = U.device_rows(host, b, offsets, cap, len(ref[b][0]))
        want, word, prims = _expected(frames[b], h, w, ref[b], rows, U.settings_for("kmeans", h, w), U.SMALL_MAX_POINTS)
        assert word == status[b]
        assert any(q[0] == "polyline" and q[2] for q in prims) == (b != 1)              # the middle frame is drawn without step 8
        assert np.array_equal(got[b], want), (b, int((got[b] != want).any(axis=-1).sum()))
    # with room for it the same frame gets its outline
    full = eng.annotate(dframes, dev, meas, p, [1], native=native)
    assert full["status"].cpu().tolist() == [0]
    rows = U.device_rows(host, 1, offsets, cap, len(ref[1][0]))
    want, _, _ = _expected(frames[1], h, w, ref[1], rows, U.settings_for("kmeans", h, w))
    assert np.array_equal(full["frames"][0].cpu().numpy(), want)


def test_a_camera_index_outside_the_table_gives_a_plain_copy():
    need_gpu()
    mode, h, w, mh, mw = U.MODES[0]
    eng = _engine(736, 960, 16)
    native, dev, ref, offsets, cap, frames, dframes = _batch(U.scenes(), mode, h, w, mh, mw, seed=4)
    B = len(ref)
    params = [_params(h, w, "kmeans", k) for k in range(4)]
    table = eng.pack_cameras(params, "cuda")
    rr = [b % 4 for b in range(B)]
    good = torch.tensor(rr, dtype=torch.int32, device="cuda")
    bad_idx = list(rr)
    bad_idx[1], bad_idx[6] = -1, 4
    bad = torch.tensor(bad_idx, dtype=torch.int32, device="cuda")
    sel = list(range(B))
    ok = eng.annotate(dframes, dev, eng.measure(dev, table, h, w, native=native, cameras=good), table, sel, cameras=good, native=native)
    ok_frames = ok["frames"].clone()
    meas_bad = eng.measure(dev, table, h, w, native=native, cameras=bad)
    out = eng.annotate(dframes, dev, meas_bad, table, sel, cameras=bad, native=native)
    for b in range(B):
        if b in (1, 6):
            assert torch.equal(out["frames"][b], dframes[b]) and not torch.equal(ok_frames[b], dframes[b])
        else:
            assert torch.equal(out["frames"][b], ok_frames[b]), b
    assert out["status"].cpu().tolist() == [0] * B
    # the index is compared on the device even when the measurement rows say the frame is fine
    mixed = eng.annotate(dframes, dev, eng.measure(dev, table, h, w, native=native, cameras=good), table, sel, cameras=bad, native=native)
    assert torch.equal(mixed["frames"][1], dframes[1]) and torch.equal(mixed["frames"][6], dframes[6])
    with pytest.raises(ValueError):         # the host-sequence form is refused before the call
        eng.annotate(dframes, dev, meas_bad, table, sel, cameras=bad_idx, native=native)


def _strip(rec):
    return {k: v for k, v in rec.items() if k != "timestamp"}


def _check_pipeline(model, frames, annotated, records, params_of, cams, retina, h, w):
    """The pictures equal the restatement fed from Engine.measure's rows on the output set the call left behind; the text equals the
    strings built from the records."""
    eng = next(iter(model._engines.values()))
    o = next(iter(model._outs.values()))
    table = eng.pack_cameras([params_of(c) for c in range(max(cams) + 1)], "cuda")
    cam_t = torch.tensor(cams, dtype=torch.int32, device="cuda")
    meas = _host(eng.measure(o, table, h, w, native=retina, cameras=cam_t))
    cnt, off = o["counts"].cpu().numpy(), o["offsets"].cpu().numpy()
    dets, xyxy = o["dets"].cpu().numpy(), o["xyxy"].cpu().numpy()
    cap = o["masks"].shape[0]
    assert model._last_frames is None            # the model does not hold on to the device batch
    complete = 0
    mw = w if retina else eng.W
    for b, pic, items in annotated:
        n = int(cnt[b])
        ms = [unpack(s, mw) for s in o["masks"][off[b]:off[b] + n].cpu().numpy()]
        rows = U.device_rows(meas, b, off, cap, n)
        p = params_of(cams[b])
        prims = A.display_list(h, w, dets[b, :n, 5], xyxy[b, :n], ms, rows, p, max_points=U.MAX_POINTS)
        want = A.rasterise(frames[b], prims)
        print(f"pipeline retina={retina} frame {b}: {n} instances, status {rows['status']}, {len(prims)} primitives")
        assert np.array_equal(pic, want), (b, int((pic != want).any(axis=-1).sum()))
        assert items == A.text_items(records[b], rows, h, p.min_stitches), b
        kinds = {(q[0], q[3]) for q in prims}
        complete += int(rows["status"] == A.OK and any(q[0] == "polyline" and q[2] for q in prims) and
                        ("circle", A.CENTRE_COLOUR) in kinds and ("line", A.WIDTH_COLOUR) in kinds)
    # the seeded model must give at least one selected frame the whole overlay (markers and a fabric outline), or the comparison
    # above would only have seen the ROI and boxes
    assert complete >= 1, complete


@pytest.mark.parametrize("dtype", ["h2", "fp32"])
@pytest.mark.parametrize("retina", [False, True])
def test_measurers_return_the_annotated_frames_over_predict(retina, dtype):
    need_gpu()
    import vti_amd
    h, w = 960, 1280
    kw = dict(conf=0.20, iou=0.25, max_det=200, imgsz=960, retina_masks=retina)
    frames = frames_u8(3, h, w, 0)
    model = vti_amd.YOLO(None, scale="n", nc=2, seed=3, cls_bias=-1.0, dtype=dtype)
    base = _params(h, w, "kmeans")
    # StitchMeasurer: a selection, out of order; the records are those of a call without annotate on a fresh measurer
    plain = vti_amd.StitchMeasurer(model, base).process_frames(frames, **kw)
    sm = vti_amd.StitchMeasurer(model, base)
    annotated, records = sm.process_frames(frames, annotate=[2, 0], **kw)
    assert [_strip(r) for r in records] == [_strip(r) for r in plain]
    assert [a[0] for a in annotated] == [2, 0] and all(a[1].shape == (h, w, 3) and a[1].dtype == np.uint8 for a in annotated)
    _check_pipeline(model, frames, annotated, records, lambda c: sm.params, [0, 0, 0], retina, h, w)
    # one frame, the reference's tuple; the record is that of the same call without annotate on a fresh measurer
    alone = vti_amd.StitchMeasurer(model, base).process_frame(frames[1], **kw)
    pic, rec = vti_amd.StitchMeasurer(model, base).process_frame(frames[1], annotate=True, **kw)
    assert pic.shape == (h, w, 3) and _strip(rec) == _strip(alone) and not np.array_equal(pic, frames[1])
    # MultiCameraMeasurer: every frame
    cams = [1, 0, 1]
    plist = [_params(h, w, "kmeans", k) for k in range(2)]
    plain = vti_amd.MultiCameraMeasurer(model, plist).process_frames(frames, cams, **kw)
    mc = vti_amd.MultiCameraMeasurer(model, plist)
    annotated, records = mc.process_frames(frames, cams, annotate="all", **kw)
    assert [_strip(r) for r in records] == [_strip(r) for r in plain]
    assert [a[0] for a in annotated] == [0, 1, 2]
    _check_pipeline(model, frames, annotated, records, lambda c: mc.params[c], cams, retina, h, w)
    assert dataclasses.asdict(mc.params[0])["drop_empty"] is False


def test_a_frame_too_large_for_the_tracers_lds_image():
    """1080 x 1920: the union's bit rows (8 * 1080 * 30 bytes) exceed the 156 KiB the outline kernel keeps in LDS, so it labels and
    traces from the scratch instead (annotate_outline_kernel<false>).  Native rows and letterbox bits, three scenes each."""
    need_gpu()
    h, w = 1080, 1920
    assert 8 * h * -(-w // 64) > 156 * 1024
    eng = _engine(736, 960, 16)
    picked = [U.scenes()[k] for k in (0, 10, 11)]
    for mode, mh, mw in (("native", h, w), ("letterbox", 736, 960)):
        native, dev, ref, offsets, cap, frames, dframes = _batch(picked, mode, h, w, mh, mw, seed=6)
        p = _params(h, w, "kmeans")
        meas = eng.measure(dev, p, h, w, native=native)
        host = _host(meas)
        out = eng.annotate(dframes, dev, meas, p, [2, 0, 1], native=native)
        got = out["frames"].cpu().numpy()
        assert out["status"].cpu().tolist() == [0, 0, 0]
        for k, b in enumerate([2, 0, 1]):
            rows = U.device_rows(host, b, offsets, cap, len(ref[b][0]))
            want, word, prims = _expected(frames[b], h, w, ref[b], rows, U.settings_for("kmeans", h, w))
            assert rows["status"] == A.OK and word == 0 and any(q[0] == "polyline" and q[2] for q in prims), b
            diff = int((got[k] != want).any(axis=-1).sum())
            print(f"{mode} {h}x{w} frame {b}: primitives {len(prims)} differing pixels {diff}")
            assert diff == 0, (mode, b, diff)
