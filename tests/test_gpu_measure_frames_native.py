"""-m gpu: vti_measure_frames_native -- the measurement of a batch whose frames differ in size from the ragged frame-size rows of
vti_masks_native_frames.  Frame b's rows are compared byte for byte with vti_measure_cameras(native = 1) called with B = 1 on views
of frame b, and with the per-frame restatement tests/measure_ref.py (counts, flags, ranks exactly; floats 1e-12 relative)."""
import dataclasses

import numpy as np
import pytest
import torch

from gpu_util import need_gpu
from test_gpu_measure import MAX_DET, _engine, pack, render
from test_gpu_measure_cameras import _host
from test_gpu_measure_frames import BAD, MH, MW, NARROW, _params, batch_plan, check_frame, poisoned

pytestmark = pytest.mark.gpu


def build_ragged(eng, plan, cut, seed=1):
    """The output set of a native predict on the mixed batch, hand-made: native rows laid out raggedly in a poisoned buffer.
    cut = (frame, instances of it that fit, extra bytes): capacity_bytes ends inside that frame's run, off a slot boundary."""
    rng = np.random.default_rng(seed)
    B = len(plan)
    shapes = [hw for _, hw, _ in plan]
    counts = np.array([len(s) for s, _, _ in plan], np.int32)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    slot = [eng.mask_native_layout(h, w)["slot_bytes"] for h, w in shapes]
    bases = np.concatenate([[0], np.cumsum([int(n) * s for n, s in zip(counts, slot)])]).astype(np.int64)
    cb, fit, extra = cut
    capacity_bytes = int(bases[cb]) + fit * slot[cb] + extra
    assert fit < counts[cb] and 0 < extra < slot[cb]
    live_slots = int(offsets[cb]) + fit                          # the live slots are a prefix of the slot order
    dets = np.zeros((B, MAX_DET, 38), np.float32)
    xyxy = np.zeros((B, MAX_DET, 4), np.float32)
    masks = np.full(int(bases[-1]), 0xFF, np.uint8)              # whatever lies past the last live slot must not be read
    ref = []
    for b, (insts, (h, w), _) in enumerate(plan):
        cls, boxes, ms = [], [], []
        for i, inst in enumerate(insts):
            m, fbox, _ = render(inst, h, w, h, w, rng)
            dets[b, i, :4] = fbox
            dets[b, i, 4] = 0.9 - 0.001 * i
            dets[b, i, 5] = inst["cls"]
            xyxy[b, i] = fbox
            s = int(offsets[b]) + i
            if s < live_slots:
                at = int(bases[b]) + i * slot[b]
                masks[at:at + slot[b]] = pack(m, True, w).reshape(-1)
            cls.append(inst["cls"])
            boxes.append(fbox)
            ms.append(m if s < live_slots else None)
        ref.append((np.array(cls), np.array(boxes, np.float32).reshape(-1, 4), ms))
    table, _, _ = eng.pack_frames(shapes, "cuda")
    dev = dict(dets=torch.from_numpy(dets).cuda(), xyxy=torch.from_numpy(xyxy).cuda(), counts=torch.from_numpy(counts).cuda(),
               offsets=torch.from_numpy(offsets).cuda(), masks=torch.from_numpy(masks).cuda(),
               mask_bases=torch.from_numpy(bases).cuda(), native_shapes=tuple(table.shapes))
    return dev, table, ref, offsets, bases, slot, capacity_bytes, live_slots


# a dead tail in the last frame | a cut inside a middle frame: every later frame then has empty masks only
@pytest.mark.parametrize("cut", [(10, 50, 1000), (7, 5, 4096)], ids=["dead_tail", "cut_in_the_middle"])
def test_measure_frames_native_is_measure_cameras_per_frame_and_the_restatement(cut):
    need_gpu()
    import measure_ref as mr
    eng = _engine(MH, MW, 16)
    plan = batch_plan()
    B = len(plan)
    shapes = [hw for _, hw, _ in plan]
    assert len(set(shapes)) == 4 and min(w for _, w in shapes) == NARROW[1]
    dev, table, ref, offsets, bases, slot, capacity_bytes, live_slots = build_ragged(eng, plan, cut)
    full = dev["masks"]
    dev = dict(dev, masks=full[:capacity_bytes])                  # the capacity in bytes: the buffer ends inside a slot
    cams = eng.pack_cameras([_params(0), _params(1)], "cuda")
    idx = torch.tensor([c for _, _, c in plan], dtype=torch.int32, device="cuda")
    rows = B * MAX_DET
    eng.measure(dev, cams, cameras=idx, frames=table, native=True, result=poisoned(B, rows))
    eng._measure_ws.fill_(0x55)                                   # whatever the scratch holds beyond a frame's own W0 is not read
    mixed = _host(eng.measure(dev, cams, cameras=idx, frames=table, native=True, result=poisoned(B, rows)))
    total = int(offsets[-1])
    assert (mixed["stitch_i32"][total:] == -7).all() and (mixed["stitch_f64"][total:] == -7.0).all()
    statuses = []
    for b, ((cls, boxes, ms), (h, w), (_, _, cam)) in enumerate(zip(ref, shapes, plan)):
        n = len(cls)
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        # 1. byte for byte vti_measure_cameras(native = 1), B = 1, on views of frame b: its run of slots as a uniform buffer
        n_live = max(0, min(n, live_slots - lo))
        view = dict(dets=dev["dets"][b:b + 1], xyxy=dev["xyxy"][b:b + 1], counts=dev["counts"][b:b + 1],
                    offsets=torch.tensor([0, n], dtype=torch.int32, device="cuda"),
                    masks=eng.frame_masks(full, table, b, int(bases[b]), n_live))
        assert view["masks"].shape[0] == n_live and view["masks"].data_ptr() % 8 == 0
        plain = _host(eng.measure(view, cams, h, w, native=True, cameras=idx[b:b + 1], result=poisoned(1, max(n, 1))))
        assert mixed["frame_f64"][b].tobytes() == plain["frame_f64"][0].tobytes(), (b, mixed["frame_f64"][b], plain["frame_f64"][0])
        assert mixed["frame_i32"][b].tobytes() == plain["frame_i32"][0].tobytes(), (b, mixed["frame_i32"][b], plain["frame_i32"][0])
        # (a slot at or beyond the B = 1 call's capacity gets no row there; the ragged call's rows are per slot INDEX, all written)
        assert mixed["stitch_f64"][lo:lo + n_live].tobytes() == plain["stitch_f64"][:n_live].tobytes(), b
        assert mixed["stitch_i32"][lo:lo + n_live].tobytes() == plain["stitch_i32"][:n_live].tobytes(), b
        # 2. the restatement at the frame's own size under its own camera; a cut instance is an empty mask there
        if cam == BAD:
            assert mixed["frame_i32"][b].tolist() == [3, 0, 0, 0, 0, 0] and np.isnan(mixed["frame_f64"][b]).all()
            statuses.append(3)
            continue
        rec, _ = check_frame(mixed, b, cls, boxes, ms, offsets, total, h, w, cam)
        statuses.append(rec["status"])
    print("statuses", statuses, "live slots", live_slots, "of", total)
    assert {0, 1, 2, 3} <= set(statuses), statuses
    assert statuses[0] == mr.OK and statuses[3] == mr.NO_FABRIC and statuses[4] == mr.NO_STITCHES and statuses[2] == mr.NO_FABRIC
    # the frames in front of the cut are those of an uncut run
    whole = _host(eng.measure(dict(dev, masks=_filled(eng, plan, full, bases, slot, offsets)), cams, cameras=idx, frames=table,
                              native=True, result=poisoned(B, rows)))
    for b in range(cut[0]):
        assert mixed["frame_f64"][b].tobytes() == whole["frame_f64"][b].tobytes() and mixed["frame_i32"][b].tobytes() == whole["frame_i32"][b].tobytes()
    lo = int(offsets[cut[0]])
    assert any(mixed[k][cut[0]:].tobytes() != whole[k][cut[0]:].tobytes() for k in ("frame_f64", "frame_i32")) or \
        mixed["stitch_f64"][lo:total].tobytes() != whole["stitch_f64"][lo:total].tobytes()       # ... and the cut changed something


def _filled(eng, plan, full, bases, slot, offsets, seed=1):
    """The same batch with every slot written (no cut)."""
    rng = np.random.default_rng(seed)
    host = full.cpu().numpy().copy()
    for b, (insts, (h, w), _) in enumerate(plan):
        for i, inst in enumerate(insts):
            m, _, _ = render(inst, h, w, h, w, rng)
            at = int(bases[b]) + i * slot[b]
            host[at:at + slot[b]] = pack(m, True, w).reshape(-1)
    return torch.from_numpy(host).cuda()


def test_multi_camera_measurer_measures_the_mixed_list_at_every_frames_own_size():
    """MultiCameraMeasurer.process_frames(list, cameras, retina_masks=True, mixed=True) == the host smoothing of one stream per camera
    fed vti_measure_cameras(native = 1) on the mixed call's own outputs, frame by frame.  (One StitchMeasurer per camera would predict
    on another canvas, the frame's own rect letterbox, so its detections differ: the comparison is on the same outputs.)"""
    need_gpu()
    import vti_amd
    from vti_amd.measure import CameraStream
    model = vti_amd.YOLO(None, scale="n", nc=2, seed=3, cls_bias=-1.0)
    params = [dataclasses.replace(_params(c), drop_empty=False) for c in range(2)]
    mc = vti_amd.MultiCameraMeasurer(model, params, frame_buffer=8)
    streams = [CameraStream(8) for _ in params]
    # camera 0 has 640 x 640 frames: their own letterbox IS the mixed call's canvas, so their detections agree with a uniform call
    sizes = [(640, 640), (481, 333), (720, 960), (640, 640), (480, 640)]
    cams = [0, 1, 1, 0, 1]
    kw = dict(conf=0.20, iou=0.25, max_det=200, imgsz=640)
    frames = [np.random.Generator(np.random.PCG64(k)).integers(0, 256, (h, w, 3), dtype=np.uint8) for k, (h, w) in enumerate(sizes)]
    with pytest.raises(ValueError, match="retina_masks"):
        mc.process_frames(frames, cams, retina_masks=True, **kw)
    with pytest.raises(ValueError, match="retina_masks=True needs frames of one size"):
        mc.process_frames(frames, cams, retina_masks=True, mixed=True, annotate="all", **kw)
    got = mc.process_frames(frames, cams, retina_masks=True, mixed=True, **kw)
    assert [g["camera"] for g in got] == cams
    (eng, table), = mc._tables.values()
    o, = model._outs.values()                                      # the output set the call measured
    assert "mask_bases" in o and o["masks"].dim() == 1
    ftab = next(iter(model._frame_tables.values()))[0]
    cnt, bases = o["counts"].cpu().tolist(), o["mask_bases"].cpu().tolist()
    assert sum(cnt) >= 4
    idx = torch.tensor(cams, dtype=torch.int32, device="cuda")
    for b, (h, w) in enumerate(sizes):
        view = dict(dets=o["dets"][b:b + 1], xyxy=o["xyxy"][b:b + 1], counts=o["counts"][b:b + 1],
                    offsets=torch.tensor([0, cnt[b]], dtype=torch.int32, device="cuda"),
                    masks=eng.frame_masks(o["masks"], ftab, b, bases[b], cnt[b]))
        r = eng.measure(view, table, h, w, native=True, cameras=idx[b:b + 1], stitch_rows=False)
        e = streams[cams[b]].record(r["frame_f64"][0].cpu().numpy(), r["frame_i32"][0].cpu().numpy())
        g = got[b]
        print("frame", b, sizes[b], "camera", cams[b], {k: v for k, v in g.items() if k != "timestamp"})
        assert {k: v for k, v in g.items() if k not in ("timestamp", "camera")} == {k: v for k, v in e.items() if k != "timestamp"}, b
    # the public comparison where the detections agree: one StitchMeasurer for camera 0, fed that camera's frames at their own size
    mine = [b for b, c in enumerate(cams) if c == 0]
    sm = vti_amd.StitchMeasurer(model, params[0], frame_buffer=8)
    want = sm.process_frames(np.stack([frames[b] for b in mine]), retina_masks=True, **kw)
    strip = lambda rec: {k: v for k, v in rec.items() if k not in ("timestamp", "camera")}
    assert [strip(got[b]) for b in mine] == [strip(w) for w in want]
