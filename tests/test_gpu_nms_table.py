"""-m gpu: the NMS table (vti_set_nms_table) -- conf, iou, max_det, agnostic and a class set per frame.  Everything here is bit for
bit: frame b under row r equals the table-free call on that frame with row r's scalars; a class set equals the table-free call on a
pred whose excluded anchors score nothing (Ultralytics' rule: the filter looks at the class of the first maximal score, after the
confidence test and before the greedy pass and max_det), and the oracle's non_max_suppression on that pred.  Synthetic pred tensors
on an engine at 64 x 64 (84 anchors) with nc = 2 (a lane per anchor in the scan kernel) and nc = 80 (four lanes per anchor)."""
import dataclasses

import numpy as np
import pytest
import torch

from gpu_util import engine_and_oracle, frames_u8, need_gpu, synth_pred
from oracle.postproc import non_max_suppression

pytestmark = pytest.mark.gpu

STRIDE = 40          # the calls' max_det: the row stride of dets and the upper bound of every row's limit


def _engine(nc, H=64, W=64, B=6):
    return engine_and_oracle("n", nc, H, W, B, "fp16")[0]


def planted(nc, B, seed):
    """pred f32 [B, 4+nc+32, 84]: per frame 12 boxes on a 4 x 3 grid of the 64 x 64 canvas, each with 3 jittered duplicates of its own
    class (IoU > 0.7: suppressed at every iou of the tests) and one more box of ANOTHER class on the same place with a lower score
    (kept by class-aware NMS, suppressed by agnostic NMS); scores spread over 0.3 .. 0.95 so that every conf of the tests cuts
    somewhere else; the other 36 anchors are background below every conf.  12 to 24 survivors: more than the smallest max_det."""
    rng = np.random.default_rng(seed)
    A = 84
    pred = np.zeros((B, 4 + nc + 32, A), np.float32)
    pred[:, 4:4 + nc] = rng.uniform(0, 0.04, (B, nc, A)).astype(np.float32)
    pred[:, 0] = rng.uniform(4, 60, (B, A))
    pred[:, 1] = rng.uniform(4, 60, (B, A))
    pred[:, 2:4] = rng.uniform(2, 6, (B, 2, A))
    pred[:, 4 + nc:] = rng.standard_normal((B, 32, A)).astype(np.float32)
    for b in range(B):
        slots = rng.permutation(A)[:48]
        for i in range(12):
            cx, cy = (i % 4 + 0.5) * 16 + rng.uniform(-1, 1), (i // 4 + 0.5) * 21 + rng.uniform(-1, 1)
            w, h = rng.uniform(11, 13), rng.uniform(15, 17)
            c = int(rng.integers(nc))
            top = rng.uniform(0.3, 0.95)
            for d in range(4):
                a = slots[4 * i + d]
                pred[b, :4, a] = [cx + rng.normal(0, 0.1), cy + rng.normal(0, 0.1), w + rng.normal(0, 0.1), h + rng.normal(0, 0.1)]
                pred[b, 4:4 + nc, a] = rng.uniform(0, 0.04, nc)
                if d < 3:
                    pred[b, 4 + c, a] = top - 0.01 * d
                else:                               # the other class on the same place, a lower score
                    pred[b, 4 + (c + 1 + int(rng.integers(nc - 1))) % nc, a] = top * 0.8
    return pred


def pairs(pred, nc):
    """The (best score, its first class) pairs the class towers write beside pred: f32 [B, A, 2]."""
    s = pred[:, 4:4 + nc]
    return np.ascontiguousarray(np.stack((s.max(1), s.argmax(1).astype(np.float32)), -1))


def table_free(eng, pred_d, best_d, b, p, stride=STRIDE):
    """Frame b alone through the table-free call with row p's scalars, padded to the stride -> (dets [stride, 38], count)."""
    dets, counts = eng.nms(pred_d[b:b + 1], p.conf, p.iou, min(p.max_det, stride), p.agnostic,
                           best=None if best_d is None else best_d[b:b + 1])
    out = torch.zeros((stride, dets.shape[2]), dtype=torch.float32, device=dets.device)
    out[:dets.shape[1]] = dets[0]
    return out.cpu().numpy(), int(counts[0])


def excluded_zeroed(pred, nc, classes):
    """pred with the class scores zeroed for every anchor whose first-maximal class is outside `classes`."""
    out = pred.copy()
    drop = ~np.isin(pred[:, 4:4 + nc].argmax(1), np.asarray(classes))          # [B, A]
    out[:, 4:4 + nc] = np.where(drop[:, None, :], 0.0, pred[:, 4:4 + nc])
    return out


@pytest.mark.parametrize("scored", [False, True], ids=["scan", "scored"])
@pytest.mark.parametrize("nc", [2, 80])
def test_every_frame_takes_its_own_row(nc, scored):
    """B = 6, three rows that differ in all four settings, rows = [0, 1, 2, 1, 0, 7]: frames 0 .. 4 bit for bit the table-free call
    on that frame with its row's scalars; frame 5 names a row outside the table: count 0 and zero rows."""
    need_gpu()
    import vti_amd
    eng = _engine(nc)
    pred = planted(nc, 6, 10 + nc)
    pred_d = torch.from_numpy(pred).cuda()
    best_d = torch.from_numpy(pairs(pred, nc)).cuda() if scored else None
    P = vti_amd.NmsParams
    rows = [P(0.25, 0.7, 300, False), P(0.5, 0.45, 5, True), P(0.35, 0.25, 12, False)]
    which = [0, 1, 2, 1, 0, 7]
    table = eng.pack_nms_table(rows)
    idx = torch.tensor(which, dtype=torch.int32, device="cuda")
    dets = torch.full((6, STRIDE, 6 + 32), -7.0, dtype=torch.float32, device="cuda")       # poisoned: the zero fill is the kernel's
    counts = torch.full((6,), -7, dtype=torch.int32, device="cuda")
    with eng.nms_table(table, idx):
        eng.nms(pred_d, 0.99, 0.01, STRIDE, False, dets=dets, counts=counts, best=best_d)      # the call's own settings are ignored
    torch.cuda.synchronize()
    got, n = dets.cpu().numpy(), counts.cpu().numpy()
    seen = []
    for b in range(5):
        ref, nref = table_free(eng, pred_d, best_d, b, rows[which[b]])
        print("frame", b, "row", which[b], "count", n[b], "reference", nref)
        assert n[b] == nref and got[b].tobytes() == ref.tobytes(), b
        assert (got[b, nref:] == 0).all()
        seen.append(nref)
    assert n[5] == 0 and (got[5] == 0).all()
    # the planted batch makes every setting matter: the limits bind, and the strict rows keep fewer than the loose one
    assert seen[1] == 5 and seen[3] == 5 and seen[2] == 12 and seen[0] > 12 and seen[4] > 12
    for b, other in ((0, 2), (2, 0), (1, 0)):                      # ... and a row mix-up does not pass
        ref, _ = table_free(eng, pred_d, best_d, b, rows[other])
        assert got[b].tobytes() != ref.tobytes(), (b, other)
    # rows=None: row 0 for every frame
    with eng.nms_table(table):
        d0, c0 = eng.nms(pred_d, 0.99, 0.01, STRIDE, False, best=best_d)
    for b in range(6):
        ref, nref = table_free(eng, pred_d, best_d, b, rows[0])
        assert int(c0[b]) == nref and d0[b].cpu().numpy().tobytes() == ref.tobytes(), b


@pytest.mark.parametrize("agnostic", [False, True], ids=["class_aware", "agnostic"])
@pytest.mark.parametrize("nc,classes", [(2, (1,)), (80, (3, 17, 64))])
def test_a_class_set_is_the_table_free_call_on_a_pred_without_the_excluded_anchors(nc, classes, agnostic):
    need_gpu()
    import vti_amd
    eng = _engine(nc)
    B = 4
    pred = planted(nc, B, 20 + nc)
    if nc == 80:        # the planted classes are random: move the boxes of every second place into the set, so that it keeps some
        for b in range(B):
            for a in np.flatnonzero(pred[b, 4:4 + nc].max(0) > 0.2)[::2]:
                j = int(pred[b, 4:4 + nc, a].argmax())
                pred[b, 4 + classes[a % 3], a], pred[b, 4 + j, a] = pred[b, 4 + j, a], pred[b, 4 + classes[a % 3], a]
    # an anchor whose best class is excluded (0.9) while an allowed class of it scores above conf (0.6): single-label NMS drops it
    a_x = int(np.flatnonzero(pred[0, 4:4 + nc].max(0) < 0.1)[0])
    out_cls = next(c for c in range(nc) if c not in classes)
    pred[0, :4, a_x] = [32.0, 60.0, 5.0, 4.0]
    pred[0, 4 + out_cls, a_x], pred[0, 4 + classes[0], a_x] = 0.9, 0.6
    conf, iou = 0.25, 0.45
    pred_z = excluded_zeroed(pred, nc, classes)
    assert pred_z[0, 4:4 + nc, a_x].max() == 0
    pred_d, pred_zd = torch.from_numpy(pred).cuda(), torch.from_numpy(pred_z).cuda()
    table = eng.pack_nms_table([vti_amd.NmsParams(conf, iou, STRIDE, agnostic, classes)])
    for scored in (False, True):
        best_d = torch.from_numpy(pairs(pred, nc)).cuda() if scored else None
        best_zd = torch.from_numpy(pairs(pred_z, nc)).cuda() if scored else None
        with eng.nms_table(table):
            dets, counts = eng.nms(pred_d, 0.0, 1.0, STRIDE, not agnostic, best=best_d)
        want, wcounts = eng.nms(pred_zd, conf, iou, STRIDE, agnostic, best=best_zd)
        torch.cuda.synchronize()
        assert torch.equal(counts, wcounts) and dets.cpu().numpy().tobytes() == want.cpu().numpy().tobytes(), scored
    dets, counts = dets.cpu().numpy(), counts.cpu().numpy()
    ref = non_max_suppression(pred_z, conf, iou, STRIDE, nc=nc, agnostic=agnostic)       # test_gpu_postproc.py's comparison
    kept = 0
    for b, r in enumerate(ref):
        assert counts[b] == len(r), (b, counts[b], len(r))
        assert np.array_equal(dets[b, :len(r)], r), f"frame {b}: rows differ"
        assert (dets[b, len(r):] == 0).all()
        assert np.isin(dets[b, :len(r), 5], classes).all()
        kept += len(r)
    print("kept", counts.tolist())
    assert kept >= 8
    assert not (np.abs(dets[0, :counts[0], :4] - np.array([29.5, 58.0, 34.5, 62.0], np.float32)).max(1) < 1e-3).any()      # a_x is gone
    if agnostic:        # filtering the rows of the unfiltered call afterwards is NOT the same: an excluded box has suppressed a wanted one
        plain, pc = eng.nms(pred_d, conf, iou, STRIDE, True)
        plain, pc = plain.cpu().numpy(), pc.cpu().numpy()
        after = [plain[b, :pc[b]][np.isin(plain[b, :pc[b], 5], classes)] for b in range(B)]
        assert any(len(after[b]) < counts[b] for b in range(B)), ([len(x) for x in after], counts.tolist())


def test_the_global_scratch_form_takes_the_rows_too():
    """640 x 640 (8400 anchors), B = 2: frame 0's row lets every anchor in (more than 2048 candidates: keys, boxes and keep list in
    global scratch), frame 1's row is strict and small."""
    need_gpu()
    import vti_amd
    eng = _engine(80, 640, 640, 4)
    rng = np.random.default_rng(5)
    pred = synth_pred(rng, 2, 80, 32, 8400)
    pred[0, 4:84] = np.maximum(pred[0, 4:84], rng.uniform(0, 0.3, (80, 8400)).astype(np.float32))
    assert (pred[0, 4:84].max(0) > 0.05).sum() > 2048
    pred_d = torch.from_numpy(pred).cuda()
    P = vti_amd.NmsParams
    rows = [P(0.6, 0.7, 7, False), P(0.05, 0.5, 300, False, tuple(range(0, 80, 2)))]
    which = [1, 0]
    pred_z = excluded_zeroed(pred, 80, rows[1].classes)
    assert (pred_z[0, 4:84].max(0) > 0.05).sum() > 2048
    pred_zd = torch.from_numpy(pred_z).cuda()
    table = eng.pack_nms_table(rows)
    for scored in (False, True):
        best_d = torch.from_numpy(pairs(pred, 80)).cuda() if scored else None
        best_zd = torch.from_numpy(pairs(pred_z, 80)).cuda() if scored else None
        with eng.nms_table(table, which):
            dets, counts = eng.nms(pred_d, 0.9, 0.9, 300, True, best=best_d)
        torch.cuda.synchronize()
        got, n = dets.cpu().numpy(), counts.cpu().numpy()
        plain = dataclasses.replace(rows[1], classes=None)
        ref0, n0 = table_free(eng, pred_zd, best_zd, 0, plain, 300)
        ref1, n1 = table_free(eng, pred_d, best_d, 1, rows[0], 300)
        print("scored", scored, "counts", n.tolist(), "reference", n0, n1)
        assert n.tolist() == [n0, n1] and got[0].tobytes() == ref0.tobytes() and got[1].tobytes() == ref1.tobytes()
        assert n1 == 7 and n0 > 7


def test_predict_classes_end_to_end():
    """predict(frames, classes=[1]): class-aware NMS with every count below max_det keeps exactly the cls == 1 rows of predict(frames)
    -- boxes, conf, masks bit for bit; with agnostic_nms=True it is the table-free NMS on the pred without the excluded anchors."""
    need_gpu()
    import vti_amd
    from test_gpu_predict import _calibrated_model
    fr = frames_u8(2, 320, 320, seed=31)
    model = _calibrated_model(vti_amd, 2, "h2", fr[0], 320, 0.25, target=120)
    kw = dict(conf=0.25, iou=0.5, max_det=300, imgsz=320)
    full = model.predict(fr, **kw)
    only = model.predict(fr, classes=[1], **kw)
    both = model.predict(fr, classes=(0, 1), **kw)
    n1 = 0
    for r, o, e in zip(full, only, both):
        sel = r.boxes.data[:, 5] == 1
        k = int(sel.sum())
        print("instances", len(r.boxes.data), "of class 1", k)
        assert 0 < len(r.boxes.data) < 300
        assert torch.equal(e.boxes.data, r.boxes.data) and torch.equal(e.masks.bits, r.masks.bits)      # every class named: no filter
        if k == 0:
            assert o.masks is None and len(o.boxes.data) == 0
            continue
        assert torch.equal(o.boxes.data, r.boxes.data[sel]) and torch.equal(o.dets, r.dets[sel])
        assert torch.equal(o.masks.bits, r.masks.bits[sel]) and torch.equal(o.masks.data, r.masks.data[sel])
        n1 += k
    assert n1 > 0 and any((r.boxes.data[:, 5] == 0).any() for r in full)
    # agnostic: against the Engine-level reference on the pred this very predict made
    only = model.predict(fr, classes=1, agnostic_nms=True, **kw)
    eng = model._engine(320, 320, 2)
    pred = next(iter(model._outs.values()))["pred"][:2].clone()
    pred_z = torch.from_numpy(excluded_zeroed(pred.cpu().numpy(), 2, (1,))).cuda()
    dets, counts = eng.nms(pred_z, 0.25, 0.5, 300, True)
    for b, o in enumerate(only):
        n = int(counts[b])
        assert len(o.boxes.data) == n and (n == 0 or torch.equal(o.dets, dets[b, :n])), b
        assert n == 0 or (o.boxes.data[:, 5] == 1).all()
    assert int(counts.sum()) > 0
    # without classes the model packs no table; with them one per (engine, settings)
    assert len(model._nms_tables) == 1


def test_a_rig_with_thresholds_per_camera_equals_one_rig_per_camera():
    """mc.process_frames(frames, cameras, conf=[.2, .5], iou=[.25, .45], max_det=[200, 20]) gives the records of two
    MultiCameraMeasurers with those scalars, each fed only its camera's frames in order (two batches: the deques carry over)."""
    need_gpu()
    import vti_amd
    from test_gpu_measure_cameras import _params
    model = vti_amd.YOLO(None, scale="n", nc=2, seed=3, cls_bias=0.0)         # scores around 0.5: both thresholds cut, both limits bind
    params = [dataclasses.replace(_params(c, 960, 1280), drop_empty=False) for c in range(2)]
    mc = vti_amd.MultiCameraMeasurer(model, params, frame_buffer=8)
    scalar = [vti_amd.MultiCameraMeasurer(model, params, frame_buffer=8) for _ in range(2)]
    conf, iou, max_det = [0.2, 0.5], [0.25, 0.45], [200, 20]
    strip = lambda rec: {k: v for k, v in rec.items() if k != "timestamp"}
    for seed, cams in ((0, [0, 1, 1, 0]), (1, [1, 0, 0, 0])):
        frames = frames_u8(4, 960, 1280, seed)
        got = mc.process_frames(frames, cams, conf=conf, iou=iou, max_det=max_det, imgsz=960)
        counts = next(iter(model._outs.values()))["counts"].cpu().tolist()
        print("cameras", cams, "counts", counts)
        assert all(counts[b] <= max_det[c] for b, c in enumerate(cams)) and any(counts[b] > 20 for b, c in enumerate(cams) if c == 0)
        assert any(counts[b] > 0 for b, c in enumerate(cams) if c == 1)        # the strict camera still detects something
        exp = [None] * 4
        for c in range(2):
            mine = [b for b, x in enumerate(cams) if x == c]
            for b, rec in zip(mine, scalar[c].process_frames(frames[mine], [c] * len(mine), conf=conf[c], iou=iou[c], max_det=max_det[c],
                                                             imgsz=960)):
                exp[b] = rec
        for b, (g, e) in enumerate(zip(got, exp)):
            print("frame", b, strip(g))
            assert strip(g) == strip(e), b
        # and the settings matter: camera 1's frames under camera 0's scalars come out otherwise
        probe = vti_amd.MultiCameraMeasurer(model, params, frame_buffer=8)
        mine = [b for b, x in enumerate(cams) if x == 1]
        probe.process_frames(frames[mine], [1] * len(mine), conf=conf[0], iou=iou[0], max_det=max_det[0], imgsz=960)
        loose = next(iter(model._outs.values()))["counts"].cpu().tolist()
        assert loose != [counts[b] for b in mine], (loose, counts)
    with pytest.raises(ValueError, match="max_det has 3 entries"):
        mc.process_frames(frames, cams, max_det=[200, 20, 5])


def test_after_the_table_is_cleared_the_plain_call_is_what_it_was():
    need_gpu()
    import vti_amd
    eng = _engine(2)
    pred_d = torch.from_numpy(planted(2, 3, 7)).cuda()
    before = [t.clone() for t in eng.nms(pred_d, 0.25, 0.7, STRIDE)]
    table = eng.pack_nms_table([vti_amd.NmsParams(0.6, 0.2, 3, True, (0,))])
    with eng.nms_table(table):
        inside = [t.clone() for t in eng.nms(pred_d, 0.25, 0.7, STRIDE)]
    after = eng.nms(pred_d, 0.25, 0.7, STRIDE)
    torch.cuda.synchronize()
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    assert not torch.equal(before[1], inside[1]) and int(inside[1].max()) <= 3
    with pytest.raises(RuntimeError):           # the table is cleared when the block is left by an exception too
        with eng.nms_table(table):
            raise RuntimeError("left early")
    again = eng.nms(pred_d, 0.25, 0.7, STRIDE)
    assert torch.equal(before[0], again[0]) and torch.equal(before[1], again[1])
