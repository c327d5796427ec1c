"""-m gpu: vti_mask_polygons_frames -- the polygons of a batch whose frames differ in size in one call.  Every frame's vertices are
compared bit for bit with vti_mask_polygons called on that frame's slots alone (letterbox bits with the frame's H0, W0; ragged
native rows as the uniform buffer Engine.frame_masks cuts) and with the host restatement polygons.masks2segments + scale_coords:
both strategies, both forms (image in LDS / in the scratch) in one call, capacity and capacity_bytes cuts over poisoned buffers, a
points buffer that is too small, scratch reuse, and YOLO.predict(..., polygons=True)."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpu_util import need_gpu
from test_gpu_polygons import _assert_same, _host, _pack, _random_blobs

pytestmark = pytest.mark.gpu

H = W = 64                                          # the engine's canvas
SHAPES = [(48, 64), (32, 64), (37, 53), (64, 40)]
COUNTS = [3, 0, 5, 2]                               # one frame has no instance
MAX_DET = 5
STRATEGY = {"largest": 0, "concat": 1}


def _engine():
    import vti_amd
    return vti_amd.Engine("n", 2, H=H, W=W, max_batch=4)


def _masks(n, h, w, seed):
    """n 0/1 masks of h x w: seeded blobs (rings with islands in their holes, speckle, lines, dots), of which the first four are
    replaced by an island inside a hole that touches all four borders, a full mask, an empty one and a frame-shaped ring."""
    m = _random_blobs(max(n, 5), h, w, seed)[:n]
    special = np.zeros((4, h, w), np.uint8)
    special[0] = 1
    special[0, 2:h - 2, 2:w - 2] = 0                # the hole of a mask that touches every border ...
    special[0, h // 2 - 3:h // 2 + 3, w // 2 - 4:w // 2 + 4] = 1      # ... and an island in it, with more corners than the ring
    special[0, h // 2, w // 2 - 4] = 0
    special[0, h // 2 - 1, w // 2 + 3] = 0
    special[1] = 1
    special[3, 1:h - 1, 1:w - 1] = 1
    special[3, 4:h - 4, 4:w - 4] = 0
    m[:min(n, 4)] = special[:min(n, 4)]
    return m


def _letterbox_set(counts=COUNTS, seed=40):
    """A hand-made output set of predict_frames_into: letterbox bit masks [capacity, 64, 8], the pool of masks and offsets."""
    total = sum(counts)
    pool = _masks(total, H, W, seed)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    cap = len(counts) * MAX_DET
    bits = torch.full((cap, H, W // 8), 0xFF, dtype=torch.uint8, device="cuda")      # slots past the live ones: never read
    bits[:total] = _pack(pool, W // 8)
    out = dict(masks=bits, offsets=torch.from_numpy(off).cuda(), counts=torch.tensor(counts, dtype=torch.int32, device="cuda"),
               dets=torch.zeros((len(counts), MAX_DET, 38), device="cuda"))
    return out, pool, off


def _ragged_set(eng, shapes, counts, seed=50, max_det=MAX_DET):
    """The ragged output set of predict_frames_into(native=True), hand-made: frame b's masks at H0[b] x W0[b] in rows of
    8 * ceil(W0[b] / 64) bytes whose pad bits hold garbage, back to back in a buffer that is poisoned past the last slot."""
    table, _, _ = eng.pack_frames(shapes, "cuda")
    slot = [eng.mask_native_layout(h, w)["slot_bytes"] for h, w in shapes]
    bases = np.concatenate([[0], np.cumsum([n * s for n, s in zip(counts, slot)])]).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    flat = torch.full((int(bases[-1]) + 4096,), 0xFF, dtype=torch.uint8, device="cuda")
    per_frame = []
    for b, ((h, w), n) in enumerate(zip(shapes, counts)):
        m = _masks(n, h, w, seed + b) if n else np.zeros((0, h, w), np.uint8)
        per_frame.append(m)
        if n:
            flat[int(bases[b]):int(bases[b + 1])] = _pack(m, 8 * -(-w // 64), garbage_seed=seed + b).reshape(-1)
    out = dict(masks=flat, offsets=torch.from_numpy(off).cuda(), counts=torch.tensor(counts, dtype=torch.int32, device="cuda"),
               dets=torch.zeros((len(shapes), max_det, 38), device="cuda"), mask_bases=torch.from_numpy(bases).cuda(),
               native_shapes=tuple(table.shapes))
    return out, table, per_frame, off, bases, slot


def _split(pts, po):
    p, o = pts.cpu().numpy(), po.cpu().numpy()
    assert o[0] == 0 and np.all(np.diff(o) >= 0) and o[-1] == len(p)
    return [p[o[i]:o[i + 1]] for i in range(len(o) - 1)]


def _frames_call(eng, out, table, native, strategy):
    return _split(*eng.mask_polygons_frames(out, table, native=native, strategy=strategy))


def _uniform_call(eng, bits, w, h0, w0, strategy):
    return _split(*eng.mask_polygons(bits, w, h0, w0, strategy))


def _raw_call(eng, out, table, native, capacity, capacity_bytes, strategy, points, ws=None):
    """The C call itself -> (rc, point_offsets i32 [capacity + 1], status word)."""
    import vti_amd
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    if ws is None:
        ws = torch.empty(eng.mask_polygons_frames_scratch_bytes(table, native), dtype=torch.uint8, device="cuda")
    po = torch.full((capacity + 1,), -5, dtype=torch.int32, device="cuda")
    rc = vti_amd.lib().vti_mask_polygons_frames(
        eng._ctx, p(out["masks"]), int(native), p(out["mask_bases"]) if native else None, capacity_bytes, p(out["offsets"]),
        *table._ptrs(), table.B, capacity, STRATEGY[strategy], p(ws), ws.numel(), p(po), p(points), points.shape[0],
        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, po, int(ws[:4].view(torch.int32)[0])


@pytest.mark.parametrize("strategy", ["largest", "concat"])
def test_letterbox_masks_are_mask_polygons_per_frame_and_the_host(strategy):
    need_gpu()
    eng = _engine()
    out, pool, off = _letterbox_set()
    table, _, _ = eng.pack_frames(SHAPES, "cuda")
    got = _frames_call(eng, out, table, False, strategy)
    assert len(got) == len(SHAPES) * MAX_DET
    for b, (h0, w0) in enumerate(SHAPES):
        mine = got[off[b]:off[b + 1]]
        _assert_same(mine, _uniform_call(eng, out["masks"][off[b]:off[b + 1]], W, h0, w0, strategy), (strategy, b, "device"))
        _assert_same(mine, _host(pool[off[b]:off[b + 1]], strategy, h0, w0), (strategy, b, "host"))
    assert all(g.shape == (0, 2) for g in got[off[-1]:])                  # slots at and beyond offsets[B]: poisoned, not read
    assert got[2].shape == (0, 2) and sum(len(g) for g in got) > 100      # the empty mask (the pool's third); the rest is not trivial


@pytest.mark.parametrize("strategy", ["largest", "concat"])
def test_ragged_native_rows_are_mask_polygons_per_frame_and_the_host(strategy):
    """W0 = 53 and W0 = 40: 11 and 24 pad bits per 8-byte row, filled with garbage."""
    need_gpu()
    eng = _engine()
    out, table, per_frame, off, bases, _ = _ragged_set(eng, SHAPES, COUNTS)
    got = _frames_call(eng, out, table, True, strategy)
    assert len(got) == len(SHAPES) * MAX_DET
    for b, (h0, w0) in enumerate(SHAPES):
        mine = got[off[b]:off[b + 1]]
        view = eng.frame_masks(out["masks"], table, b, int(bases[b]), COUNTS[b])
        assert view.shape[0] == COUNTS[b]
        _assert_same(mine, _uniform_call(eng, view, w0, h0, w0, strategy), (strategy, b, "device"))
        _assert_same(mine, _host(per_frame[b], strategy, h0, w0), (strategy, b, "host"))
    assert all(g.shape == (0, 2) for g in got[off[-1]:])


_TALL = {}


def _tall_host(strategy, m):
    if strategy not in _TALL:                       # the host tracer on 1100 x 1280 masks: once per strategy
        _TALL[strategy] = _host(m, strategy, 1100, 1280)
    return _TALL[strategy]


@pytest.mark.parametrize("strategy", ["largest", "concat"])
def test_both_forms_in_one_call_in_either_order(strategy):
    """1100 * 20 * 8 B = 176 000 B is more than the 156 KiB LDS image, so the 1100 x 1280 frame's slots are traced in the scratch
    form and the 48 x 64 frame's in the LDS form, by the same call."""
    need_gpu()
    eng = _engine()
    tall = np.zeros((2, 1100, 1280), np.uint8)
    tall[0, 10:1090, 20:1270] = 1
    tall[0, 400:700, 300:900] = 0
    tall[0, 500:600, 500:700] = 1                   # an island in the hole
    tall[1, 1099, :] = 1
    tall[1, :, 0] = 1
    tall[1, 0, :] = 1
    tall[1, :, 1279] = 1                            # all four borders
    tall[1, 50:60, 1200:1280] = 1
    for order in ((0, 1), (1, 0)):
        shapes = [[(1100, 1280), (48, 64)][k] for k in order]
        counts = [[2, 3][k] for k in order]
        out, table, per_frame, off, bases, _ = _ragged_set(eng, shapes, counts, max_det=3)
        t = order.index(0)                          # where the tall frame is
        at = int(bases[t])
        out["masks"][at:at + 2 * 1100 * 160] = _pack(tall, 160).reshape(-1)
        per_frame[t] = tall
        assert eng.mask_polygons_frames_scratch_bytes(table, True) == eng.mask_polygons_scratch_bytes(1100, 1280, 160)
        got = _frames_call(eng, out, table, True, strategy)
        for b, (h0, w0) in enumerate(shapes):
            mine = got[off[b]:off[b + 1]]
            view = eng.frame_masks(out["masks"], table, b, int(bases[b]), counts[b])
            _assert_same(mine, _uniform_call(eng, view, w0, h0, w0, strategy), (strategy, order, b, "device"))
            ref = _tall_host(strategy, tall) if b == t else _host(per_frame[b], strategy, h0, w0)
            _assert_same(mine, ref, (strategy, order, b, "host"))
        assert all(g.shape == (0, 2) for g in got[off[-1]:])


def _check_cut(got, ref, live):
    _assert_same(got[:live], ref[:live])
    assert all(g.shape == (0, 2) for g in got[live:])


def test_capacity_and_capacity_bytes_cut_in_the_middle_of_a_frame():
    """Every slot that is not live has 0 vertices, and what the mask buffer holds behind the cut does not matter."""
    need_gpu()
    eng = _engine()
    table, _, _ = eng.pack_frames(SHAPES, "cuda")
    points = torch.empty((1 << 14, 2), dtype=torch.float32, device="cuda")
    # letterbox masks, capacity = 5: frame 2 (slots 3 .. 7) keeps two of its five, frame 3 none
    out, pool, off = _letterbox_set()
    ref = _frames_call(eng, out, table, False, "concat")
    results = []
    for poison in (0xFF, 0x00, 0x5A):
        out["masks"][5:] = poison
        rc, po, status = _raw_call(eng, out, table, False, 5, 0, "concat", points)
        assert rc == 0 and status == 0
        _check_cut(_split(points[:int(po[-1])], po), ref, 5)
        results.append((po.cpu().numpy().tobytes(), points[:int(po[-1])].cpu().numpy().tobytes()))
    assert results[0] == results[1] == results[2]
    # the ragged rows, capacity = 5 of the 20 slots: the same cut by the slot index
    out, table, per_frame, off, bases, slot = _ragged_set(eng, SHAPES, COUNTS)
    ref = _frames_call(eng, out, table, True, "concat")
    total_bytes = out["masks"].numel()
    results = []
    for poison in (0xFF, 0x00):
        out["masks"][int(bases[2]) + 2 * slot[2]:] = poison
        rc, po, status = _raw_call(eng, out, table, True, 5, total_bytes, "concat", points)
        assert rc == 0 and status == 0
        _check_cut(_split(points[:int(po[-1])], po), ref, 5)
        results.append((po.cpu().numpy().tobytes(), points[:int(po[-1])].cpu().numpy().tobytes()))
    assert results[0] == results[1]
    # capacity_bytes ends inside frame 2's third slot: two of its slots are live; point_offsets is constant from there on
    cut = int(bases[2]) + 2 * slot[2] + 100
    results = []
    for poison in (0xFF, 0x00):
        out["masks"][cut - 100:] = poison
        rc, po, status = _raw_call(eng, out, table, True, len(SHAPES) * MAX_DET, cut, "concat", points)
        assert rc == 0 and status == 0
        _check_cut(_split(points[:int(po[-1])], po), ref, 5)
        o = po.cpu().numpy()
        assert np.all(o[5:] == o[5]) and o[5] == sum(len(r) for r in ref[:5])
        results.append((o.tobytes(), points[:int(po[-1])].cpu().numpy().tobytes()))
    assert results[0] == results[1]
    # capacity_bytes = 0 and capacity = 0: nothing is live
    rc, po, status = _raw_call(eng, out, table, True, len(SHAPES) * MAX_DET, 0, "largest", points)
    assert rc == 0 and status == 0 and torch.all(po == 0)
    rc, po, status = _raw_call(eng, out, table, True, 0, total_bytes, "largest", points)
    assert rc == 0 and status == 0 and po.tolist() == [0]


def test_too_few_points_and_scratch_reuse():
    need_gpu()
    eng = _engine()
    out, table, per_frame, off, bases, _ = _ragged_set(eng, SHAPES, COUNTS)
    cap = len(SHAPES) * MAX_DET
    ref_pts, ref_po = eng.mask_polygons_frames(out, table, native=True, strategy="concat")
    ref_pts, ref_po = ref_pts.clone(), ref_po.clone()
    total = int(ref_po[-1])
    assert total > 50
    ws = torch.empty(eng.mask_polygons_frames_scratch_bytes(table, True), dtype=torch.uint8, device="cuda")
    small = torch.full((total - 1, 2), -3.0, device="cuda")                # one vertex short
    rc, po, status = _raw_call(eng, out, table, True, cap, out["masks"].numel(), "concat", small, ws)
    assert rc == 0 and status == 0 and torch.equal(po, ref_po) and torch.all(small == -3.0)
    room = torch.full((total, 2), -3.0, device="cuda")
    rc, po, status = _raw_call(eng, out, table, True, cap, out["masks"].numel(), "concat", room, ws)
    assert rc == 0 and status == 0 and torch.equal(po, ref_po)
    assert torch.equal(room.view(torch.int32), ref_pts.view(torch.int32))
    # the engine's own second launch when its kept buffer is too small
    eng._poly_points = torch.full((max(total // 3, 1), 2), -7.0, device="cuda")
    kept = eng._poly_points
    pts, po = eng.mask_polygons_frames(out, table, native=True, strategy="concat")
    assert torch.equal(pts.view(torch.int32), ref_pts.view(torch.int32)) and torch.equal(po, ref_po) and torch.all(kept == -7.0)
    # other masks through the same kept scratch: the bytes of a fresh engine
    lb, _, _ = _letterbox_set(seed=77)
    for strategy in ("largest", "concat"):
        used = [t.clone() for t in eng.mask_polygons_frames(lb, table, strategy=strategy)]
        fresh = [t.clone() for t in _engine().mask_polygons_frames(lb, table, strategy=strategy)]
        assert torch.equal(used[0].view(torch.int32), fresh[0].view(torch.int32)) and torch.equal(used[1], fresh[1])


def _frames(shapes, seed=4):
    return [np.random.Generator(np.random.PCG64(seed * 100 + k)).integers(0, 256, (h, w, 3), dtype=np.uint8)
            for k, (h, w) in enumerate(shapes)]


def _count_calls(monkeypatch, vti_amd):
    seen = {"vti_mask_polygons": 0, "vti_mask_polygons_frames": 0}
    L = vti_amd.lib()
    for name in seen:
        def wrapper(*a, _f=getattr(L, name), _n=name):
            seen[_n] += 1
            return _f(*a)
        monkeypatch.setattr(L, name, wrapper)
    return seen


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("retina", [False, True])
def test_predict_polygons_makes_the_batch_in_one_call(monkeypatch, retina, drop):
    need_gpu()
    import vti_amd
    shapes = [(480, 640), (24, 32), (481, 333)]     # the tiny frame is there so that all-zero masks occur
    frames = _frames(shapes)
    kw = dict(conf=0.25, iou=0.7, max_det=50, imgsz=640, retina_masks=retina, mixed=retina)
    model = vti_amd.YOLO(None, scale="n", nc=2, seed=3, cls_bias=-1.0, dtype="h2", drop_empty_masks=drop)
    lazy = model.predict(frames, **kw)
    want = [(r.masks.xy, r.masks.xyn) if r.masks is not None else None for r in lazy]      # the per-frame calls
    seen = _count_calls(monkeypatch, vti_amd)
    res = model.predict(frames, polygons=True, **kw)
    assert seen == {"vti_mask_polygons": 0, "vti_mask_polygons_frames": 1}
    n = 0
    for r, w, l in zip(res, want, lazy):
        assert (r.masks is None) == (w is None) and len(r) == len(l)
        if w is None:
            continue
        assert r.masks._xy is not None                                      # made before predict returned
        _assert_same(r.masks.xy, w[0])
        _assert_same(r.masks.xyn, w[1])
        n += len(w[0])
    assert n >= 3 and seen == {"vti_mask_polygons": 0, "vti_mask_polygons_frames": 1}       # .xy / .xyn touched no device
    if not retina:                                  # frames of one size: one vti_mask_polygons call over the live slots
        same = [frames[0], frames[0][::-1].copy()]
        lazy = model.predict(same, **kw)
        want = [r.masks.xy if r.masks is not None else None for r in lazy]
        seen.update({k: 0 for k in seen})
        res = model.predict(same, polygons=True, **kw)
        assert seen == {"vti_mask_polygons": 1, "vti_mask_polygons_frames": 0}
        for r, w in zip(res, want):
            assert (r.masks is None) == (w is None)
            if w is not None:
                _assert_same(r.masks.xy, w)
        assert seen == {"vti_mask_polygons": 1, "vti_mask_polygons_frames": 0} and any(w for w in want)
