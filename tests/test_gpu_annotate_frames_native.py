"""-m gpu: vti_annotate_frames_native / vti_annotate_checker_frames_native -- the pictures of a batch whose frames differ in size,
drawn from the ragged frame-size rows of vti_masks_native_frames.  Every picture and status is compared byte for byte with
vti_annotate(native = 1) (checker: vti_annotate_checker_cameras(native = 1)) called with B = 1 at that frame's size on the frame's
run of slots as a uniform buffer -- in which `capacity` cuts the slot index and a slot cut by capacity_bytes is what the family's
measurement made of it: all zeros with its rows (vti_measure_frames_native wrote them for an empty mask), or for the checker a slot
beyond the capacity (vti_measure_checker_frames_native writes no row for it, so there is none to read) -- and with
the restatement annotate.rasterise(frame, annotate.display_list(...) / checker_display_list(...)) fed the frame-size masks and the
rows the device wrote.  The batch is test_gpu_measure_frames.batch_plan() as test_gpu_measure_frames_native.build_ragged lays it
out (four sizes: the 333-wide one has a partial last word; an empty frame between two that have instances, so two bases are
equal; a camera index outside the table) with one 1080 x 1920 frame of status OK appended, so that both tracer forms draw."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import annotate_util as U
from gpu_util import need_gpu
from test_gpu_measure import MAX_DET, _engine, scenes, unpack
from test_gpu_measure_cameras import CALIBS
from test_gpu_measure_frames import BAD, CAMS, MH, MW, NARROW, _params, batch_plan
from test_gpu_measure_frames_native import _filled, build_ragged
from vti_amd import annotate as A

pytestmark = pytest.mark.gpu
POISON = 0xA5
GUARD = 4096
CUT = (7, 5, 4096)              # capacity_bytes ends 4096 bytes into the sixth slot of frame 7: every later slot is cut too
ROWS_CUT = (5, 3)               # `capacity` ends after the third slot of frame 5: its fabric (the last instance) has no slot
KINDS = ("uncut", "bytes", "rows")
FAMILIES = ("annotate", "annotate_checker")


def plan():
    return batch_plan() + [(scenes()[0], (1080, 1920), 0)]


def _camera_params(fam):
    """Two cameras per family; camera 1 drops empty masks, so that the scan of a fabric mask's rows runs on the ragged rows too."""
    import vti_amd
    if fam == "annotate":
        return [_params(0), dataclasses.replace(_params(1), drop_empty=True)]
    return [vti_amd.CheckerParams(*CALIBS[CAMS[0][0]]), vti_amd.CheckerParams(*CALIBS[CAMS[1][0]], min_stitches=2, drop_empty=True)]


@functools.lru_cache(maxsize=None)
def _base():
    """The hand-made ragged set, its frames and the two camera tables: computed once, shared by the tests, never changed."""
    eng = _engine(MH, MW, 16)
    pl = plan()
    dev, table, ref, offsets, bases, slot, capacity_bytes, live_slots = build_ragged(eng, pl, CUT)
    shapes = [hw for _, hw, _ in pl]
    assert sorted(set(shapes)) == [NARROW, (720, 960), (960, 1280), (1080, 1920)] and NARROW[1] % 64 != 0
    assert pl[2][0] == [] and pl[1][0] and pl[3][0] and bases[2] == bases[3]           # the empty frame: two equal bases
    assert [c for _, _, c in pl].count(BAD) == 1
    assert int(bases[CUT[0]]) < capacity_bytes < int(bases[CUT[0] + 1]) and CUT[0] < len(pl) - 2
    full = dev["masks"]                                          # slots from live_slots on are 0xFF: never to be read
    whole = _filled(eng, pl, full, bases, slot, offsets)
    frames = [np.random.Generator(np.random.PCG64(900 + b)).integers(0, 256, (h, w, 3), dtype=np.uint8) for b, (h, w) in enumerate(shapes)]
    flat = np.zeros(table.total_bytes, np.uint8)
    for f, at in zip(frames, table.byte_offsets):
        flat[at:at + f.size] = f.reshape(-1)
    idx = torch.tensor([c for _, _, c in pl], dtype=torch.int32, device="cuda")
    cams = dict(annotate=eng.pack_cameras(_camera_params("annotate"), "cuda"),
                annotate_checker=eng.pack_checker_cameras(_camera_params("annotate_checker"), "cuda"))
    cap_rows = int(offsets[ROWS_CUT[0]]) + ROWS_CUT[1]
    assert ROWS_CUT[1] < len(pl[ROWS_CUT[0]][0]) and pl[ROWS_CUT[0]][0][-1]["cls"] == 1
    return dict(eng=eng, plan=pl, shapes=shapes, dev=dev, table=table, ref=ref, offsets=offsets, bases=bases, slot=slot,
                capacity_bytes=capacity_bytes, full=full, whole=whole, frames=frames, flat=flat, dflat=torch.from_numpy(flat).cuda(),
                idx=idx, cams=cams, cap_rows=cap_rows, B=len(pl))


def _draw(s, fam, *a, **kw):
    return getattr(s["eng"], fam)(*a, **kw)


def _pictures(buf, shapes, offsets):
    host = buf.cpu().numpy()
    return [host[at:at + 3 * h * w].reshape(h, w, 3) for (h, w), at in zip(shapes, offsets)]


@functools.lru_cache(maxsize=None)
def _case(kind, fam):
    """One family's measurement and its all-frames pictures (poisoned output with a guard behind it, poisoned scratch) for
    uncut: every slot written, the whole buffer;  bytes: the buffer truncated at capacity_bytes, which ends inside a slot of frame
    7 (the bytes behind it were 0xFF);  rows: every slot written, the per-slot rows of the measurement cut inside frame 5."""
    s = _base()
    eng, B, table, idx, cams = s["eng"], s["B"], s["table"], s["idx"], s["cams"][fam]
    masks = s["full"][:s["capacity_bytes"]] if kind == "bytes" else s["whole"]
    out = dict(s["dev"], masks=masks)
    measure = eng.measure if fam == "annotate" else eng.measure_checker
    meas = measure(out, cams, cameras=idx, frames=table, native=True)
    assert meas["stitch_i32"].shape[0] == B * MAX_DET
    cap = B * MAX_DET
    if kind == "rows":
        cap = s["cap_rows"]
        meas = dict(meas, stitch_f64=meas["stitch_f64"][:cap], stitch_i32=meas["stitch_i32"][:cap])
    sel = list(range(B))
    first = _draw(s, fam, s["dflat"], out, meas, cams, sel, cameras=idx, table=table, native=True)      # allocates the scratch
    eng._annotate_ws.fill_(POISON)
    total = first["table"].total_bytes
    guard = torch.full((total + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    res = dict(buf=guard[:total], status=torch.full((B,), -7, dtype=torch.int32, device="cuda"))
    got = _draw(s, fam, s["dflat"], out, meas, cams, sel, cameras=idx, table=table, native=True, result=res)
    torch.cuda.synchronize()
    host = {k: meas[k].cpu().numpy() for k in ("frame_i32", "stitch_f64", "stitch_i32")}
    return dict(out=out, meas=meas, cap=cap, got=got, guard=guard.cpu().numpy(), status=got["status"].cpu().tolist(),
                pics=_pictures(got["buf"], got["shapes"], got["byte_offsets"]), host=host, masks_host=masks.cpu().numpy())


def _uniform_slots(s, c, b, fam):
    """Frame b's run of slots as the uniform [n, H0, row_bytes] buffer of the reference call (host): the slots whose index is below
    the capacity; of those, one that does not end inside the mask buffer is all zeros -- or, for the checker, is not there (the
    capacity of its reference call ends in front of it).  -> (buffer, slots read from the masks, slots the bytes cut away)."""
    h, w = s["shapes"][b]
    n, lo = len(s["plan"][b][0]), int(s["offsets"][b])
    n_idx = max(0, min(n, c["cap"] - lo))
    sb, rb = s["slot"][b], s["slot"][b] // h
    base = int(s["bases"][b])
    n_read = max(0, min(n_idx, (c["masks_host"].size - base) // sb))
    cut = n_idx - n_read
    if fam == "annotate_checker":
        n_idx = n_read
    buf = np.zeros((n_idx, h, rb), np.uint8)
    buf[:n_read] = c["masks_host"][base:base + n_read * sb].reshape(n_read, h, rb)
    return buf, n_read, cut


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("kind", KINDS)
def test_every_picture_is_the_uniform_native_call_on_the_frames_run_of_slots(kind, fam):
    need_gpu()
    s, c = _base(), _case(kind, fam)
    eng, dev, idx, cams = s["eng"], s["dev"], s["idx"], s["cams"][fam]
    drawn, zeroed, no_row = 0, 0, 0
    for b, (h, w) in enumerate(s["shapes"]):
        n, lo = len(s["plan"][b][0]), int(s["offsets"][b])
        ubuf, n_read, cut = _uniform_slots(s, c, b, fam)
        n_idx = ubuf.shape[0]
        zeroed += cut
        no_row += n - n_idx - (cut if fam == "annotate_checker" else 0)
        if kind != "bytes":
            view = eng.frame_masks(c["out"]["masks"], s["table"], b, int(s["bases"][b]), n_idx)      # Engine's own cut of the run
            assert n_read == n_idx and np.array_equal(view.cpu().numpy(), ubuf)
        rows = max(n_idx, 1)                                     # an empty run still passes rows (never read: capacity 0)
        pad = lambda t: t if t.shape[0] else torch.zeros((1,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
        meas_b = dict(frame_i32=c["meas"]["frame_i32"][b:b + 1], stitch_f64=pad(c["meas"]["stitch_f64"][lo:lo + n_idx]),
                      stitch_i32=pad(c["meas"]["stitch_i32"][lo:lo + n_idx]))
        assert meas_b["stitch_i32"].shape[0] == rows
        view = dict(dets=dev["dets"][b:b + 1], xyxy=dev["xyxy"][b:b + 1], counts=dev["counts"][b:b + 1],
                    offsets=torch.tensor([0, n], dtype=torch.int32, device="cuda"), masks=torch.from_numpy(ubuf).cuda())
        dense = torch.from_numpy(s["frames"][b][None]).cuda()
        one = _draw(s, fam, dense, view, meas_b, cams, [0], native=True, cameras=idx[b:b + 1])
        want, status = one["frames"][0].cpu().numpy(), int(one["status"][0])
        diff = int((want != c["pics"][b]).any(axis=-1).sum())
        print(f"{kind} {fam} frame {b} {h}x{w}: {n} instances, {n_idx} with a row, {n_read} read; status {c['status'][b]} / {status}, "
              f"differing pixels {diff}")
        assert diff == 0 and c["status"][b] == status == 0, (b, diff)
        drawn += int((want != s["frames"][b]).any())
    assert drawn >= 7                                            # (a camera that drops empty masks draws nothing of a frame cut away)
    assert (zeroed > 0) == (kind == "bytes") and (no_row > 0) == (kind == "rows")


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("kind", ["uncut", "bytes"])
def test_every_picture_equals_the_restatement(kind, fam):
    need_gpu()
    s, c = _base(), _case(kind, fam)
    xy = s["dev"]["xyxy"].cpu().numpy()
    params = _camera_params(fam)
    lister = A.display_list if fam == "annotate" else A.checker_display_list
    outlined, statuses = set(), []
    for b, ((cls, _, _), (h, w), (_, _, cam)) in enumerate(zip(s["ref"], s["shapes"], s["plan"])):
        ubuf, n_read, cut = _uniform_slots(s, c, b, fam)
        # the frame-size masks the device saw: a cut slot is all zeros, or for the checker has no slot (None) and no row
        ms = [unpack(ubuf[i], w) if i < ubuf.shape[0] else None for i in range(len(cls))]
        assert ubuf.shape[0] + (cut if fam == "annotate_checker" else 0) == len(cls) and all(not m.any() for m in ms[n_read:ubuf.shape[0]])
        rows = U.device_rows(c["host"], b, s["offsets"], min(c["cap"], int(s["offsets"][b]) + ubuf.shape[0]), len(cls))
        prims, word = lister(h, w, cls, xy[b, :len(cls)], ms, rows, params[cam if cam != BAD else 0], max_points=U.MAX_POINTS,
                             with_status=True)
        want = A.rasterise(s["frames"][b], prims)
        diff = np.argwhere((c["pics"][b] != want).any(axis=-1))
        print(f"{kind} {fam} frame {b} {h}x{w}: measure status {rows['status']}, primitives {len(prims)}, differing pixels {len(diff)}"
              + (f" first at (y, x) {diff[0].tolist()}" if len(diff) else ""))
        assert len(diff) == 0 and word == c["status"][b] == 0, (b, len(diff), diff[:5].tolist())
        statuses.append(rows["status"])
        if cam == BAD:
            assert rows["status"] == A.BAD_CAMERA and prims == [] and np.array_equal(c["pics"][b], s["frames"][b])      # a plain copy
        if rows["status"] == A.OK and any(q[0] == "polyline" and q[2] for q in prims):
            outlined.add((h, w))
    print("statuses", statuses, "outlined", sorted(outlined))
    assert {A.NO_FABRIC, A.NO_STITCHES, A.BAD_CAMERA} <= set(statuses)
    if kind == "uncut" and fam == "annotate":                    # the global-image tracer and the LDS tracer, the partial last word
        assert statuses.count(A.OK) >= 4
        assert 8 * 960 * -(-1280 // 64) <= 156 * 1024 < 8 * 1080 * -(-1920 // 64)
        assert {(1080, 1920), (960, 1280), NARROW} <= outlined


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("kind", KINDS)
def test_only_the_pictures_are_written(kind, fam):
    need_gpu()
    s, c = _base(), _case(kind, fam)
    out, offs = c["guard"], c["got"]["byte_offsets"]
    total = c["got"]["table"].total_bytes
    assert c["got"]["shapes"] == s["shapes"] and c["got"]["buf"].numel() == total
    assert (out[total:] == POISON).all() and len(out) == total + GUARD       # the guard behind the last picture
    end, gap_bytes = 0, 0
    for (h, w), at in zip(s["shapes"], offs):
        assert (out[end:at] == POISON).all(), (end, at)                       # the gap in front of this picture
        gap_bytes += at - end
        end = at + 3 * h * w
    assert (out[end:total] == POISON).all() and gap_bytes > 0
    assert np.array_equal(s["dflat"].cpu().numpy(), s["flat"])                # dev_frames is read only
    if kind == "bytes":          # the buffer ended at capacity_bytes, inside a slot, and what lay behind it was 0xFF
        assert c["out"]["masks"].numel() == s["capacity_bytes"] and (s["full"][s["capacity_bytes"]:].cpu().numpy() == 0xFF).all()
        assert (s["capacity_bytes"] - int(s["bases"][CUT[0]])) % s["slot"][CUT[0]] == CUT[2]


@pytest.mark.parametrize("fam", FAMILIES)
def test_any_selection_and_the_pitches_of_small_selections(fam):
    need_gpu()
    s, c = _base(), _case("bytes", fam)
    eng, B, cams = s["eng"], s["B"], s["cams"][fam]
    small = [b for b in range(B) if s["shapes"][b] == NARROW]
    mid = [b for b in range(B) if s["shapes"][b] == (720, 960)]
    assert len(small) == 3 and len(mid) == 2
    # a subset, reversed order, duplicates, only the smallest frames (pitches 481 x 333), two sizes below the batch's maxima
    for sel in ([10, 1, 10, 4, 1], list(range(B))[::-1], [11], small, mid + small[:1], [6, 2]):
        eng._annotate_ws.fill_(POISON)
        got = _draw(s, fam, s["dflat"], c["out"], c["meas"], cams, sel, cameras=s["idx"], table=s["table"], native=True)
        assert got["shapes"] == [s["shapes"][b] for b in sel] and got["status"].cpu().tolist() == [c["status"][b] for b in sel]
        assert (got["table"].max_H0, got["table"].max_W0) == (max(s["shapes"][b][0] for b in sel), max(s["shapes"][b][1] for b in sel))
        for k, pic in enumerate(_pictures(got["buf"], got["shapes"], got["byte_offsets"])):
            assert np.array_equal(pic, c["pics"][sel[k]]), (sel, k)
    # capacity_bytes as an argument is the truncated buffer
    whole = dict(c["out"], masks=s["full"])
    got = _draw(s, fam, s["dflat"], whole, c["meas"], cams, [CUT[0], B - 1], cameras=s["idx"], table=s["table"], native=True,
                capacity_bytes=s["capacity_bytes"])
    for k, pic in enumerate(_pictures(got["buf"], got["shapes"], got["byte_offsets"])):
        assert np.array_equal(pic, c["pics"][[CUT[0], B - 1][k]]), k
    # capacity_bytes 0: no mask is read at all, every slot is an empty mask with its rows
    none = _draw(s, fam, s["dflat"], whole, c["meas"], cams, [0], cameras=s["idx"], table=s["table"], native=True, capacity_bytes=0)
    assert int(none["status"][0]) == 0
    with pytest.raises(ValueError):
        _draw(s, fam, s["dflat"], c["out"], c["meas"], cams, [B], cameras=s["idx"], table=s["table"], native=True)
    plain = dict(c["out"], masks=torch.zeros((4, MH, MW // 8), dtype=torch.uint8, device="cuda"))
    plain.pop("mask_bases")
    with pytest.raises(ValueError, match="mask_bases"):
        _draw(s, fam, s["dflat"], plain, c["meas"], cams, [0], cameras=s["idx"], table=s["table"], native=True)


@pytest.mark.parametrize("fam", FAMILIES)
def test_the_result_feeds_encode_jpeg_with_a_table(fam):
    need_gpu()
    from vti_amd import jpeg
    s, c = _base(), _case("uncut", fam)
    sel = [1, 5, 0]
    got = _draw(s, fam, s["dflat"], c["out"], c["meas"], s["cams"][fam], sel, cameras=s["idx"], table=s["table"], native=True)
    data, off = s["eng"].encode_jpeg(got["buf"], quality=90, table=got["table"])
    off = off.cpu().numpy()
    assert len(off) == len(sel) + 1 and (np.diff(off) > 0).all()
    k = 0                                                        # the 481 x 333 picture
    pic = c["pics"][sel[k]]
    assert (pic != s["frames"][sel[k]]).any()
    assert data[int(off[k]):int(off[k + 1])].cpu().numpy().tobytes() == jpeg.encode(pic, 90)


def _strip(rec):
    return {k: v for k, v in rec.items() if k != "timestamp"}


@pytest.mark.parametrize("how", ["retina_masks", "windows"])
def test_multi_camera_measurer_draws_the_mixed_list_from_its_frame_resolution_masks(how):
    """MultiCameraMeasurer.process_frames(list, cameras, retina_masks=True | windows="roi", mixed=True, annotate="all",
    annotate_native=True): every picture is the uniform Engine.annotate(native=True) at that frame's size on the call's own outputs
    (per-size sub-batches would be predicted on other letterbox canvases), and the records are those of the call without annotate."""
    need_gpu()
    import vti_amd
    model = vti_amd.YOLO(None, scale="n", nc=2, seed=3, cls_bias=-1.0)
    params = [dataclasses.replace(_params(c), drop_empty=False) for c in range(2)]
    sizes = [(640, 640), (481, 333), (720, 960), (640, 640), (480, 640)]
    cams = [0, 1, 1, 0, 1]
    kw = dict(conf=0.20, iou=0.25, max_det=200, imgsz=640, mixed=True)
    kw.update(dict(retina_masks=True) if how == "retina_masks" else dict(windows="roi"))
    frames = [np.random.Generator(np.random.PCG64(k)).integers(0, 256, (h, w, 3), dtype=np.uint8) for k, (h, w) in enumerate(sizes)]
    with pytest.raises(ValueError, match="retina_masks=True needs frames of one size"):
        vti_amd.MultiCameraMeasurer(model, params).process_frames(frames, cams, annotate="all", **kw)
    records = vti_amd.MultiCameraMeasurer(model, params, frame_buffer=8).process_frames(frames, cams, **kw)
    mc = vti_amd.MultiCameraMeasurer(model, params, frame_buffer=8)
    annotated, again = mc.process_frames(frames, cams, annotate="all", annotate_native=True, **kw)
    assert [_strip(r) for r in again] == [_strip(r) for r in records]
    assert [b for b, _, _ in annotated] == list(range(len(sizes)))
    (eng, table), = mc._tables.values()
    o, = model._outs.values()                                      # the output set the call measured and drew from
    assert "mask_bases" in o and o["masks"].dim() == 1
    ftab = next(iter(model._frame_tables.values()))[0] if how == "retina_masks" else next(iter(model._window_tables.values())).frames
    res, = mc._res.values()
    cnt, off, bases = o["counts"].cpu().tolist(), o["offsets"].cpu().tolist(), o["mask_bases"].cpu().tolist()
    assert sum(cnt) >= 4
    idx = torch.tensor(cams, dtype=torch.int32, device="cuda")
    drawn = 0
    for b, (h, w) in enumerate(sizes):
        n, lo = cnt[b], off[b]
        pad = lambda t: t if t.shape[0] else torch.zeros((1,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
        view = dict(dets=o["dets"][b:b + 1], xyxy=o["xyxy"][b:b + 1], counts=o["counts"][b:b + 1],
                    offsets=torch.tensor([0, n], dtype=torch.int32, device="cuda"), masks=eng.frame_masks(o["masks"], ftab, b, bases[b], n))
        assert view["masks"].shape[0] == n
        meas_b = dict(frame_i32=res["frame_i32"][b:b + 1], stitch_f64=pad(res["stitch_f64"][lo:lo + n]),
                      stitch_i32=pad(res["stitch_i32"][lo:lo + n]))
        one = eng.annotate(torch.from_numpy(frames[b][None]).cuda(), view, meas_b, table, [0], native=True, cameras=idx[b:b + 1])
        want = one["frames"][0].cpu().numpy()
        pic = annotated[b][1]
        diff = int((pic != want).any(axis=-1).sum())
        print(how, "frame", b, sizes[b], "camera", cams[b], "instances", n, "differing pixels", diff, _strip(again[b]))
        # (random weights give ragged masks: an outline may pass max_points and is then left out of both pictures alike)
        assert pic.shape == (h, w, 3) and diff == 0, b
        drawn += int((pic != frames[b]).any())
    assert drawn >= 2
    # the files of the same call: encode="jpeg" gives jpeg.encode of those pictures
    from vti_amd import jpeg
    files, _ = vti_amd.MultiCameraMeasurer(model, params, frame_buffer=8).process_frames(
        frames, cams, annotate=[1], encode="jpeg", jpeg_quality=90, annotate_native=True, **kw)
    assert files[0][0] == 1 and files[0][1] == jpeg.encode(annotated[1][1], 90)
