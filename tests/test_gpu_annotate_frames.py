"""-m gpu: vti_annotate_frames -- the annotated picture of the selected frames of a batch whose frames differ in size, each at its
own size.  Every picture is compared byte for byte with vti_annotate run at that frame's size on the same outputs, and with the
restatement annotate.rasterise(frame, annotate.display_list(...)) fed the rows the device wrote.  The batch is
test_gpu_measure_frames.batch_plan() -- four sizes (one odd, so that the next frame's offset is padded; one whose union fits the
tracer's LDS image and one whose union does not), two cameras, a camera index outside the table -- with two frames added so that
the largest size certainly has a frame with status OK and an empty frame sees a camera whose ROI is on."""
import functools

import numpy as np
import pytest
import torch

import annotate_util as U
from gpu_util import need_gpu
from test_gpu_measure import _engine, scenes
from test_gpu_measure_frames import BAD, MH, MW, NARROW, _params, batch_plan, build
from vti_amd import annotate as A

pytestmark = pytest.mark.gpu
POISON = 0xA5
GUARD = 4096
HOST_KEYS = ("frame_i32", "stitch_f64", "stitch_i32")


def plan():
    return batch_plan() + [(scenes()[0], (1080, 1920), 0), ([], NARROW, 1)]


def _flat(frames, table):
    flat = np.zeros(table.total_bytes, np.uint8)
    for f, at in zip(frames, table.byte_offsets):
        flat[at:at + f.size] = f.reshape(-1)
    return flat


def _pictures(buf, shapes, offsets):
    host = buf.cpu().numpy()
    return [host[at:at + 3 * h * w].reshape(h, w, 3) for (h, w), at in zip(shapes, offsets)]


def _setup(pl, dead=3, seed=5):
    eng = _engine(MH, MW, 16)
    shapes = [hw for _, hw, _ in pl]
    dev, ref, offsets, cap = build(pl, dead)
    table, _, _ = eng.pack_frames(shapes, "cuda")
    cams = eng.pack_cameras([_params(0), _params(1)], "cuda")
    idx = torch.tensor([c for _, _, c in pl], dtype=torch.int32, device="cuda")
    dev["xyxy"] = eng.scale_boxes(dev["dets"], dev["counts"], frames=table)
    meas = eng.measure(dev, cams, cameras=idx, frames=table)
    frames = [np.random.Generator(np.random.PCG64(seed * 100 + b)).integers(0, 256, (h, w, 3), dtype=np.uint8)
              for b, (h, w) in enumerate(shapes)]
    flat = _flat(frames, table)
    return dict(eng=eng, shapes=shapes, dev=dev, ref=ref, offsets=offsets, cap=cap, table=table, cams=cams, idx=idx, meas=meas,
                frames=frames, flat=flat, dflat=torch.from_numpy(flat).cuda(), plan=pl)


@functools.lru_cache(maxsize=None)
def _every():
    """The batch, and the all-frames call on a poisoned output and scratch: computed once, shared by the tests, never changed."""
    s = _setup(plan())
    eng, B = s["eng"], len(s["shapes"])
    first = eng.annotate(s["dflat"], s["dev"], s["meas"], s["cams"], list(range(B)), cameras=s["idx"], table=s["table"])   # allocates the scratch
    eng._annotate_ws.fill_(POISON)
    total = first["table"].total_bytes
    out = torch.full((total + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    res = dict(buf=out[:total], status=torch.full((B,), -7, dtype=torch.int32, device="cuda"))
    got = eng.annotate(s["dflat"], s["dev"], s["meas"], s["cams"], list(range(B)), cameras=s["idx"], table=s["table"], result=res)
    torch.cuda.synchronize()
    s.update(out=out.cpu().numpy(), got=got, status=got["status"].cpu().tolist(), pics=_pictures(got["buf"], got["shapes"], got["byte_offsets"]),
             host={k: s["meas"][k].cpu().numpy() for k in HOST_KEYS}, xy=s["dev"]["xyxy"].cpu().numpy())
    return s


@functools.lru_cache(maxsize=None)
def _restated():
    """Per frame (picture, status word, primitives) of the restatement, from the rows the device wrote."""
    s = _every()
    out = []
    for b, ((cls, ms), (h, w), (_, _, cam)) in enumerate(zip(s["ref"], s["shapes"], s["plan"])):
        rows = U.device_rows(s["host"], b, s["offsets"], s["cap"], len(cls))
        prims, word = A.display_list(h, w, cls, s["xy"][b, :len(cls)], ms, rows, _params(cam if cam != BAD else 0),
                                     max_points=U.MAX_POINTS, with_status=True)
        out.append((A.rasterise(s["frames"][b], prims), word, prims, rows["status"]))
    return out


def test_the_batch_crosses_every_per_frame_decision():
    need_gpu()
    s = _every()
    assert sorted(set(s["shapes"])) == [(481, 333), (720, 960), (960, 1280), (1080, 1920)]
    assert (3 * 481 * 333) % 16 != 0                                        # the frame behind a narrow one starts at a padded offset
    gaps = [s["got"]["byte_offsets"][k + 1] - (s["got"]["byte_offsets"][k] + 3 * h * w) for k, (h, w) in enumerate(s["shapes"][:-1])]
    assert max(gaps) > 0 and all(at % 16 == 0 for at in s["got"]["byte_offsets"])
    assert 8 * 960 * -(-1280 // 64) <= 156 * 1024 < 8 * 1080 * -(-1920 // 64)      # the tracer's LDS image: fits / does not fit
    assert s["got"]["table"].shapes == s["shapes"] and s["got"]["buf"].numel() == s["got"]["table"].total_bytes


def test_every_picture_equals_vti_annotate_at_that_frames_size():
    need_gpu()
    s = _every()
    eng, dev, B = s["eng"], s["dev"], len(s["shapes"])
    for h, w in sorted(set(s["shapes"])):
        rows = [b for b in range(B) if s["shapes"][b] == (h, w)]
        dense = np.zeros((B, h, w, 3), np.uint8)
        for b in rows:
            dense[b] = s["frames"][b]
        uni = dict(dev, xyxy=eng.scale_boxes(dev["dets"], dev["counts"], h, w))
        meas = eng.measure(uni, s["cams"], h, w, cameras=s["idx"])
        one = eng.annotate(torch.from_numpy(dense).cuda(), uni, meas, s["cams"], rows, cameras=s["idx"])
        pics, status = one["frames"].cpu().numpy(), one["status"].cpu().tolist()
        for k, b in enumerate(rows):
            diff = int((pics[k] != s["pics"][b]).any(axis=-1).sum())
            print(f"{h}x{w} frame {b}: status {s['status'][b]} / {status[k]}, differing pixels {diff}")
            assert diff == 0 and s["status"][b] == status[k], (b, diff)


def test_every_picture_equals_the_restatement():
    need_gpu()
    s = _every()
    for b, (want, word, prims, st) in enumerate(_restated()):
        diff = np.argwhere((s["pics"][b] != want).any(axis=-1))
        print(f"frame {b} {s['shapes'][b]}: measure status {st}, primitives {len(prims)}, differing pixels {len(diff)}"
              + (f" first at (y, x) {diff[0].tolist()}" if len(diff) else ""))
        assert len(diff) == 0 and word == s["status"][b] == 0, (b, len(diff), diff[:5].tolist())


def test_only_the_pictures_are_written():
    need_gpu()
    s = _every()
    out, offs = s["out"], s["got"]["byte_offsets"]
    total = s["got"]["table"].total_bytes
    assert (out[total:] == POISON).all() and len(out) == total + GUARD      # the guard behind the last picture
    end = 0
    gap_bytes = 0
    for (h, w), at in zip(s["shapes"], offs):
        assert (out[end:at] == POISON).all(), (end, at)                     # the gap in front of this picture
        gap_bytes += at - end
        end = at + 3 * h * w
    assert (out[end:total] == POISON).all() and gap_bytes > 0
    assert np.array_equal(s["dflat"].cpu().numpy(), s["flat"])              # dev_frames is read only


def test_any_selection_and_picture_k_depends_on_its_frame_only():
    need_gpu()
    s = _every()
    eng, B = s["eng"], len(s["shapes"])
    for sel in ([10, 1, 10, 4, 1], list(range(B))[::-1], [3], [1], [11, 6]):
        n = len(sel)
        eng._annotate_ws.fill_(POISON)
        got = eng.annotate(s["dflat"], s["dev"], s["meas"], s["cams"], sel, cameras=s["idx"], table=s["table"])
        assert got["shapes"] == [s["shapes"][b] for b in sel] and got["status"].cpu().tolist() == [s["status"][b] for b in sel]
        for k, pic in enumerate(_pictures(got["buf"], got["shapes"], got["byte_offsets"])):
            assert np.array_equal(pic, s["pics"][sel[k]]), (sel, k)
        assert n == len(got["byte_offsets"])
    # the out table of a selection seen before is the packed and uploaded one, also after other selections in between
    again = eng.annotate(s["dflat"], s["dev"], s["meas"], s["cams"], [3], cameras=s["idx"], table=s["table"])
    assert again["table"] is eng._out_tables[(((1080, 1920),), str(s["dflat"].device))] and len(eng._out_tables) <= 16
    assert eng.annotate(s["dflat"], s["dev"], s["meas"], s["cams"], [3], cameras=s["idx"], table=s["table"])["table"] is again["table"]
    with pytest.raises(ValueError):
        eng.annotate(s["dflat"], s["dev"], s["meas"], s["cams"], [B], cameras=s["idx"], table=s["table"])
    with pytest.raises(ValueError):
        eng.annotate(s["dflat"], s["dev"], s["meas"], s["cams"], [0], cameras=s["idx"], table=s["table"], native=True)


def test_status_per_frame_bad_camera_empty_frame_and_a_skipped_outline():
    need_gpu()
    import vti_amd
    s = _every()
    restated = _restated()
    bad = [b for b, (_, _, cam) in enumerate(s["plan"]) if cam == BAD]
    assert bad == [6] and restated[6][3] == A.BAD_CAMERA and restated[6][2] == []
    assert np.array_equal(s["pics"][6], s["frames"][6])                     # a plain copy
    # the empty frames: nothing but the ROI of their camera (camera 0 has none, camera 1's is clamped to the frame)
    assert s["plan"][2][0] == [] and s["plan"][12][0] == []
    assert restated[2][2] == [] and np.array_equal(s["pics"][2], s["frames"][2])
    (kind, p1, p2, colour, thick), = restated[12][2]
    assert kind == "rect" and colour == A.ROI_COLOUR and p2 == (332, 480) and not np.array_equal(s["pics"][12], s["frames"][12])
    # an outline beyond max_points: the middle frame is drawn without it, its neighbours of other sizes are untouched by that
    plain, comb, plain2 = U.jagged_scenes()
    t = _setup([(plain, (1080, 1920), 0), (comb, (960, 1280), 0), (plain2, (720, 960), 0)], dead=0, seed=7)
    eng = t["eng"]
    got = eng.annotate(t["dflat"], t["dev"], t["meas"], t["cams"], [0, 1, 2], cameras=t["idx"], table=t["table"], max_points=U.SMALL_MAX_POINTS)
    status = got["status"].cpu().tolist()
    assert status == [0, vti_amd._lib.VTI_ANNOTATE_OUTLINE_SKIPPED, 0]
    host = {k: t["meas"][k].cpu().numpy() for k in HOST_KEYS}
    xy = t["dev"]["xyxy"].cpu().numpy()
    for b, pic in enumerate(_pictures(got["buf"], got["shapes"], got["byte_offsets"])):
        cls, ms = t["ref"][b]
        h, w = t["shapes"][b]
        rows = U.device_rows(host, b, t["offsets"], t["cap"], len(cls))
        prims, word = A.display_list(h, w, cls, xy[b, :len(cls)], ms, rows, _params(0), max_points=U.SMALL_MAX_POINTS, with_status=True)
        assert rows["status"] == A.OK and word == status[b]
        assert any(q[0] == "polyline" and q[2] for q in prims) == (b != 1)
        assert np.array_equal(pic, A.rasterise(t["frames"][b], prims)), b


def test_every_size_is_drawn_on_and_both_tracers_draw_an_outline():
    need_gpu()
    s = _every()
    restated = _restated()
    drawn, outlined = set(), set()
    for b, (want, word, prims, st) in enumerate(restated):
        if not np.array_equal(s["pics"][b], s["frames"][b]):
            drawn.add(s["shapes"][b])
        if st == A.OK and any(q[0] == "polyline" and q[2] for q in prims):
            outlined.add(s["shapes"][b])
    print("drawn", sorted(drawn), "outlined", sorted(outlined))
    assert drawn == set(s["shapes"])
    assert (1080, 1920) in outlined and (960, 1280) in outlined            # the global-image tracer and the LDS tracer
