"""The refusals of the measure, annotate, overlay and JPEG-encode entry points, and of everything that packs, reads or predicts through
a frame table or a window table (vti_pack_frames / vti_pack_windows, the table readers, letterbox, scale_boxes, the ragged native
masks and the three table predicts), as data: for each entry point a valid baseline call built from fake pointers (never
dereferenced), and a list of single-fault overrides, one or more per argument check.  cases() yields (entry point, case name,
call); call() -> (status, message).  Every case is refused before the weights / workspace state check and before the first HIP
call, so nothing here launches anything; faults that only a launch could find stay out.  tests/golden/make_abi_refusals.py records
the answers of one commit's library in tests/golden/abi_refusals.json; test_abi_refusals.py replays the cases against the current
library and compares byte for byte.  Which fault wins when two are present is not part of the record: every case has exactly one."""
import ctypes as C
import dataclasses as dc

import torch

from test_oracle_geometry import load_calib

SHAPES = [(960, 1280), (481, 333), (720, 960), (1080, 1920)]
SEL = [3, 0, 3]
NAN = float("nan")


def _at(n):
    return C.c_void_p(4096 + n)


def _hp(t):
    return C.c_void_p(t.host.data_ptr())


def _i32(*v):
    return (C.c_int32 * len(v))(*v)


def _corrupt(t, row):
    """A copy of a host frame table whose row `row` has a byte offset that is no multiple of 16."""
    c = t.host.clone()
    c[64 + 64 * row] = 1
    return c


def _corrupt_window(t, row, what):
    """A copy of a host window table with one thing wrong in row `row` (a WindowRow: the crop's FrameRow, whose first field is the
    crop's byte offset, then frame_offset i64, H0, W0, x0, y0 i32), everything else kept consistent with it."""
    c = t.host.clone()
    i64, i32 = c[64 + 128 * row:][:128].view(torch.int64), c[64 + 128 * row:][:128].view(torch.int32)
    if what == "frame_offset":          # no multiple of 16; the crop moves with its frame
        i64[8] += 1
        i64[0] += 1
    elif what == "crop offset":         # not where the origin puts it
        i64[0] += 3
    elif what == "outside":             # one column past the frame's right edge; the crop moves with its origin
        (H0, W0), (x0, _, w, _) = t.shapes[row], t.windows[row]
        i32[20] = W0 - w + 1
        i64[0] += 3 * (W0 - w + 1 - x0)
    return c


def _settings_faults(p, measure):
    """The faults of one settings struct (vti_measure_params / vti_checker_params)."""
    f = [("equal class ids", dc.replace(p, fabric_id=0)), ("stitch_id -1", dc.replace(p, stitch_id=-1)),
         ("fabric_id -1", dc.replace(p, fabric_id=-1)), ("neighborhood -1", dc.replace(p, envelope_neighborhood=-1)),
         ("neighborhood 65", dc.replace(p, envelope_neighborhood=65)), ("min_stitches 0", dc.replace(p, min_stitches=0)),
         ("kmeans_iters -1", dc.replace(p, kmeans_iters=-1)), ("frame_buffer 0", dc.replace(p, frame_buffer=0)),
         ("NaN max_px_distance", dc.replace(p, max_px_distance=NAN))]
    if measure:
        f.append(("NaN two_row_threshold_px", dc.replace(p, two_row_threshold_px=NAN)))
    out = [(name, q.to_c()) for name, q in f]
    for flag in ("skip_cluster", "drop_empty"):        # the dataclasses hold booleans: the value 2 goes into the C struct
        c = p.to_c()
        setattr(c, flag, 2)
        out.append((flag + " 2", c))
    return out


def cases(vti_amd):
    L = vti_amd.lib()
    eng = vti_amd.Engine("n", 2, H=736, W=960, max_batch=4)
    wide_eng = vti_amd.Engine("n", 2, H=2176, W=3840, max_batch=1)       # (4 W + 2 H) * 4 bytes of resize tables: above 60 KiB
    other = vti_amd.Engine("n", 2, H=64, W=96, max_batch=4)
    ctx = eng._ctx
    calib = load_calib()
    mp_, cp_ = vti_amd.MeasureParams(*calib), vti_amd.CheckerParams(*calib)
    one, ws = C.c_void_p(4096), C.c_void_p(1 << 20)
    B, H0, W0, max_det, cap, n_sel, mp = 4, 960, 1280, 200, 800, 3, 4096
    keep = [eng, wide_eng, other]                                       # what the fake calls point into stays alive with the closures

    def entry(name, order, base, faults, message=True):
        fn = getattr(L, name)
        for case, over in faults:
            a = dict(base, **over)

            def call(a=a, keep=keep):
                rc = fn(*[a[k] for k in order])
                return int(rc), (L.vti_last_error(a["ctx"]) or b"").decode() if message else ""
            yield name, case, call

    def nulls(names):
        return [("null " + n, {n: None}) for n in names]

    def table_faults(ht, dt, B_name, t, B_, other_kind=None):
        """The faults the table check finds in the table pair (ht, dt) of B_ rows; t: the FrameTable or WindowTable of the baseline.
        other_kind: the same frames' table of the other kind, which the call must refuse as it refuses junk."""
        windows = isinstance(t, vti_amd.WindowTable)
        oc = other.pack_windows(t.shapes, t.windows, device="cpu") if windows else other.pack_frames(t.shapes, device="cpu")[0]
        row, junk = min(1, B_ - 1), (C.c_uint8 * 256)()
        bad = _corrupt_window(t, row, "frame_offset") if windows else _corrupt(t, row)
        keep.extend([oc, bad, junk])
        faults = [(f"null {ht}", {ht: None}), (f"null {dt}", {dt: None}), (f"{dt} misaligned", {dt: _at(8)}),
                  (f"{ht} junk", {ht: C.cast(junk, C.c_void_p)}), (f"{ht} other canvas", {ht: _hp(oc)}),
                  (f"{ht} corrupt row", {ht: C.c_void_p(bad.data_ptr())})]
        if windows:
            crop, outside = _corrupt_window(t, row, "crop offset"), _corrupt_window(t, row, "outside")
            keep.extend([crop, outside])
            faults += [(f"{ht} crop offset off its origin", {ht: C.c_void_p(crop.data_ptr())}),
                       (f"{ht} window outside its frame", {ht: C.c_void_p(outside.data_ptr())})]
        if other_kind is not None:
            keep.append(other_kind)
            faults.append((f"{ht} of the other kind", {ht: _hp(other_kind)}))
        return faults + ([(f"{B_name} + 1", {B_name: B_ + 1}), (f"{B_name} 0", {B_name: 0})] if B_name else [])

    t_in, _, _ = eng.pack_frames(SHAPES, device="cpu")
    t_out, _, _ = eng.pack_frames([SHAPES[b] for b in SEL], device="cpu")
    wide = [(960, 1280), (480, 8200), (720, 960), (1080, 1920)]
    t_wide, _, _ = eng.pack_frames(wide, device="cpu")
    t_wide_out, _, _ = eng.pack_frames([wide[b] for b in (3, 1, 3)], device="cpu")
    keep.extend([t_in, t_out, t_wide, t_wide_out])

    # ---- the measurement family ---------------------------------------------------------------------------------------------
    m_in = ["masks", "native", "dets", "xyxy", "counts", "offsets"]
    m_out = ["scratch", "nbytes", "ff", "fi", "sf", "si", "stream"]
    m_need = L.vti_measure_scratch_bytes(ctx, B, cap, W0)
    m_need_frames = L.vti_measure_scratch_bytes(ctx, B, cap, 1920)
    m_base = dict(ctx=ctx, masks=one, native=0, dets=one, xyxy=one, counts=one, offsets=one, B=B, max_det=max_det, cap=cap, H0=H0, W0=W0,
                  scratch=ws, nbytes=m_need, ff=one, fi=one, sf=one, si=one, stream=None)
    m_ptr_faults = nulls(["masks", "dets", "xyxy", "counts", "offsets", "ff", "fi", "scratch"]) + [
        ("max_det 0", dict(max_det=0)), ("max_det 1001", dict(max_det=1001)), ("cap -1", dict(cap=-1)),
        ("native 2", dict(native=2)), ("native -1", dict(native=-1)),
        ("masks misaligned", dict(masks=_at(8))), ("scratch misaligned", dict(scratch=C.c_void_p((1 << 20) + 64))),
        ("scratch one byte short", dict(nbytes=m_need - 1))]
    m_size_faults = [("B -1", dict(B=-1)), ("H0 0", dict(H0=0)), ("W0 0", dict(W0=0)), ("native masks misaligned", dict(native=1, masks=_at(4))),
                     ("canvas too large", dict(ctx=wide_eng._ctx)), ("B * W0", dict(B=1 << 20, W0=4096, nbytes=1 << 60))]
    shape = ["B", "max_det", "cap", "H0", "W0"]
    for name, params, faults in (("vti_measure", mp_, _settings_faults(mp_, True)), ("vti_measure_checker", cp_, _settings_faults(cp_, False))):
        yield from entry(name, ["ctx", "params"] + m_in + shape + m_out, dict(m_base, params=C.byref(params.to_c())),
                         [("null ctx", dict(ctx=None)), ("null params", dict(params=None))] + m_ptr_faults + m_size_faults +
                         [(case, dict(params=C.byref(c))) for case, c in faults])

    cam_head = ["ctx", "cameras", "n_cams", "cams"]
    cam_base = dict(m_base, cameras=one, n_cams=2, cams=one)
    cam_faults = [("null ctx", dict(ctx=None)), ("null cameras", dict(cameras=None)), ("null cams", dict(cams=None)), ("n_cams 0", dict(n_cams=0)),
                  ("cameras misaligned", dict(cameras=_at(8))), ("cams misaligned", dict(cams=_at(2)))]
    fr_base = dict(cam_base, ht=_hp(t_in), dt=one, nbytes=m_need_frames)
    fr_short = [(c, dict(o, nbytes=m_need_frames - 1) if c == "scratch one byte short" else o) for c, o in m_ptr_faults]
    cam_bytes = L.vti_measure_cameras_bytes(2)
    cam_table = (C.c_uint8 * cam_bytes)()

    def rig(stem, pack, array, p, measure):
        """The camera-table and frame-table forms of vti_measure (stem) or vti_measure_checker, and the family's pack call."""
        yield from entry(stem + "_cameras", cam_head + m_in + shape + m_out, cam_base, cam_faults + m_ptr_faults + m_size_faults)
        yield from entry(stem + "_frames", cam_head + m_in + ["ht", "dt", "B", "max_det", "cap"] + m_out, fr_base,
                         cam_faults + table_faults("ht", "dt", "B", t_in, B) + fr_short + [("native 1", dict(native=1))])
        yield from entry(stem + "_frames_native",
                         cam_head + ["masks", "bases", "cbytes"] + m_in[2:] + ["ht", "dt", "B", "max_det", "cap"] + m_out,
                         dict(fr_base, bases=one, cbytes=1 << 20),
                         cam_faults + table_faults("ht", "dt", "B", t_in, B) + [(c, o) for c, o in fr_short if "native" not in c and c != "masks misaligned"] +
                         [("null bases", dict(bases=None)), ("cbytes -1", dict(cbytes=-1)), ("bases misaligned", dict(bases=_at(4))),
                          ("masks misaligned", dict(masks=_at(4)))])
        pack_faults = [("null params", dict(params=None)), ("n_cams 0", dict(n_cams=0)), ("null table", dict(table=None)),
                       ("table one byte short", dict(nbytes=cam_bytes - 1))]
        for case, c in _settings_faults(p, measure):
            pack_faults.append(("camera 1: " + case, dict(params=array(p.to_c(), c))))
        yield from entry(pack, ["ctx", "params", "n_cams", "table", "nbytes"],
                         dict(ctx=ctx, params=array(p.to_c(), p.to_c()), n_cams=2, table=cam_table, nbytes=cam_bytes), pack_faults)

    yield from rig("vti_measure", "vti_measure_pack_cameras", vti_amd._lib.VtiMeasureParams * 2, mp_, True)
    yield from rig("vti_measure_checker", "vti_checker_pack_cameras", vti_amd._lib.VtiCheckerParams * 2, cp_, False)

    # ---- the drawing calls of one frame size -----------------------------------------------------------------------------------
    d_in = ["masks", "native", "dets", "xyxy", "counts", "offsets", "max_det", "cap"]
    d_meas = ["fi", "sf", "si"]
    d_sel = ["hsel", "dsel", "n_sel"]
    d_out = ["out", "status", "scratch", "nbytes", "stream"]
    a_need = L.vti_annotate_scratch_bytes(ctx, n_sel, max_det, H0, W0, mp)
    d_base = dict(ctx=ctx, frames=one, B=B, H0=H0, W0=W0, masks=one, native=0, dets=one, xyxy=one, counts=one, offsets=one, max_det=max_det,
                  cap=cap, fi=one, sf=one, si=one, hsel=_i32(*SEL), dsel=one, n_sel=n_sel, mp=mp, out=one, status=one, scratch=ws,
                  nbytes=a_need, stream=None)
    d_ptrs = ["frames", "masks", "dets", "xyxy", "counts", "offsets", "hsel", "dsel", "out", "status", "scratch"]
    d_faults = [("null ctx", dict(ctx=None)), ("n_sel 0", dict(n_sel=0)), ("n_sel -2", dict(n_sel=-2)),
                ("hsel[1] -1", dict(hsel=_i32(0, -1, 1))), ("hsel[2] B", dict(hsel=_i32(0, 1, B))),
                ("max_det 1001", dict(max_det=1001)), ("max_det 0", dict(max_det=0)), ("H0 8193", dict(H0=8193, nbytes=1 << 40)),
                ("W0 8193", dict(W0=8193, nbytes=1 << 40)), ("H0 0", dict(H0=0)), ("W0 0", dict(W0=0)), ("B 0", dict(B=0)),
                ("cap -1", dict(cap=-1)), ("mp -1", dict(mp=-1)), ("native 2", dict(native=2)), ("native -1", dict(native=-1)),
                ("2^40 bytes of pictures", dict(n_sel=6000, H0=8192, W0=8192, nbytes=1 << 60)),
                ("scratch one byte short", dict(nbytes=a_need - 1)), ("scratch misaligned", dict(scratch=C.c_void_p((1 << 20) + 64))),
                ("masks misaligned", dict(masks=_at(8))), ("native masks misaligned", dict(native=1, masks=_at(4))),
                ("dsel misaligned", dict(dsel=_at(2)))]
    meas_faults = nulls(d_meas) + [("sf misaligned", dict(sf=_at(4))), ("si misaligned", dict(si=_at(2))), ("fi misaligned", dict(fi=_at(2))),
                                   ("status misaligned", dict(status=_at(2)))]
    yield from entry("vti_annotate", ["ctx", "frames", "B", "H0", "W0", "cameras", "n_cams", "cams"] + d_in + d_meas + d_sel + ["mp"] + d_out,
                     dict(d_base, cameras=one, n_cams=2, cams=one),
                     d_faults + nulls(d_ptrs + ["cameras"]) + meas_faults +
                     [("n_cams 0", dict(n_cams=0)), ("cameras misaligned", dict(cameras=_at(8))), ("cams misaligned", dict(cams=_at(2)))])
    yield from entry("vti_annotate_checker", ["ctx", "frames", "B", "H0", "W0", "params"] + d_in + d_meas + d_sel + ["mp"] + d_out,
                     dict(d_base, params=C.byref(cp_.to_c())),
                     d_faults + nulls(d_ptrs + ["params"]) + meas_faults + [("canvas too large", dict(ctx=wide_eng._ctx))] +
                     [(case, dict(params=C.byref(c))) for case, c in _settings_faults(cp_, False)])

    yield from entry("vti_annotate_checker_cameras",
                     ["ctx", "frames", "B", "H0", "W0", "cameras", "n_cams", "cams"] + d_in + d_meas + d_sel + ["mp"] + d_out,
                     dict(d_base, cameras=one, n_cams=2, cams=one),
                     d_faults + nulls(d_ptrs + ["cameras"]) + meas_faults + [("canvas too large", dict(ctx=wide_eng._ctx))] +
                     [("n_cams 0", dict(n_cams=0)), ("cameras misaligned", dict(cameras=_at(8))), ("cams misaligned", dict(cams=_at(2)))])

    o_need = L.vti_overlay_scratch_bytes(ctx, n_sel, max_det, H0, W0, mp)
    o_mid = ["plates", "pal", "nc", "alpha", "beta"]
    o_base = dict(d_base, plates=one, pal=(C.c_uint8 * 18)(*range(18)), nc=6, alpha=0.3, beta=0.7, mode=3, ann=None, nbytes=o_need)
    o_faults = [("mode 0", dict(mode=0)), ("mode 4", dict(mode=4)), ("mode -1", dict(mode=-1)), ("nc 0", dict(nc=0)), ("nc 17", dict(nc=17)),
                ("alpha NaN", dict(alpha=NAN)), ("beta inf", dict(beta=float("inf"))), ("blend without a picture", dict(mode=2)),
                ("draw with a picture", dict(mode=1, ann=one)), ("both with a picture", dict(mode=3, ann=one)),
                ("plates misaligned", dict(plates=_at(8)))] + \
               [(n + " misaligned", {n: _at(2)}) for n in ("counts", "offsets", "status", "dets", "xyxy")]
    yield from entry("vti_overlay", ["ctx", "frames", "B", "H0", "W0"] + d_in + o_mid + d_sel + ["mode", "ann", "mp"] + d_out, o_base,
                     [(c, dict(o, nbytes=o_need - 1) if c == "scratch one byte short" else o) for c, o in d_faults] +
                     nulls(d_ptrs + ["pal"]) + o_faults)

    # ---- the drawing calls for frames of differing sizes ---------------------------------------------------------------------
    f_faults = [(c, o) for c, o in d_faults if not any(k in o for k in ("H0", "W0", "B"))] + \
               table_faults("ht", "dt", "B", t_in, B) + table_faults("hot", "dot", None, t_out, n_sel) + [
        ("out row 1 of another size", dict(hsel=_i32(3, 1, 3))), ("out table of 4 rows", dict(hot=_hp(t_in))),
        ("n_sel 2 with an out table of 3", dict(n_sel=2, hsel=_i32(3, 0))),
        ("a selected frame of 8200 columns", dict(ht=_hp(t_wide), hot=_hp(t_wide_out), hsel=_i32(3, 1, 3), nbytes=1 << 40)),
        ("frames misaligned", dict(frames=_at(8))), ("out misaligned", dict(out=_at(8)))]
    # the walk over the selection compares row k of the out table on its way: the bad index goes where the rows before it agree
    f_faults = [(c, dict(hsel=_i32(3, -1, 3)) if c == "hsel[1] -1" else dict(hsel=_i32(3, 0, B)) if c == "hsel[2] B" else o)
                for c, o in f_faults if c != "native masks misaligned"]
    # 5462 pictures of 8192 x 8192 are more than 2^40 bytes: each frame passes, the selection as a whole does not
    t_one, _, _ = eng.pack_frames([(8192, 8192)], device="cpu")
    t_many, _, _ = eng.pack_frames([(8192, 8192)] * 5462, device="cpu")
    keep.extend([t_one, t_many])
    f_faults.append(("2^40 bytes of pictures", dict(ht=_hp(t_one), B=1, hot=_hp(t_many), n_sel=5462, hsel=_i32(*[0] * 5462), nbytes=1 << 60)))
    af_need = L.vti_annotate_frames_scratch_bytes(ctx, _hp(t_out), max_det, mp)
    f_base = dict(ht=_hp(t_in), dt=one, hot=_hp(t_out), dot=one)
    short = lambda faults, need: [(c, dict(o, nbytes=need - 1) if c == "scratch one byte short" else o) for c, o in faults]
    for name in ("vti_annotate_frames", "vti_annotate_checker_frames"):
        yield from entry(name, ["ctx", "frames", "ht", "dt", "B", "cameras", "n_cams", "cams"] + d_in + d_meas + d_sel +
                         ["mp", "hot", "dot"] + d_out, dict(d_base, cameras=one, n_cams=2, cams=one, nbytes=af_need, **f_base),
                         short(f_faults, af_need) + nulls(d_ptrs + ["cameras"]) + meas_faults +
                         [("native 1", dict(native=1)), ("n_cams 0", dict(n_cams=0)), ("cameras misaligned", dict(cameras=_at(8))),
                          ("cams misaligned", dict(cams=_at(2)))])
    of_need = L.vti_overlay_frames_scratch_bytes(ctx, _hp(t_out), max_det, mp)
    yield from entry("vti_overlay_frames", ["ctx", "frames", "ht", "dt", "B", "masks", "native", "bases", "cbytes"] + d_in[2:] + o_mid + d_sel +
                     ["mode", "ann", "mp", "hot", "dot"] + d_out, dict(o_base, bases=None, cbytes=0, nbytes=of_need, **f_base),
                     short(f_faults, of_need) + nulls(d_ptrs + ["pal"]) + o_faults +
                     [("bases with letterbox masks", dict(bases=one)), ("native without bases", dict(native=1)),
                      ("cbytes -1", dict(cbytes=-1)), ("bases misaligned", dict(native=1, bases=_at(4), cbytes=1 << 20)),
                      ("native masks misaligned", dict(native=1, bases=one, cbytes=1 << 20, masks=_at(4))),
                      ("ann misaligned", dict(mode=2, ann=_at(8)))])

    big, _, _ = eng.pack_frames([(8200, 480)], device="cpu")
    junk = (C.c_uint8 * 256)()
    keep.extend([big, junk])
    for name in ("vti_annotate_frames_scratch_bytes", "vti_overlay_frames_scratch_bytes"):     # refusal here is the answer 0
        yield from entry(name, ["ctx", "hot", "max_det", "mp"], dict(ctx=ctx, hot=_hp(t_out), max_det=max_det, mp=mp),
                         [("null ctx", dict(ctx=None)), ("null table", dict(hot=None)), ("junk table", dict(hot=C.cast(junk, C.c_void_p))),
                          ("max_det 0", dict(max_det=0)), ("max_det 1001", dict(max_det=1001)), ("mp -1", dict(mp=-1)),
                          ("a frame of 8200 rows", dict(hot=_hp(big)))], message=False)

    # ---- the JPEG encoder -------------------------------------------------------------------------------------------------------
    j_need = L.vti_encode_jpeg_scratch_bytes(ctx, 3, H0, W0)
    j_tail = ["rgb", "quality", "scratch", "nbytes", "offsets", "out", "max_bytes", "stream"]
    j_base = dict(ctx=ctx, frames=one, n=3, H0=H0, W0=W0, rgb=0, quality=95, scratch=ws, nbytes=j_need, offsets=one, out=one,
                  max_bytes=1 << 20, stream=None)
    j_faults = [("null ctx", dict(ctx=None)), ("quality 0", dict(quality=0)), ("quality 101", dict(quality=101)), ("rgb 2", dict(rgb=2)),
                ("max_bytes -1", dict(max_bytes=-1)), ("offsets misaligned", dict(offsets=_at(4))),
                ("scratch misaligned", dict(scratch=C.c_void_p((1 << 20) + 64)))] + nulls(["frames", "offsets", "out", "scratch"])
    yield from entry("vti_encode_jpeg", ["ctx", "frames", "n", "H0", "W0"] + j_tail, j_base,
                     j_faults + [("n 0", dict(n=0)), ("H0 8193", dict(H0=8193)), ("W0 0", dict(W0=0)),
                                 ("scratch one byte short", dict(nbytes=j_need - 1)),
                                 ("more than 2^28 MCUs", dict(n=1025, H0=8192, W0=8192, nbytes=1 << 60))])
    jf_need = L.vti_encode_jpeg_frames_scratch_bytes(ctx, _hp(t_out))
    yield from entry("vti_encode_jpeg_frames", ["ctx", "frames", "ht", "dt", "n"] + j_tail,
                     dict(j_base, ht=_hp(t_out), dt=one, nbytes=jf_need),
                     j_faults + table_faults("ht", "dt", "n", t_out, 3) +
                     [("a frame of 8200 columns", dict(ht=_hp(t_wide_out), nbytes=1 << 40)), ("scratch one byte short", dict(nbytes=jf_need - 1))])

    # ---- the readers of frame-table rows -----------------------------------------------------------------------------------------
    i32, f64 = (C.c_int32 * 8)(), (C.c_double * 5)()
    yield from entry("vti_frame_table_info", ["ht", "b", "i32", "f64"], dict(ctx=None, ht=_hp(t_in), b=1, i32=i32, f64=f64),
                     [("null table", dict(ht=None)), ("null out", dict(i32=None)), ("b -2", dict(b=-2)), ("b B", dict(b=4)),
                      ("junk table", dict(ht=C.cast(junk, C.c_void_p)))], message=False)
    raw_shapes = [(960, 1280), (480, 332), (720, 960)]
    rt = eng.pack_raw_frames(raw_shapes, 0, device="cpu")
    rt4 = eng.pack_raw_frames(SHAPES[:1] + raw_shapes, 0, device="cpu")
    ft, _, _ = eng.pack_frames(raw_shapes, device="cpu")
    keep.extend([rt, rt4, ft])
    yield from entry("vti_convert_raw_frames", ["ctx", "raw", "raw_bytes", "hrt", "drt", "ht", "dt", "n", "rgb", "out", "out_bytes", "stream"],
                     dict(ctx=ctx, raw=one, raw_bytes=rt.raw_bytes, hrt=_hp(rt), drt=one, ht=_hp(ft), dt=one, n=3, rgb=0, out=one,
                          out_bytes=ft.total_bytes, stream=None),
                     [("null ctx", dict(ctx=None)), ("rgb 2", dict(rgb=2)), ("drt misaligned", dict(drt=_at(8))),
                      ("raw table of 4 rows", dict(hrt=_hp(rt4))), ("raw_bytes short", dict(raw_bytes=rt.raw_bytes - 1)),
                      ("out_bytes short", dict(out_bytes=ft.total_bytes - 1)), ("a frame of another size", dict(ht=_hp(t_out), out_bytes=1 << 40))] +
                     nulls(["raw", "hrt", "drt", "out"]) + table_faults("ht", "dt", None, ft, 3))

    # ---- the two other users of the shared scratch check ------------------------------------------------------------------------
    small = vti_amd.Engine("n", 2, H=64, W=64, max_batch=1)
    keep.append(small)
    p_need = small.mask_polygons_scratch_bytes(48, 64, 8)
    yield from entry("vti_mask_polygons", ["ctx", "masks", "n", "live", "H", "W", "rb", "H0", "W0", "strategy", "scratch", "nbytes", "offsets",
                                           "points", "max_points", "stream"],
                     dict(ctx=small._ctx, masks=one, n=3, live=None, H=48, W=64, rb=8, H0=60, W0=80, strategy=0, scratch=ws, nbytes=p_need,
                          offsets=one, points=one, max_points=100, stream=None),
                     [("null scratch", dict(scratch=None)), ("scratch misaligned", dict(scratch=C.c_void_p((1 << 20) + 64))),
                      ("scratch one byte short", dict(nbytes=p_need - 1))])
    import jpeg_decode_util as U
    import jpeg_util as J
    files = [U.own_file(J.frame("ramp", 17, 33), 95, "420"), U.own_file(J.frame("noise", 50, 70), 95, "444", restart=3)]
    rc, plan = U.plan(vti_amd, files)
    assert rc == 0
    keep.append(plan)
    yield from entry("vti_decode_jpeg", ["ctx", "files", "host", "dev", "n", "rgb", "out", "out_bytes", "info", "scratch", "nbytes", "stream"],
                     dict(ctx=small._ctx, files=_at(1), host=plan["table"].ctypes.data, dev=C.c_void_p(1 << 21), n=2, rgb=1, out=_at(1),
                          out_bytes=int(plan["out_off"][-1]), info=C.c_void_p(1 << 22), scratch=ws, nbytes=plan["scratch_bytes"], stream=None),
                     [("null scratch", dict(scratch=None)), ("scratch misaligned", dict(scratch=C.c_void_p((1 << 20) + 64))),
                      ("scratch one byte short", dict(nbytes=plan["scratch_bytes"] - 1))])

    # ---- frame tables and window tables: packing, reading, letterbox, boxes, ragged masks, predict --------------------------------
    # No "null ctx" cases: the table check answers a null ctx without a message, and vti_last_error(NULL) then returns whatever an
    # earlier null-ctx call left.  No case for "a frame of host_table has no native mask layout" either: a row that passes the table
    # check (sides in 1..16384, a canvas of multiples of 32) always has a bit-packed layout (slots of at most 32 MiB).
    WIN = [(100, 50, 640, 480), (3, 7, 300, 400), (0, 0, 960, 720), (640, 300, 1000, 700)]           # (x0, y0, w, h) per frame of SHAPES
    eng8 = vti_amd.Engine("n", 2, H=736, W=960, max_batch=8)           # the same canvas: packs window tables of more rows than eng takes
    w_in = eng.pack_windows(SHAPES, WIN, device="cpu")
    five = SHAPES + [(600, 800)]
    t5, _, _ = eng.pack_frames(five, device="cpu")
    w5 = eng8.pack_windows(five, WIN + [(0, 0, 800, 600)], device="cpu")
    keep.extend([eng8, w_in, t5, w5])
    kinds = [("frames", t_in, w_in, t5), ("windows", w_in, t_in, w5)]                                # suffix, table, other kind, 5 rows

    def arr(ctype, v):
        return (ctype * len(v))(*v)

    offs, total = t_in.byte_offsets, t_in.total_bytes
    p_order = ["ctx", "H", "W", "H0s", "W0s", "offs", "B", "total", "table", "nbytes"]
    pw_order = p_order[:6] + ["wins"] + p_order[6:]
    heights, widths = [h for h, _ in SHAPES], [w for _, w in SHAPES]
    flat = lambda wins: _i32(*[v for w in wins for v in w])
    for name, order, table_bytes in (("vti_pack_frames", p_order, L.vti_frame_table_bytes), ("vti_pack_windows", pw_order, L.vti_window_table_bytes)):
        nb = int(table_bytes(B))
        out = (C.c_uint8 * int(table_bytes(8)))()
        p_base = dict(ctx=ctx, H=736, W=960, H0s=_i32(*heights), W0s=_i32(*widths), offs=arr(C.c_int64, offs), wins=flat(WIN), B=B,
                      total=total, table=out, nbytes=nb)
        frame1 = lambda h, w, off=offs[1]: dict(H0s=_i32(heights[0], h, *heights[2:]), W0s=_i32(widths[0], w, *widths[2:]),
                                                offs=arr(C.c_int64, [offs[0], off] + offs[2:]))
        p_faults = nulls(["H0s", "W0s", "offs", "table"]) + [
            ("B 0", dict(B=0)), ("H 0", dict(H=0)), ("H 740", dict(H=740)), ("W 950", dict(W=950)), ("total_bytes -1", dict(total=-1)),
            ("table one byte short", dict(nbytes=nb - 1)), ("frame 1: H0 0", frame1(0, 333)), ("frame 1: W0 16385", frame1(481, 16385)),
            ("frame 1: offset + 8", frame1(481, 333, offs[1] + 8)), ("frame 3 past total_bytes", dict(total=total - 16)),
            ("frame 1: resized below 1 px", dict(frame1(1, 16384), wins=flat([WIN[0], (0, 0, 16384, 1)] + WIN[2:])))]
        if name == "vti_pack_windows":
            big = dict(H0s=_i32(16384), W0s=_i32(16384), offs=arr(C.c_int64, [0]), B=1, total=3 * 16384 * 16384, nbytes=int(table_bytes(1)))
            p_faults += nulls(["wins"]) + [
                ("B above max_batch", dict(H0s=_i32(*heights, 600), W0s=_i32(*widths, 800), offs=arr(C.c_int64, t5.byte_offsets),
                                           wins=flat(WIN + [(0, 0, 800, 600)]), B=5, total=t5.total_bytes, nbytes=int(table_bytes(5)))),
                ("window 1: w 0", dict(wins=flat([WIN[0], (3, 7, 0, 400)] + WIN[2:]))),
                ("window 1: h -1", dict(wins=flat([WIN[0], (3, 7, 300, -1)] + WIN[2:]))),
                ("window 1: x0 -1", dict(wins=flat([WIN[0], (-1, 7, 300, 400)] + WIN[2:]))),
                ("window 1: one column past the right edge", dict(wins=flat([WIN[0], (34, 7, 300, 400)] + WIN[2:]))),
                ("window 1: one row past the bottom edge", dict(wins=flat([WIN[0], (3, 82, 300, 400)] + WIN[2:]))),
                ("window resized below 1 px", dict(big, wins=_i32(0, 0, 16384, 1)))]
        yield from entry(name, order, p_base, p_faults)

    yield from entry("vti_window_table_info", ["ht", "b", "i32", "f64"], dict(ctx=None, ht=_hp(w_in), b=1, i32=(C.c_int32 * 12)(), f64=f64),
                     [("null table", dict(ht=None)), ("null out", dict(i32=None)), ("b -2", dict(b=-2)), ("b B", dict(b=4)),
                      ("junk table", dict(ht=C.cast(junk, C.c_void_p))), ("a frame table", dict(ht=_hp(t_in)))], message=False)

    above = lambda rows5: ("B above max_batch", dict(ht=_hp(rows5), B=5))
    n_base = dict(ctx=ctx, dets=one, xyxy=one, counts=one, proto=one, ht=None, dt=one, B=B, max_det=max_det, mode=0, packing=1, masks=one,
                  cbytes=1 << 20, offsets=one, bases=one, stream=None)
    n_faults = nulls(["dets", "counts", "proto", "offsets", "bases"]) + [
        ("max_det 0", dict(max_det=0)), ("cbytes -1", dict(cbytes=-1)), ("cbytes 16 with null masks", dict(cbytes=16, masks=None)),
        ("packing u8", dict(packing=0)), ("packing 2", dict(packing=2)), ("masks misaligned", dict(masks=_at(4))),
        ("bases misaligned", dict(bases=_at(4))), ("offsets misaligned", dict(offsets=_at(2))), ("B * max_det", dict(max_det=1 << 30))]
    pr_head = ["ctx", "frames", "ht", "dt", "B", "swap_rb", "conf", "iou", "max_det", "agnostic", "mode", "packing", "input", "pred", "proto",
               "dets", "counts", "masks"]
    pr_base = dict(n_base, frames=one, swap_rb=1, conf=0.25, iou=0.7, agnostic=0, input=one, pred=one, cap=cap)
    head_faults = nulls(["frames", "input"]) + [("frames misaligned", dict(frames=_at(8))), ("input misaligned", dict(input=_at(2))),
                                                ("xyxy misaligned", dict(xyxy=_at(8)))]
    for kind, t, twin, rows5 in kinds:
        tf = table_faults("ht", "dt", "B", t, B, other_kind=twin)
        base = dict(n_base, ht=_hp(t))
        yield from entry("vti_letterbox_" + kind, ["ctx", "frames", "ht", "dt", "B", "out", "stream"], dict(base, frames=one, out=one),
                         tf + nulls(["frames", "out"]) + [("frames misaligned", dict(frames=_at(8))), ("out misaligned", dict(out=_at(2))),
                                                          above(rows5)])
        yield from entry("vti_scale_boxes_" + kind, ["ctx", "dets", "counts", "ht", "dt", "B", "max_det", "xyxy", "stream"], base,
                         tf + nulls(["dets", "counts", "xyxy"]) + [("max_det 0", dict(max_det=0)), ("xyxy misaligned", dict(xyxy=_at(8))),
                                                                   ("B * max_det", dict(max_det=1 << 30))])
        yield from entry(f"vti_mask_native_{kind}_bytes", ["ctx", "ht", "max_det"], base,
                         [("null ctx", dict(ctx=None)), ("null table", dict(ht=None)), ("max_det 0", dict(max_det=0)),
                          ("junk table", dict(ht=C.cast(junk, C.c_void_p))), ("a table of the other kind", dict(ht=_hp(twin))),
                          ("a table of another canvas", dict(ctx=other._ctx)), ("a table of 5 rows", dict(ht=_hp(rows5)))] +
                         [(c, o) for c, o in tf if c in ("ht corrupt row", "ht crop offset off its origin", "ht window outside its frame")],
                         message=False)
        # the ragged masks: vti_masks_native_frames takes the frame-px boxes, vti_masks_native_windows needs 8-byte aligned dets instead
        own = [("null xyxy", dict(xyxy=None))] if kind == "frames" else [("dets misaligned", dict(dets=_at(4)))]
        n_order = ["ctx", "dets"] + (["xyxy"] if kind == "frames" else []) + ["counts", "proto", "ht", "dt", "B", "max_det", "mode", "packing",
                                                                              "masks", "cbytes", "offsets", "bases", "stream"]
        yield from entry("vti_masks_native_" + kind, n_order, base, tf + n_faults + own + [("mode 2", dict(mode=2)), above(rows5)])
        # the native predicts: null xyxy and null pred have checks of their own, ahead of the ragged-mask checks and the head's
        name = "vti_predict_frames_native" if kind == "frames" else "vti_predict_windows"
        yield from entry(name, pr_head + ["cbytes", "offsets", "bases", "xyxy", "stream"], dict(pr_base, ht=_hp(t)),
                         tf + n_faults + ([] if kind == "frames" else own) + head_faults +
                         [("null xyxy", dict(xyxy=None)), ("null pred", dict(pred=None)), ("mode 2", dict(mode=2)),
                          ("mode native | 2", dict(mode=0x12)), above(rows5)])
    # vti_predict_frames: canvas-size masks; its own checks end at the head's (dets, counts and max_det only with dev_xyxy)
    yield from entry("vti_predict_frames", pr_head + ["cap", "offsets", "xyxy", "stream"], dict(pr_base, ht=_hp(t_in)),
                     table_faults("ht", "dt", "B", t_in, B, other_kind=w_in) + head_faults + nulls(["dets", "counts"]) +
                     [("max_det 0", dict(max_det=0)), ("mode native", dict(mode=0x10)), above(t5)])
