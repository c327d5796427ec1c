"""vti_annotate_frames_native / vti_annotate_checker_frames_native without a GPU: the marker, the declarations, the exports and the
ctypes signatures agree; every refusal comes before the first HIP call (fake pointers, never dereferenced; without a GPU a call that
reaches HIP ends with the HIP status instead); Engine.annotate / annotate_checker(table=, native=True) tell a ragged set from a plain
one before a device is touched; process_frames takes annotate_native by keyword only and keeps today's refusals without it.  The
GPU parity tests are in test_gpu_annotate_frames_native.py."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from test_oracle_geometry import load_calib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vti_annotate_frames_native", "vti_annotate_checker_frames_native")
SHAPES = [(960, 1280), (481, 333), (720, 960), (1080, 1920)]
ARG, UNSUPPORTED = -1, -6


def _hp(t):
    return C.c_void_p(t.host.data_ptr())


def test_marker_declarations_exports_and_signatures_agree(lib_built):
    vti_amd = lib_built
    hdr = open(os.path.join(ROOT, "include", "vti.h")).read()
    assert len(re.findall(r"^#define VTI_ANNOTATE_NATIVE_API\s*$", hdr, re.M)) == 1
    marked = re.findall(r"^VTI_ANNOTATE_NATIVE_API\s+int32_t\s+(vti_[a-z0-9_]+)\s*\(", hdr, re.M)
    assert tuple(marked) == NAMES
    exported = subprocess.run(["nm", "-D", "--defined-only", vti_amd.LIB_PATH], check=True, capture_output=True, text=True).stdout
    I32, I64, P, SZ = C.c_int32, C.c_int64, C.c_void_p, C.c_size_t
    for name, old in zip(NAMES, ("vti_annotate_frames", "vti_annotate_checker_frames")):
        assert re.search(r"\bT %s$" % name, exported, re.M), name
        res, args = vti_amd.SIGNATURES[name]
        ores, oargs = vti_amd.SIGNATURES[old]
        # the letterbox form's arguments with `native` (the tenth) replaced by dev_mask_bases, capacity_bytes
        assert oargs[9] is I32 and res is ores is I32
        assert list(args) == list(oargs[:9]) + [P, I64] + list(oargs[10:]) and args[-2] is SZ
        decl = hdr[hdr.index("int32_t %s(" % name):]
        decl = decl[:decl.index(";")]
        assert "native," not in decl and "int32_t native" not in decl
        assert re.search(r"const uint8_t\* dev_masks,\s*const int64_t\* dev_mask_bases,\s*int64_t capacity_bytes,", decl)
        assert len(decl.split(",")) == len(args)
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "`VTI_ANNOTATE_NATIVE_API`" in readme and all("`%s`" % n in readme for n in NAMES)
    assert "Still missing: pictures from frame-resolution masks" not in readme


@pytest.mark.parametrize("name", NAMES)
def test_every_refusal_comes_before_any_hip_call(lib_built, name):
    vti_amd = lib_built
    L = vti_amd.lib()
    fn = getattr(L, name)
    eng = vti_amd.Engine("n", 2, H=736, W=960, max_batch=4)
    B, max_det, cap, mp = 4, 200, 800, 4096
    sel = [3, 0, 3]
    t_in, _, _ = eng.pack_frames(SHAPES, device="cpu")
    t_out, _, _ = eng.pack_frames([SHAPES[b] for b in sel], device="cpu")
    need = L.vti_annotate_frames_scratch_bytes(eng._ctx, _hp(t_out), max_det, mp)
    assert need > 0
    one, ws = C.c_void_p(4096), C.c_void_p(1 << 20)                # never dereferenced
    good_sel = (C.c_int32 * 3)(*sel)
    err = lambda ctx=eng._ctx: L.vti_last_error(ctx)

    def call(ctx=eng._ctx, frames=one, ht=_hp(t_in), dt=one, B=B, cams=one, n_cams=2, cof=one, masks=one, bases=one, cb=1 << 20,
             dets=one, xyxy=one, counts=one, offsets=one, max_det=max_det, cap=cap, fi=one, sf=one, si=one, hsel=good_sel, dsel=one,
             n_sel=3, mp=mp, hot=_hp(t_out), dot=one, out=one, status=one, scratch=ws, nbytes=need):
        return fn(ctx, frames, ht, dt, B, cams, n_cams, cof, masks, bases, cb, dets, xyxy, counts, offsets, max_det, cap, fi, sf, si,
                  hsel, dsel, n_sel, mp, hot, dot, out, status, scratch, nbytes, None)

    def refused(needle, status=ARG, **kw):
        rc, msg = call(**kw), err()
        assert rc == status and msg.startswith(name.encode()) and needle in msg, (kw, rc, msg)

    assert call(ctx=None) == ARG and err(None).startswith(name.encode() + b": null ctx")
    # the ragged rows: the bases, capacity_bytes, and the masks they place
    refused(b"null dev_mask_bases", bases=None)
    refused(b"dev_mask_bases must be 8-byte aligned", bases=C.c_void_p(4096 + 4))
    refused(b"capacity_bytes must be >= 0", cb=-1)
    refused(b"null pointer", masks=None)                            # capacity_bytes > 0 needs the masks ...
    refused(b"null pointer", masks=None, cap=0)                     # ... whatever the slot capacity says
    refused(b"native masks must be 8-byte aligned", masks=C.c_void_p(4096 + 4))
    # NULL pointers
    for arg in ("frames", "ht", "dt", "cams", "dets", "xyxy", "counts", "offsets", "fi", "sf", "si", "hsel", "dsel", "hot", "dot", "out",
                "status", "scratch"):
        assert call(**{arg: None}) == ARG and err().startswith(name.encode()), arg
    # a table for another canvas, or for another B -- the input table and the out table alike
    small = vti_amd.Engine("n", 2, H=64, W=96, max_batch=4)
    other_canvas, _, _ = small.pack_frames(SHAPES, device="cpu")
    other_out, _, _ = small.pack_frames([SHAPES[b] for b in sel], device="cpu")
    refused(b"another canvas", ht=_hp(other_canvas))
    refused(b"another B", B=3)
    refused(b"another canvas", hot=_hp(other_out))
    assert name.encode() + b" (out table)" in err()
    refused(b"another B", n_sel=2, hsel=(C.c_int32 * 2)(3, 0))      # out table of 3 rows, n_sel = 2
    refused(b"another B", hot=_hp(t_in))                            # 4 rows
    refused(b"n_sel", n_sel=0)
    corrupt = t_in.host.clone()
    corrupt[64] = 1                                                  # row 0's byte offset is no longer a multiple of 16
    refused(b"frame 0 of host_table", ht=C.c_void_p(corrupt.data_ptr()))
    assert call(dt=C.c_void_p(4096 + 8)) == ARG and call(dot=C.c_void_p(4096 + 8)) == ARG
    # the scratch
    refused(b"scratch smaller than vti_annotate_frames_scratch_bytes()", nbytes=need - 1)
    refused(b"256-byte aligned", scratch=C.c_void_p((1 << 20) + 64))
    # the selection
    refused(b"host_select[1] = -1", hsel=(C.c_int32 * 3)(3, -1, 3))
    refused(b"host_select[2] = 4", hsel=(C.c_int32 * 3)(3, 0, B))
    refused(b"row 1 of the out table", hsel=(C.c_int32 * 3)(3, 1, 3))
    refused(b"row 2 of the out table", hsel=(C.c_int32 * 3)(3, 0, 0))
    # a selected frame above 8192 (the table allows 16384): names the frame; not selected, the same table is served
    wide = [(960, 1280), (8200, 480), (720, 960), (1080, 1920)]
    t_wide, _, _ = eng.pack_frames(wide, device="cpu")
    t_wide_out, _, _ = eng.pack_frames([wide[b] for b in (3, 1, 3)], device="cpu")
    refused(b"8192", ht=_hp(t_wide), hot=_hp(t_wide_out), hsel=(C.c_int32 * 3)(3, 1, 3), nbytes=1 << 40)
    assert b"frame 1" in err()
    assert call(ht=_hp(t_wide)) not in (ARG, UNSUPPORTED)
    # the other size and alignment rules of vti_annotate_frames
    for kw in (dict(max_det=1001), dict(max_det=0), dict(mp=-1), dict(n_cams=0), dict(cap=-1)):
        refused(b"bad size", **kw)
    refused(b"16-byte aligned", cams=C.c_void_p(4096 + 8))
    refused(b"4-byte aligned", dsel=C.c_void_p(4096 + 2))
    refused(b"4-byte aligned", cof=C.c_void_p(4096 + 2))
    refused(b"misaligned", sf=C.c_void_p(4096 + 4))
    refused(b"dev_frames and dev_out must be 16-byte aligned", frames=C.c_void_p(4096 + 8))
    refused(b"dev_frames and dev_out must be 16-byte aligned", out=C.c_void_p(4096 + 8))
    # what IS accepted up to the device check: without a GPU the call then stops with the HIP status, never with an argument error.
    # capacity_bytes == 0 needs no masks; the checker's letterbox canvas rule does not apply (no letterbox mask is resized)
    for kw in (dict(), dict(cof=None), dict(cb=0, masks=None), dict(cb=0, masks=None, cap=0), dict(cap=0),
               dict(hsel=(C.c_int32 * 3)(3, 0, 3)), dict(masks=C.c_void_p(4096 + 8))):
        assert call(**kw) not in (ARG, UNSUPPORTED), kw


def test_the_letterbox_forms_keep_refusing_native(lib_built):
    """vti_annotate_frames(native = 1) and vti_annotate_checker_frames(native = 1): VTI_ERR_UNSUPPORTED with the text they always had."""
    vti_amd = lib_built
    L = vti_amd.lib()
    eng = vti_amd.Engine("n", 2, H=736, W=960, max_batch=4)
    sel = [3, 0, 3]
    t_in, _, _ = eng.pack_frames(SHAPES, device="cpu")
    t_out, _, _ = eng.pack_frames([SHAPES[b] for b in sel], device="cpu")
    need = L.vti_annotate_frames_scratch_bytes(eng._ctx, _hp(t_out), 200, 4096)
    one, ws = C.c_void_p(4096), C.c_void_p(1 << 20)
    for name, text in (("vti_annotate_frames", b"vti_annotate_frames: native masks need frames of one size (vti_annotate)"),
                       ("vti_annotate_checker_frames",
                        b"vti_annotate_checker_frames: native masks need frames of one size (vti_annotate_checker_cameras)")):
        rc = getattr(L, name)(eng._ctx, one, _hp(t_in), one, 4, one, 2, one, one, 1, one, one, one, one, 200, 800, one, one, one,
                              (C.c_int32 * 3)(*sel), one, 3, 4096, _hp(t_out), one, one, one, ws, need, None)
        assert rc == UNSUPPORTED and L.vti_last_error(eng._ctx) == text


def test_the_refusals_run_clean_in_a_stand_alone_program_under_the_host_sanitizers(lib_built, tmp_path):
    """tests/annotate_native_frames_args_main.cpp: its own main, built with -fsanitize=address,undefined, linked against libvti.so and
    run directly (nothing is loaded into Python, nothing is preloaded).  Every call it makes is refused before the first HIP call."""
    vti_amd = lib_built
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    lib_dir = os.path.dirname(vti_amd.LIB_PATH)
    exe = str(tmp_path / "annotate_native_frames_args_main")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx).startswith("g++") else []    # no link-order rule to meet
    subprocess.run([cxx, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static, "-I",
                    os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "annotate_native_frames_args_main.cpp"), "-L", lib_dir,
                    "-lvti", "-Wl,-rpath," + lib_dir, "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and re.fullmatch(r"ok \d+\n", run.stdout) and run.stderr == "", (run.returncode, run.stdout, run.stderr)


def _plain_out(torch, B, max_det=8, cap=4):
    return dict(dets=torch.zeros((B, max_det, 38)), xyxy=torch.zeros((B, max_det, 4)), counts=torch.zeros(B, dtype=torch.int32),
                offsets=torch.zeros(B + 1, dtype=torch.int32), masks=torch.zeros((cap, 64, 8), dtype=torch.uint8))


@pytest.mark.parametrize("checker", [False, True], ids=["annotate", "annotate_checker"])
def test_engine_tells_a_ragged_set_from_a_plain_one_before_it_touches_a_device(lib_built, checker):
    import torch
    vti_amd = lib_built
    eng = vti_amd.Engine("n", 2, H=64, W=64, max_batch=2)
    shapes = [(48, 64), (32, 40)]
    table, _, total = eng.pack_frames(shapes, device="cpu")
    max_det = 8
    meas = dict(frame_i32=torch.zeros((2, 6), dtype=torch.int32), stitch_f64=torch.zeros((2 * max_det, 7), dtype=torch.float64),
                stitch_i32=torch.zeros((2 * max_det, 2), dtype=torch.int32))
    params = (vti_amd.CheckerParams if checker else vti_amd.MeasureParams)(*load_calib())
    draw = eng.annotate_checker if checker else eng.annotate
    buf = torch.zeros(total, dtype=torch.uint8)
    # a plain set: refused, and the text says what a ragged set is
    with pytest.raises(ValueError, match="native.*mask_bases"):
        draw(buf, _plain_out(torch, 2), meas, params, [0], native=True, table=table)
    flat = dict(_plain_out(torch, 2), masks=torch.zeros(64, dtype=torch.uint8))          # flat masks alone are not a ragged set
    with pytest.raises(ValueError, match="native.*mask_bases"):
        draw(buf, flat, meas, params, [0], native=True, table=table)
    # the ragged set of alloc_outputs(native_frames=), on the host: past that refusal, as far as the device check
    ragged = eng.alloc_outputs(2, max_det, 0, device="cpu", native_frames=table)
    assert "mask_bases" in ragged and ragged["masks"].dim() == 1 and ragged["masks"].numel() == eng.mask_native_frames_bytes(table, max_det)
    with pytest.raises(ValueError, match="device batch"):
        draw(buf, ragged, meas, params, [1, 0], native=True, table=table)
    with pytest.raises(ValueError, match="device batch"):
        draw(buf, ragged, meas, params, [1, 0], native=True, table=table, capacity_bytes=0)
    with pytest.raises(ValueError, match="device batch"):
        draw(buf, ragged, meas, params, [1], native=True, table=table, capacity_bytes=ragged["masks"].numel())
    # capacity_bytes: an integer inside the buffer, and only with the ragged rows
    for bad in (-1, ragged["masks"].numel() + 1, 1.5, True, "all"):
        with pytest.raises(ValueError, match="capacity_bytes"):
            draw(buf, ragged, meas, params, [0], native=True, table=table, capacity_bytes=bad)
    with pytest.raises(ValueError, match="capacity_bytes"):
        draw(buf, _plain_out(torch, 2), meas, params, [0], table=table, capacity_bytes=0)
    with pytest.raises(ValueError, match="capacity_bytes"):
        draw(torch.zeros((2, 48, 64, 3), dtype=torch.uint8), _plain_out(torch, 2), meas, params, [0], capacity_bytes=0)
    # a set allocated for other shapes than the table's, mask_bases of another length
    other, _, _ = eng.pack_frames([(48, 64), (32, 48)], device="cpu")
    with pytest.raises(ValueError, match="other frame shapes"):
        draw(torch.zeros(other.total_bytes, dtype=torch.uint8), ragged, meas, params, [0], native=True, table=other)
    with pytest.raises(ValueError, match="mask_bases"):
        draw(buf, dict(ragged, mask_bases=ragged["mask_bases"][:2]), meas, params, [0], native=True, table=table)
    # the other refusals of table= stand
    with pytest.raises(ValueError, match="flat uint8"):
        draw(buf.view(1, -1), ragged, meas, params, [0], native=True, table=table)
    with pytest.raises(ValueError, match="select|frame index"):
        draw(buf, ragged, meas, params, [2], native=True, table=table)
    with pytest.raises(ValueError, match="meas needs stitch_i32"):
        draw(buf, ragged, dict(meas, stitch_i32=None), params, [0], native=True, table=table)


def test_process_frames_takes_annotate_native_by_keyword_and_keeps_its_refusals(lib_built, monkeypatch):
    vti_amd = lib_built
    params = vti_amd.MeasureParams(*load_calib())
    cparams = vti_amd.CheckerParams(*load_calib())
    model = vti_amd.YOLO(None, scale="n", nc=2, seed=3)

    def no_predict(*a, **k):
        raise AssertionError("predict was reached")
    for stage in ("_predict_outputs", "_predict_outputs_frames", "_predict_outputs_windows"):
        monkeypatch.setattr(model, stage, no_predict)
    sm = vti_amd.StitchMeasurer(model, params)
    mc = vti_amd.MultiCameraMeasurer(model, [params, params])
    ck = vti_amd.MultiCameraChecker(model, [cparams, cparams])
    a, b = np.zeros((48, 64, 3), np.uint8), np.zeros((32, 64, 3), np.uint8)
    calls = ((sm, ()), (mc, ([0, 1],)), (ck, ([0, 1],)))
    # without the keyword (or with False): the four refusals of today, word for word
    plain = re.escape("process_frames: annotate needs frames of one size; the frames of this list differ in shape "
                      "(vti_annotate has no frame-table form)")
    retina = re.escape("process_frames: retina_masks=True needs frames of one size; the frames of this list differ in shape")
    for kw in (dict(), dict(annotate_native=False)):
        for who, cams in calls:
            with pytest.raises(ValueError, match=plain):
                who.process_frames([a, b], *cams, annotate="all", imgsz=64, **kw)
            with pytest.raises(ValueError, match=retina):
                who.process_frames([a, b], *cams, retina_masks=True, imgsz=64, **kw)
            with pytest.raises(ValueError, match=retina):
                who.process_frames([a, b], *cams, retina_masks=True, annotate="all", mixed=True, imgsz=64, **kw)
        with pytest.raises(ValueError, match=retina):
            sm.process_frames([a, b], window="roi", annotate="all", mixed=True, imgsz=64, **kw)
        with pytest.raises(ValueError, match=retina):
            mc.process_frames([a, b], [0, 1], windows="roi", annotate=[1], mixed=True, imgsz=64, **kw)
    # the keyword does not replace mixed=True
    for who, cams in calls:
        with pytest.raises(ValueError, match=plain):
            who.process_frames([a, b], *cams, retina_masks=True, annotate="all", annotate_native=True, imgsz=64)
    with pytest.raises(ValueError, match=retina):
        sm.process_frames([a, b], window="roi", annotate="all", annotate_native=True, imgsz=64)
    # ... nor the other refusals
    for who, cams in calls:
        with pytest.raises(ValueError, match="encode needs annotate"):
            who.process_frames([a, b], *cams, retina_masks=True, encode="jpeg", mixed=True, annotate_native=True, imgsz=64)
        with pytest.raises(ValueError, match="burn_text needs annotate"):
            who.process_frames([a, b], *cams, retina_masks=True, burn_text=True, mixed=True, annotate_native=True, imgsz=64)
    # a bool, and keyword only
    for bad in ("yes", 1, 0, None):
        for who, cams in calls:
            with pytest.raises(ValueError, match="annotate_native must be True or False"):
                who.process_frames([a, b], *cams, annotate="all", mixed=True, annotate_native=bad, imgsz=64)
    with pytest.raises(TypeError):
        sm.process_frames([a, b], 0.2, 0.25, 200, 960, True, "all", None, 95, True)
    with pytest.raises(TypeError):
        ck.process_frames([a, b], [0, 1], 0.2, 0.45, 200, 64, True, False, "all", None, 95, True)
    # StitchDistanceChecker does not take it, and keeps refusing a mixed list
    one = vti_amd.StitchDistanceChecker(model, cparams)
    with pytest.raises(TypeError):
        one.process_frames([a, b], annotate_native=True)
    with pytest.raises(ValueError, match="needs frames of one size"):
        one.process_frames([a, b])
    # with it (and mixed=True) the call gets as far as the predict
    for who, cams in calls:
        with pytest.raises(AssertionError, match="predict was reached"):
            who.process_frames([a, b], *cams, retina_masks=True, annotate="all", mixed=True, annotate_native=True, imgsz=64)
        with pytest.raises(AssertionError, match="predict was reached"):
            who.process_frames([a, b], *cams, retina_masks=True, annotate=[1], encode="jpeg", mixed=True, annotate_native=True, imgsz=64)
    with pytest.raises(AssertionError, match="predict was reached"):
        sm.process_frames([a, b], window="roi", annotate="all", mixed=True, annotate_native=True, imgsz=64)
    with pytest.raises(AssertionError, match="predict was reached"):
        mc.process_frames([a, b], [0, 1], windows=["roi", None], annotate=[0], encode="jpeg", mixed=True, annotate_native=True, imgsz=64)
    # frames of one size: the keyword changes nothing (the uniform predict is reached, with and without it)
    batch = np.zeros((2, 48, 64, 3), np.uint8)
    for kw in (dict(), dict(annotate_native=True)):
        for who, cams in calls:
            with pytest.raises(AssertionError, match="predict was reached"):
                who.process_frames(batch, *cams, retina_masks=True, annotate="all", imgsz=64, **kw)
    assert model._engines == {}                                     # nothing was built, nothing uploaded
    # an argument all the way down: nothing of it stays on the object, and the public signatures are the old ones
    assert not any(hasattr(who, "_annotate_native") or hasattr(who, "annotate_native") for who, _ in calls)
    sig = lambda cls: inspect.signature(cls.process_frames)
    assert list(sig(vti_amd.StitchMeasurer).parameters) == ["self", "frames", "conf", "iou", "max_det", "imgsz", "retina_masks", "annotate",
                                                            "encode", "jpeg_quality"]
    assert [p.default for p in list(sig(vti_amd.StitchMeasurer).parameters.values())[2:]] == [0.20, 0.25, 200, 960, False, None, None, 95]
    assert list(sig(vti_amd.MultiCameraMeasurer).parameters) == ["self", "frames", "cameras", "conf", "iou", "max_det", "imgsz",
                                                                 "retina_masks", "annotate", "encode", "jpeg_quality"]
    assert [p.default for p in list(sig(vti_amd.MultiCameraMeasurer).parameters.values())[3:]] == [0.20, 0.25, 200, 960, False, None, None, 95]
    ps = sig(vti_amd.MultiCameraChecker).parameters
    assert list(ps) == ["self", "frames", "cameras", "conf", "iou", "max_det", "imgsz", "retina_masks", "rows", "annotate", "encode",
                        "jpeg_quality", "mixed", "burn_text", "extra_text", "rasterise"]
    assert [ps[k].default for k in list(ps)[3:]] == [0.20, 0.45, 200, 640, False, False, None, None, 95, False, False, None, None]
    assert all(ps[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("mixed", "burn_text", "extra_text", "rasterise"))
    from vti_amd.measure import _DeviceStage
    assert "annotate_native" in inspect.signature(_DeviceStage._frame_records).parameters
    for cls in (vti_amd.StitchMeasurer, vti_amd.MultiCameraMeasurer, vti_amd.MultiCameraChecker):
        assert "annotate_native" in inspect.signature(cls._process_frames).parameters
        assert "annotate_native" in cls.process_frames.__doc__
