"""vti_annotate_checker's C ABI without a GPU: the entry point is declared, exported and bound with the documented signature, every
argument check returns VTI_ERR_ARG with a message before the first HIP call (fake pointers, never dereferenced; every call here is
refused, so none launches anything), the Python surface refuses what it cannot serve before it touches a device, and the
stand-alone program tests/annotate_checker_args_main.cpp runs the same checks clean under the host sanitizers.  The GPU parity tests
are in test_gpu_annotate_checker.py."""
import ctypes as C
import dataclasses as dc
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from test_oracle_geometry import load_calib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALIB = load_calib()
NAME = "vti_annotate_checker"


def test_the_entry_point_is_declared_exported_and_bound(lib_built):
    vti_amd = lib_built
    hdr = open(os.path.join(ROOT, "include", "vti.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", vti_amd.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT %s$" % NAME, exported, re.M)
    decl = re.search(r"int32_t\s+%s\s*\(([^)]*)\)\s*;" % NAME, hdr).group(1)
    args = [" ".join(a.split()) for a in decl.split(",")]
    assert args == ["vti_ctx* ctx", "const uint8_t* dev_frames", "int32_t B", "int32_t H0", "int32_t W0", "const vti_checker_params* params",
                    "const uint8_t* dev_masks", "int32_t native", "const float* dev_dets", "const float* dev_xyxy",
                    "const int32_t* dev_counts", "const int32_t* dev_offsets", "int32_t max_det", "int32_t capacity",
                    "const int32_t* frame_i32", "const double* stitch_f64", "const int32_t* stitch_i32", "const int32_t* host_select",
                    "const int32_t* dev_select", "int32_t n_sel", "int32_t max_points", "uint8_t* dev_out", "int32_t* dev_status",
                    "void* dev_scratch", "size_t scratch_bytes", "void* stream"]
    P, I32 = C.c_void_p, C.c_int32
    res, argtypes = vti_amd.SIGNATURES[NAME]
    assert res is I32 and argtypes == [P, P, I32, I32, I32, C.POINTER(vti_amd._lib.VtiCheckerParams), P, I32, P, P, P, P, I32, I32, P, P,
                                       P, P, P, I32, I32, P, P, P, C.c_size_t, P]
    # vti_annotate's shape with the settings struct in the place of the camera table, its row count and the per-frame index
    theirs = vti_amd.SIGNATURES["vti_annotate"][1]
    assert argtypes[:5] == theirs[:5] and argtypes[6:] == theirs[8:]
    assert "vti_annotate_scratch_bytes" in hdr[hdr.index("the stitch-distance checker's picture on device"):hdr.index("int32_t " + NAME)]
    assert "the drawing left out" not in hdr
    assert hasattr(vti_amd.Engine, "annotate_checker") and callable(vti_amd.annotate.checker_display_list)
    assert "checker_display_list" in vti_amd.__all__ and vti_amd.checker_display_list is vti_amd.annotate.checker_display_list
    readme = open(os.path.join(ROOT, "README.md")).read()
    declared = len(re.findall(r"^(?:int32_t|int64_t|void|const char\*)\s+vti_\w+\s*\(", hdr, re.M))
    assert declared == 73 and f"{declared} entry points" in readme


def test_argument_checks_come_before_any_hip_call(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    eng = vti_amd.Engine("n", 2, H=736, W=960, max_batch=4)
    p = vti_amd.CheckerParams(*CALIB)
    B, H0, W0, max_det, cap, n_sel, mp = 4, 960, 1280, 200, 800, 3, 4096
    need = eng.annotate_scratch_bytes(n_sel, max_det, H0, W0, mp)
    one, ws = C.c_void_p(4096), C.c_void_p(1 << 20)            # never dereferenced
    good_sel = (C.c_int32 * n_sel)(3, 0, 3)

    def call(ctx=eng._ctx, frames=one, B=B, H0=H0, W0=W0, params=p, masks=one, native=0, dets=one, xyxy=one, counts=one, offsets=one,
             max_det=max_det, cap=cap, fi=one, sf=one, si=one, hsel=good_sel, dsel=one, n_sel=n_sel, mp=mp, out=one, status=one,
             scratch=ws, nbytes=need):
        cp = params.to_c() if params is not None else None
        return L.vti_annotate_checker(ctx, frames, B, H0, W0, C.byref(cp) if cp is not None else None, masks, native, dets, xyxy, counts,
                                      offsets, max_det, cap, fi, sf, si, hsel, dsel, n_sel, mp, out, status, scratch, nbytes, None)

    def refused(needle=b"", **kw):
        """VTI_ERR_ARG, and vti_last_error names the function and the argument."""
        rc = call(**kw)
        msg = L.vti_last_error(eng._ctx)
        assert rc == -1 and msg.startswith(b"vti_annotate_checker:") and needle in msg, (kw, rc, msg)

    assert call(ctx=None) == -1
    refused(b"null", params=None)
    for name in ("frames", "masks", "dets", "xyxy", "counts", "offsets", "fi", "sf", "si", "hsel", "dsel", "out", "status"):
        refused(b"null pointer", **{name: None})
    refused(b"scratch", scratch=None)
    refused(b"bad size", n_sel=0)
    refused(b"bad size", n_sel=-2)
    refused(b"host_select[1] = -1", hsel=(C.c_int32 * 3)(0, -1, 1))
    refused(b"host_select[2] = 4", hsel=(C.c_int32 * 3)(0, 1, B))
    refused(b"VTI_MEASURE_MAX_DET", max_det=vti_amd._lib.VTI_MEASURE_MAX_DET + 1)
    refused(b"bad size", max_det=0)
    refused(b"8192", H0=8193, nbytes=1 << 40)
    refused(b"8192", W0=8193, nbytes=1 << 40)
    refused(b"bad size", H0=0)
    refused(b"bad size", B=0)
    refused(b"bad size", cap=-1)
    refused(b"bad size", mp=-1)
    refused(b"bad size", native=2)
    refused(b"scratch smaller", nbytes=need - 1)
    refused(b"256-byte aligned", scratch=C.c_void_p((1 << 20) + 64))
    refused(b"16-byte", masks=C.c_void_p(4096 + 8))                # letterbox bits: 16-byte loads
    refused(b"8-byte", native=1, masks=C.c_void_p(4096 + 4))        # native rows: 8-byte loads
    refused(b"aligned", dsel=C.c_void_p(4096 + 2))
    refused(b"misaligned", sf=C.c_void_p(4096 + 4))
    refused(b"stitch_id and fabric_id", params=dc.replace(p, fabric_id=0))             # equal class ids
    refused(b"stitch_id and fabric_id", params=dc.replace(p, stitch_id=-1))
    for nb in (-1, 65):
        refused(b"envelope_neighborhood", params=dc.replace(p, envelope_neighborhood=nb))
    refused(b"bad setting", params=dc.replace(p, min_stitches=0))
    refused(b"bad setting", params=dc.replace(p, frame_buffer=0))
    refused(b"NaN", params=dc.replace(p, max_px_distance=float("nan")))


def _fake_out(torch, B, max_det=8, cap=4):
    return dict(dets=torch.zeros((B, max_det, 38)), xyxy=torch.zeros((B, max_det, 4)), counts=torch.zeros(B, dtype=torch.int32),
                offsets=torch.zeros(B + 1, dtype=torch.int32), masks=torch.zeros((cap, 64, 8), dtype=torch.uint8))


def test_engine_annotate_checker_refuses_bad_input_before_it_touches_a_device(lib_built):
    import torch
    vti_amd = lib_built
    eng = vti_amd.Engine("n", 2, H=64, W=64, max_batch=2)
    B = 2
    out = _fake_out(torch, B)
    meas = dict(frame_i32=torch.zeros((B, 6), dtype=torch.int32), stitch_f64=torch.zeros((4, 7), dtype=torch.float64),
                stitch_i32=torch.zeros((4, 2), dtype=torch.int32))
    params = vti_amd.CheckerParams(*CALIB)
    frames = torch.zeros((B, 48, 64, 3), dtype=torch.uint8)         # a host batch: the shape and value checks come first
    with pytest.raises(ValueError, match="uint8"):
        eng.annotate_checker(frames.float(), out, meas, params, [0])
    for sel in ([B], [-1], [0, 1, 2], [], [[0]], [0.5]):
        with pytest.raises(ValueError, match="select|frame index"):
            eng.annotate_checker(frames, out, meas, params, sel)
    with pytest.raises(ValueError, match="stitch_rows"):
        eng.annotate_checker(frames, out, dict(frame_i32=meas["frame_i32"]), params, [0])
    with pytest.raises(ValueError, match="frames but an output set"):
        eng.annotate_checker(frames, _fake_out(torch, 3), meas, params, [0])
    with pytest.raises(ValueError, match="device batch"):              # a good call on host memory stops at the device check
        eng.annotate_checker(frames, out, meas, params, [0])


def test_process_frames_refuses_a_bad_encode_or_selection_before_it_predicts(lib_built, monkeypatch):
    import torch
    vti_amd = lib_built
    model = vti_amd.YOLO(None, scale="n", nc=2, seed=3)
    ck = vti_amd.StitchDistanceChecker(model, vti_amd.CheckerParams(*CALIB))
    frames = np.zeros((3, 48, 64, 3), np.uint8)

    def no_predict(*a, **k):
        raise AssertionError("predict was reached")
    monkeypatch.setattr(model, "_predict_outputs", no_predict)
    with pytest.raises(ValueError, match="encode needs annotate"):
        ck.process_frames(frames, encode="jpeg")
    with pytest.raises(ValueError, match='encode must be None or "jpeg"'):
        ck.process_frames(frames, annotate="all", encode="png")
    with pytest.raises(ValueError, match="jpeg_quality"):
        ck.process_frames(frames, annotate="all", encode="jpeg", jpeg_quality=0)
    with pytest.raises(ValueError, match="needs frames of one size"):
        ck.process_frames([frames[0], np.zeros((32, 64, 3), np.uint8)], annotate="all")
    # a selection outside the batch: refused once the batch size is known, before the measurement (predict is stubbed: no GPU here)
    eng = vti_amd.Engine("n", 2, H=64, W=64, max_batch=3)
    monkeypatch.setattr(model, "_predict_outputs", lambda *a, **k: (eng, _fake_out(torch, 3), (3, 48, 64), (64, 64)))
    for sel in ([3], [0, -1], [], "every"):
        with pytest.raises(ValueError):
            ck.process_frames(frames, annotate=sel)
    import inspect
    sig = inspect.signature(vti_amd.StitchDistanceChecker.process_frames)
    assert [sig.parameters[k].default for k in ("annotate", "encode", "jpeg_quality", "rows")] == [None, None, 95, False]
    assert list(sig.parameters)[:7] == ["self", "frames", "conf", "iou", "max_det", "imgsz", "retina_masks"]


def test_the_argument_checks_run_clean_in_a_stand_alone_program_under_the_host_sanitizers(lib_built, tmp_path):
    """tests/annotate_checker_args_main.cpp: its own main, built with -fsanitize=address,undefined, linked against libvti.so and run
    directly (nothing is loaded into Python, nothing is preloaded).  Every call it makes is refused before the first HIP call."""
    vti_amd = lib_built
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    lib_dir = os.path.dirname(vti_amd.LIB_PATH)
    exe = str(tmp_path / "annotate_checker_args_main")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx).startswith("g++") else []    # no link-order rule to meet
    subprocess.run([cxx, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "annotate_checker_args_main.cpp"), "-L", lib_dir, "-lvti", "-Wl,-rpath," + lib_dir,
                    "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and re.fullmatch(r"ok \d+\n", run.stdout) and run.stderr == "", (run.returncode, run.stdout, run.stderr)
    assert int(run.stdout.split()[1]) >= 40
