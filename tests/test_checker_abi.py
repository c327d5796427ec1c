"""vti_measure_checker's C ABI without a GPU: the entry point is declared, exported and bound with the documented signature, the
settings struct has the size of its ctypes mirror, every argument check comes before the first HIP call (fake pointers, never
dereferenced), and vti_measure's own struct and camera-table row keep their sizes (280 and 272 bytes, as before this entry point
existed)."""
import ctypes as C
import dataclasses as dc
import os
import re
import shutil
import subprocess

import pytest

from test_oracle_geometry import load_calib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALIB = load_calib()
FIELDS = ("K", "dist", "R", "t", "max_px_distance", "stitch_id", "fabric_id", "min_stitches", "envelope_neighborhood", "skip_cluster",
          "kmeans_iters", "drop_empty", "frame_buffer")


def test_the_entry_point_is_declared_exported_and_bound(lib_built):
    vti_amd = lib_built
    hdr = open(os.path.join(ROOT, "include", "vti.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", vti_amd.LIB_PATH], check=True, capture_output=True, text=True).stdout
    name = "vti_measure_checker"
    assert re.search(r"\bT %s$" % name, exported, re.M)
    decl = re.search(r"int32_t\s+%s\s*\(([^)]*)\)\s*;" % name, hdr).group(1)
    args = [" ".join(a.split()) for a in decl.split(",")]
    assert args == ["vti_ctx* ctx", "const vti_checker_params* params", "const uint8_t* dev_masks", "int32_t native",
                    "const float* dev_dets", "const float* dev_xyxy", "const int32_t* dev_counts", "const int32_t* dev_offsets",
                    "int32_t B", "int32_t max_det", "int32_t capacity", "int32_t H0", "int32_t W0", "void* dev_scratch",
                    "size_t scratch_bytes", "double* frame_f64", "int32_t* frame_i32", "double* stitch_f64", "int32_t* stitch_i32",
                    "void* stream"]
    P, I32 = C.c_void_p, C.c_int32
    res, argtypes = vti_amd.SIGNATURES[name]
    assert res is I32 and argtypes == [P, C.POINTER(vti_amd._lib.VtiCheckerParams), P, I32, P, P, P, P, I32, I32, I32, I32, I32, P,
                                       C.c_size_t, P, P, P, P, P]
    # the same shape as vti_measure but for the settings struct
    assert [a for k, a in enumerate(argtypes) if k != 1] == [a for k, a in enumerate(vti_amd.SIGNATURES["vti_measure"][1]) if k != 1]
    for public in ("CheckerParams", "StitchDistanceChecker", "checker_text_items"):
        assert public in vti_amd.__all__ and hasattr(vti_amd, public)
    assert hasattr(vti_amd.Engine, "measure_checker")


@pytest.fixture(scope="module")
def c_sizes(tmp_path_factory):
    """sizeof / offsetof as a C++ compiler sees include/vti.h."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    cmd = [cxx, "-x", "c++"] if cxx else ["/opt/rocm/bin/hipcc", "-x", "c++"]      # the compiler build() needs is always there
    d = tmp_path_factory.mktemp("sizes")
    src = d / "sizes.cpp"
    offs = "".join(f"        case {k + 1}: return (long)offsetof(vti_checker_params, {f});\n" for k, f in enumerate(FIELDS))
    src.write_text('#include <cstddef>\n#include "vti.h"\nextern "C" long vti_size_of(int what) {\n    switch (what) {\n'
                   "        case 0: return (long)sizeof(vti_checker_params);\n" + offs +
                   "        case 100: return (long)sizeof(vti_measure_params);\n        default: return -1;\n    }\n}\n")
    so = str(d / "libsizes.so")
    subprocess.run(cmd + ["-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), "-o", so, str(src)], check=True)
    fn = C.CDLL(so).vti_size_of
    fn.restype, fn.argtypes = C.c_long, [C.c_int]
    return fn


def test_the_settings_struct_matches_its_mirror_and_the_old_ones_keep_their_sizes(lib_built, c_sizes):
    vti_amd = lib_built
    M = vti_amd._lib.VtiCheckerParams
    assert c_sizes(0) == C.sizeof(M) == 248
    assert [name for name, _ in M._fields_] == list(FIELDS)
    for k, f in enumerate(FIELDS):
        assert c_sizes(k + 1) == getattr(M, f).offset, f
    # vti_measure's struct and its camera-table row: byte for byte what they were
    assert c_sizes(100) == C.sizeof(vti_amd._lib.VtiMeasureParams) == 280
    assert vti_amd.lib().vti_measure_cameras_bytes(1) == 272
    p = vti_amd.CheckerParams(*CALIB).to_c()
    assert (p.max_px_distance, p.stitch_id, p.fabric_id, p.min_stitches, p.envelope_neighborhood, p.skip_cluster, p.kmeans_iters,
            p.drop_empty, p.frame_buffer) == (150.0, 0, 1, 3, 3, 0, 10, 0, 8)
    assert list(p.K) == CALIB[0].ravel().tolist() and list(p.t) == CALIB[3].tolist()
    G = os.path.join(ROOT, "tests", "golden")
    q = vti_amd.CheckerParams.from_files(os.path.join(G, "camera_calibration.json"), os.path.join(G, "extrinsics.json"), min_stitches=5)
    m = vti_amd.MeasureParams.from_files(os.path.join(G, "camera_calibration.json"), os.path.join(G, "extrinsics.json"))
    assert q.min_stitches == 5 and q.max_px_distance == 150 and (q.R == m.R).all() and (q.K == m.K).all()
    with pytest.raises(ValueError):
        dc.replace(q, dist=[0.0] * 4).to_c()


def test_argument_checks_come_before_any_hip_call(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    eng = vti_amd.Engine("n", 2, H=64, W=64, max_batch=2)
    p = vti_amd.CheckerParams(*CALIB)
    B, max_det, cap, H0, W0 = 2, 10, 20, 48, 64
    need = eng.measure_scratch_bytes(B, cap, W0)
    one, ws = C.c_void_p(4096), C.c_void_p(1 << 20)           # never dereferenced: every check comes before any HIP call

    def call(params=p, ctx=eng._ctx, masks=one, native=0, dets=one, xyxy=one, counts=one, offsets=one, B=B, max_det=max_det, cap=cap,
             scratch=ws, nbytes=need, frame_f64=one, frame_i32=one):
        cp = params.to_c() if params is not None else None
        return L.vti_measure_checker(ctx, C.byref(cp) if cp is not None else None, masks, native, dets, xyxy, counts, offsets, B,
                                     max_det, cap, H0, W0, scratch, nbytes, frame_f64, frame_i32, None, None, None)

    def refused(**kw):
        """VTI_ERR_ARG, and vti_last_error names the function."""
        rc = call(**kw)
        msg = L.vti_last_error(eng._ctx)
        return rc == -1 and msg.startswith(b"vti_measure_checker:"), (rc, msg)

    assert call(ctx=None) == -1
    for name in ("params", "masks", "dets", "xyxy", "counts", "offsets", "frame_f64", "frame_i32", "scratch"):
        ok, what = refused(**{name: None})
        assert ok, (name, what)
    ok, what = refused(cap=-1)
    assert ok, what
    assert refused(B=-1)[0] and refused(max_det=0)[0] and refused(native=2)[0]
    ok, what = refused(max_det=vti_amd._lib.VTI_MEASURE_MAX_DET + 1)
    assert ok and b"VTI_MEASURE_MAX_DET" in what[1], what
    assert call(max_det=vti_amd._lib.VTI_MEASURE_MAX_DET, B=0, cap=0, masks=None, nbytes=0, scratch=None) == 0
    ok, what = refused(nbytes=need - 1)
    assert ok and b"scratch smaller" in what[1], what
    ok, what = refused(scratch=C.c_void_p((1 << 20) + 64))
    assert ok and b"256-byte aligned" in what[1], what
    ok, what = refused(params=dc.replace(p, fabric_id=0))
    assert ok and b"stitch_id and fabric_id" in what[1], what
    assert refused(params=dc.replace(p, stitch_id=-1))[0]
    for nb in (-1, 65):
        ok, what = refused(params=dc.replace(p, envelope_neighborhood=nb))
        assert ok and b"envelope_neighborhood" in what[1], (nb, what)
    for nb in (0, 64):      # the two ends of the range pass the checks (nothing to do: no launch)
        assert call(params=dc.replace(p, envelope_neighborhood=nb), B=0, cap=0, masks=None, nbytes=0, scratch=None) == 0
    assert refused(params=dc.replace(p, min_stitches=0))[0] and refused(params=dc.replace(p, kmeans_iters=-1))[0]
    assert refused(params=dc.replace(p, frame_buffer=0))[0] and refused(params=dc.replace(p, max_px_distance=float("nan")))[0]
    assert refused(masks=C.c_void_p(4096 + 8))[0]                 # letterbox bits: 16-byte loads
    assert refused(masks=C.c_void_p(4096 + 4), native=1)[0]       # native rows: 8-byte loads
    assert call(masks=C.c_void_p(4096 + 8), native=1, B=0) == 0   # ... for which 8-byte alignment is enough
    assert call(B=0, cap=0, masks=None, nbytes=0, scratch=None) == 0          # nothing to do: no launch
    assert call(B=0, cap=0, masks=None, nbytes=0, scratch=None, params=None) == -1


def test_engine_measure_checker_needs_the_frame_size(lib_built):
    import torch
    eng = lib_built.Engine("n", 2, H=64, W=64, max_batch=2)
    out = dict(dets=torch.zeros((2, 10, 38)), xyxy=torch.zeros((2, 10, 4)), counts=torch.zeros(2, dtype=torch.int32),
               offsets=torch.zeros(3, dtype=torch.int32), masks=torch.zeros((0, 64, 8), dtype=torch.uint8))
    with pytest.raises(ValueError):
        eng.measure_checker(out, lib_built.CheckerParams(*CALIB))
