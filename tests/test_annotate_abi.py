"""vti_annotate's C ABI without a GPU: the two entry points exist, the scratch size, every argument check (all before the first HIP
call: fake pointers, never dereferenced), and the Python surface refuses what it cannot serve before it touches a device.  The GPU
parity tests are in test_gpu_annotate.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_oracle_geometry import load_calib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vti_annotate_scratch_bytes", "vti_annotate")


def test_the_entry_points_are_declared_exported_and_bound(lib_built):
    vti_amd = lib_built
    hdr = open(os.path.join(ROOT, "include", "vti.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", vti_amd.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"\bT %s$" % name, exported, re.M), name
        assert name in vti_amd.SIGNATURES
    assert hasattr(vti_amd.Engine, "annotate") and "annotate" in vti_amd.__all__
    assert vti_amd._lib.VTI_ANNOTATE_OUTLINE_SKIPPED == 1 and re.search(r"VTI_ANNOTATE_OUTLINE_SKIPPED\s*=\s*1", hdr)


def test_scratch_bytes_is_zero_on_bad_arguments_and_monotone(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    eng = vti_amd.Engine("n", 2, H=736, W=960, max_batch=1)
    f = lambda n_sel=8, max_det=200, H0=960, W0=1280, mp=4096, ctx=eng._ctx: L.vti_annotate_scratch_bytes(ctx, n_sel, max_det, H0, W0, mp)
    base = f()
    assert base > 0 and base % 256 == 0
    # per frame at least: the records, the envelope's points, the outline's vertices and the union's bit rows
    assert base >= 8 * (32 * (3 + 7 * 200) + 8 * 1280 + 8 * 4096 + 960 * 20 * 8)
    assert f(ctx=None) == 0 and f(n_sel=0) == 0 and f(n_sel=-1) == 0 and f(max_det=0) == 0 and f(max_det=1001) == 0
    assert f(H0=0) == 0 and f(W0=0) == 0 and f(H0=8193) == 0 and f(W0=8193) == 0 and f(mp=-1) == 0
    assert f(mp=0) > 0 and f(max_det=1000) > 0 and f(H0=8192, W0=8192, n_sel=1) > 0
    sizes = [f(n_sel=n) for n in (1, 2, 8, 64)]
    assert sizes == sorted(sizes) and len(set(sizes)) == 4
    sizes = [f(mp=m) for m in (0, 1, 100, 4096, 1 << 20)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
    assert eng.annotate_scratch_bytes(8, 200, 960, 1280, 4096) == base


def test_annotate_argument_checks_come_before_any_hip_call(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    eng = vti_amd.Engine("n", 2, H=736, W=960, max_batch=4)
    B, H0, W0, max_det, cap, n_sel, mp = 4, 960, 1280, 200, 800, 3, 4096
    need = eng.annotate_scratch_bytes(n_sel, max_det, H0, W0, mp)
    one, ws = C.c_void_p(4096), C.c_void_p(1 << 20)            # never dereferenced
    good_sel = (C.c_int32 * n_sel)(3, 0, 3)

    def call(ctx=eng._ctx, frames=one, B=B, H0=H0, W0=W0, cams=one, n_cams=2, cof=one, masks=one, native=0, dets=one, xyxy=one,
             counts=one, offsets=one, max_det=max_det, cap=cap, fi=one, sf=one, si=one, hsel=good_sel, dsel=one, n_sel=n_sel, mp=mp,
             out=one, status=one, scratch=ws, nbytes=need):
        return L.vti_annotate(ctx, frames, B, H0, W0, cams, n_cams, cof, masks, native, dets, xyxy, counts, offsets, max_det, cap,
                              fi, sf, si, hsel, dsel, n_sel, mp, out, status, scratch, nbytes, None)

    assert call(ctx=None) == -1
    for name in ("frames", "cams", "dets", "xyxy", "counts", "offsets", "fi", "sf", "si", "hsel", "dsel", "out", "status", "scratch"):
        assert call(**{name: None}) == -1, name
    assert b"null pointer" in L.vti_last_error(eng._ctx) or b"scratch" in L.vti_last_error(eng._ctx)
    assert call(masks=None) == -1                               # capacity > 0 needs the masks ...
    assert call(n_sel=0) == -1 and call(n_sel=-2) == -1
    assert call(hsel=(C.c_int32 * 3)(0, -1, 1)) == -1
    assert b"host_select[1] = -1" in L.vti_last_error(eng._ctx)
    assert call(hsel=(C.c_int32 * 3)(0, 1, B)) == -1
    assert b"host_select[2] = 4" in L.vti_last_error(eng._ctx)
    assert call(native=2) == -1 and call(native=-1) == -1
    assert call(masks=C.c_void_p(4096 + 8)) == -1               # letterbox bits: 16-byte aligned
    assert b"16-byte" in L.vti_last_error(eng._ctx)
    assert call(native=1, masks=C.c_void_p(4096 + 4)) == -1     # native rows: 8-byte aligned
    assert call(scratch=C.c_void_p((1 << 20) + 64)) == -1
    assert call(nbytes=need - 1) == -1
    assert b"scratch" in L.vti_last_error(eng._ctx)
    assert call(max_det=1001) == -1 and call(max_det=0) == -1
    assert call(mp=-1) == -1
    assert call(B=0) == -1 and call(n_cams=0) == -1 and call(cap=-1) == -1
    assert call(H0=0) == -1 and call(W0=8193, nbytes=1 << 40) == -1
    assert call(cams=C.c_void_p(4096 + 8)) == -1 and call(cof=C.c_void_p(4096 + 2)) == -1 and call(dsel=C.c_void_p(4096 + 2)) == -1
    assert call(sf=C.c_void_p(4096 + 4)) == -1
    # what IS accepted up to the device check: NULL camera index (row 0), no masks when the capacity is 0, native rows at 8 bytes.
    # Without a GPU the call then stops at the device check, with the HIP status, never with VTI_ERR_ARG.
    for kw in (dict(cof=None), dict(cap=0, masks=None), dict(native=1, masks=C.c_void_p(4096 + 8)), dict(hsel=(C.c_int32 * 3)(2, 2, 2))):
        assert call(**kw) != -1, kw


def _fake_out(torch, B, max_det=8, cap=4):
    return dict(dets=torch.zeros((B, max_det, 38)), xyxy=torch.zeros((B, max_det, 4)), counts=torch.zeros(B, dtype=torch.int32),
                offsets=torch.zeros(B + 1, dtype=torch.int32), masks=torch.zeros((cap, 64, 8), dtype=torch.uint8))


def test_engine_annotate_refuses_bad_input_before_it_touches_a_device(lib_built):
    import torch
    vti_amd = lib_built
    eng = vti_amd.Engine("n", 2, H=64, W=64, max_batch=2)
    B = 2
    out = _fake_out(torch, B)
    meas = dict(frame_i32=torch.zeros((B, 6), dtype=torch.int32), stitch_f64=torch.zeros((4, 7), dtype=torch.float64),
                stitch_i32=torch.zeros((4, 2), dtype=torch.int32))
    params = vti_amd.MeasureParams(*load_calib())
    frames = torch.zeros((B, 48, 64, 3), dtype=torch.uint8)         # a host batch: the shape and value checks come first
    with pytest.raises(ValueError, match="uint8"):
        eng.annotate(frames.float(), out, meas, params, [0])
    for sel in ([B], [-1], [0, 1, 2], [], [[0]], [0.5]):
        with pytest.raises(ValueError, match="select|frame index"):
            eng.annotate(frames, out, meas, params, sel)
    with pytest.raises(ValueError, match="stitch_rows"):
        eng.annotate(frames, out, dict(frame_i32=meas["frame_i32"]), params, [0])
    with pytest.raises(ValueError, match="frames but an output set"):
        eng.annotate(frames, _fake_out(torch, 3), meas, params, [0])
    with pytest.raises(ValueError, match="device batch"):              # a good call on host memory stops at the device check
        eng.annotate(frames, out, meas, params, [0])


def test_process_frames_refuses_a_bad_selection_and_differing_sizes(lib_built, monkeypatch):
    import torch
    vti_amd = lib_built
    params = vti_amd.MeasureParams(*load_calib())
    model = vti_amd.YOLO(None, scale="n", nc=2, seed=3)
    sm = vti_amd.StitchMeasurer(model, params)
    mc = vti_amd.MultiCameraMeasurer(model, [params, params])
    a, b = np.zeros((48, 64, 3), np.uint8), np.zeros((32, 64, 3), np.uint8)
    # frames of differing sizes: refused by name before anything is predicted
    with pytest.raises(ValueError, match="annotate needs frames of one size"):
        sm.process_frames([a, b], annotate="all")
    with pytest.raises(ValueError, match="annotate needs frames of one size"):
        mc.process_frames([a, b], [0, 1], annotate=[0])
    # a selection outside the batch: refused once the batch size is known, before the measurement (predict is stubbed: no GPU here)
    B = 3
    eng = vti_amd.Engine("n", 2, H=64, W=64, max_batch=B)
    monkeypatch.setattr(model, "_predict_outputs", lambda *a, **k: (eng, _fake_out(torch, B), (B, 48, 64), (64, 64)))
    frames = np.zeros((B, 48, 64, 3), np.uint8)
    for sel in ([B], [0, -1], [], "every"):
        with pytest.raises(ValueError):
            sm.process_frames(frames, annotate=sel)
        with pytest.raises(ValueError):
            mc.process_frames(frames, [0, 1, 0], annotate=sel)
