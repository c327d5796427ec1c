"""The stitch-distance checker's rig forms without a GPU: the six entry points are declared with their marker, exported and bound
with the documented argument lists; vti_checker_pack_cameras validates every entry and is deterministic; every argument check of the
five device calls comes before the first HIP call (fake pointers, never dereferenced; without a GPU a call that gets past them ends
with the HIP status instead); Engine and MultiCameraChecker refuse bad input before they touch a device; every camera keeps its own
pair of deques; and the stand-alone program tests/checker_rig_args_main.cpp repeats the refusals clean under the host sanitizers.
The GPU parity tests are in test_gpu_checker_rig.py."""
import ctypes as C
import dataclasses as dc
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

from test_oracle_geometry import load_calib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
CALIB = load_calib()
NAMES = ("vti_checker_pack_cameras", "vti_measure_checker_cameras", "vti_measure_checker_frames", "vti_measure_checker_frames_native",
         "vti_annotate_checker_cameras", "vti_annotate_checker_frames")
TWIN = {"vti_measure_checker_cameras": "vti_measure_cameras", "vti_measure_checker_frames": "vti_measure_frames",
        "vti_measure_checker_frames_native": "vti_measure_frames_native", "vti_annotate_checker_cameras": "vti_annotate",
        "vti_annotate_checker_frames": "vti_annotate_frames"}
SHAPES = [(960, 1280), (481, 333), (720, 960), (1080, 1920)]
ARG, UNSUPPORTED = -1, -6


def _hp(t):
    return C.c_void_p(t.host.data_ptr())


def _args(hdr, name):
    decl = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, hdr).group(1)
    return [" ".join(a.split()) for a in decl.split(",")]


def test_the_six_entry_points_are_declared_with_the_marker_exported_and_bound(lib_built):
    vti_amd = lib_built
    hdr = open(os.path.join(ROOT, "include", "vti.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", vti_amd.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert re.search(r"^#define VTI_CHECKER_RIG_API$", hdr, re.M)
    marked = re.findall(r"^VTI_CHECKER_RIG_API (?:int32_t|int64_t)\s+(vti_\w+)\s*\(", hdr, re.M)
    assert tuple(marked) == NAMES
    for name in NAMES:
        assert re.search(r"\bT %s$" % name, exported, re.M), name
        assert name in vti_amd.SIGNATURES
    # the documented argument lists: the measure twin's word for word; the picture's with the table in the struct's place
    for name, twin in TWIN.items():
        assert _args(hdr, name) == _args(hdr, twin), name
        assert vti_amd.SIGNATURES[name] == vti_amd.SIGNATURES[twin], name
    assert _args(hdr, NAMES[0]) == ["vti_ctx* ctx", "const vti_checker_params* params", "int32_t n_cams", "void* host_table", "size_t nbytes"]
    P = C.c_void_p
    assert vti_amd.SIGNATURES[NAMES[0]] == (C.c_int32, [P, C.POINTER(vti_amd._lib.VtiCheckerParams), C.c_int32, P, C.c_size_t])
    uniform = _args(hdr, "vti_annotate_checker")
    at = uniform.index("const vti_checker_params* params")
    assert _args(hdr, "vti_annotate_checker_cameras") == (uniform[:at] + ["const void* dev_cameras", "int32_t n_cams",
                                                                           "const int32_t* dev_camera_of_frame"] + uniform[at + 1:])
    # the table has the measure table's size: no new size query
    section = hdr[hdr.index("#define VTI_CHECKER_RIG_API"):hdr.index("int32_t vti_checker_pack_cameras")]
    assert "vti_measure_cameras_bytes(n_cams)" in section
    assert "MultiCameraChecker" in vti_amd.__all__ and hasattr(vti_amd.Engine, "pack_checker_cameras")
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "MultiCameraChecker" in readme and all(name in readme for name in NAMES)


def _two(vti_amd):
    calib = os.path.join(G, "camera_calibration.json")
    p, q = (vti_amd.MeasureParams.from_files(calib, os.path.join(G, name)) for name in ("extrinsics.json", "camera_extrinsics.json"))
    return [vti_amd.CheckerParams(x.K, x.dist, x.R, x.t) for x in (p, q)]


def test_checker_pack_cameras_validates_every_entry_and_is_deterministic(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    eng = vti_amd.Engine("n", 2, H=64, W=64, max_batch=2)
    p, q = _two(vti_amd)
    row = L.vti_measure_cameras_bytes(1)

    def pack(params, n=None, out="alloc", nbytes=None):
        n = len(params) if n is None else n
        arr = (vti_amd._lib.VtiCheckerParams * max(len(params), 1))(*[x.to_c() for x in params]) if params is not None else None
        buf = (C.c_uint8 * max(row * max(n, 1), 1))(*([0xA5] * max(row * max(n, 1), 1))) if out == "alloc" else out
        rc = L.vti_checker_pack_cameras(eng._ctx, arr, n, buf, row * n if nbytes is None else nbytes)
        return rc, (bytes(buf) if buf is not None else None)

    rc, a = pack([p, q, p])
    assert rc == 0
    rc, b = pack([p, q, p])
    assert rc == 0 and a == b                                                # equal inputs, equal bytes (padding included)
    assert a[:row] == a[2 * row:3 * row] and a[:row] != a[row:2 * row]
    for change in (dict(fabric_id=0, stitch_id=1), dict(skip_cluster=True), dict(drop_empty=True), dict(min_stitches=2),
                   dict(envelope_neighborhood=5), dict(max_px_distance=40.0), dict(kmeans_iters=3)):
        rc, c = pack([dc.replace(p, **change)])
        assert rc == 0 and c[:row] != a[:row], change                        # every setting the kernels read is part of the row
    rc, d = pack([dc.replace(p, frame_buffer=3)])
    assert rc == 0 and d[:row] == a[:row]                                    # frame_buffer is the host's
    # the bad settings of test_annotate_checker_abi.py, each at every index: the message names the index and the setting
    bad = [(dc.replace(p, fabric_id=0), b"stitch_id and fabric_id"), (dc.replace(p, stitch_id=-1), b"stitch_id and fabric_id"),
           (dc.replace(p, envelope_neighborhood=-1), b"envelope_neighborhood"), (dc.replace(p, envelope_neighborhood=65), b"envelope_neighborhood"),
           (dc.replace(p, min_stitches=0), b"bad setting"), (dc.replace(p, frame_buffer=0), b"bad setting"),
           (dc.replace(p, max_px_distance=float("nan")), b"NaN")]
    for x, needle in bad:
        for k in range(3):
            lst = [p, q, p]
            lst[k] = x
            rc, out = pack(lst)
            msg = L.vti_last_error(eng._ctx)
            assert rc == ARG and msg.startswith(b"vti_checker_pack_cameras: camera %d:" % k) and needle in msg, (x, k, msg)
            assert out == bytes([0xA5]) * (3 * row)                          # nothing is written when an entry fails
    assert pack([p, dc.replace(p, envelope_neighborhood=65), dc.replace(p, min_stitches=0)])[0] == ARG
    assert b"camera 1:" in L.vti_last_error(eng._ctx)
    assert pack(None, n=2)[0] == ARG
    assert pack([p], n=0)[0] == ARG and pack([p], n=-1)[0] == ARG
    assert pack([p, q], out=None)[0] == ARG
    assert pack([p, q], nbytes=2 * row - 1)[0] == ARG
    assert b"vti_measure_cameras_bytes" in L.vti_last_error(eng._ctx)
    arr = (vti_amd._lib.VtiCheckerParams * 1)(p.to_c())
    buf = (C.c_uint8 * row)()
    assert L.vti_checker_pack_cameras(None, arr, 1, buf, row) == 0 and bytes(buf) == a[:row]      # a NULL ctx only loses the text
    # Engine.pack_checker_cameras: the same packer
    with pytest.raises(ValueError):
        eng.pack_checker_cameras([])
    with pytest.raises(vti_amd.VtiError, match="camera 1"):
        eng.pack_checker_cameras([p, dc.replace(p, min_stitches=0)], device="cpu")
    t = eng.pack_checker_cameras([p, q, p], device="cpu")
    assert bytes(t.numpy()) == a


def test_the_measure_calls_check_every_argument_before_any_hip_call(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    eng = vti_amd.Engine("n", 2, H=736, W=960, max_batch=4)
    B, max_det, cap = 4, 10, 20
    t_in, _, _ = eng.pack_frames(SHAPES, device="cpu")
    W0 = max(w for _, w in SHAPES)
    need = eng.measure_scratch_bytes(B, cap, W0)
    one, ws = C.c_void_p(4096), C.c_void_p(1 << 20)
    err = lambda: L.vti_last_error(eng._ctx)

    def cameras(ctx=eng._ctx, table=one, n_cams=3, index=one, masks=one, native=0, dets=one, B=B, max_det=max_det, cap=cap, scratch=ws,
                nbytes=need, frame_f64=one, **_):
        return L.vti_measure_checker_cameras(ctx, table, n_cams, index, masks, native, dets, one, one, one, B, max_det, cap, 1080, W0,
                                             scratch, nbytes, frame_f64, one, None, None, None)

    def frames(ctx=eng._ctx, table=one, n_cams=3, index=one, masks=one, native=0, dets=one, B=B, max_det=max_det, cap=cap, scratch=ws,
               nbytes=need, frame_f64=one, ht=_hp(t_in), dt=one):
        return L.vti_measure_checker_frames(ctx, table, n_cams, index, masks, native, dets, one, one, one, ht, dt, B, max_det, cap,
                                            scratch, nbytes, frame_f64, one, None, None, None)

    def ragged(ctx=eng._ctx, table=one, n_cams=3, index=one, masks=one, native=None, dets=one, B=B, max_det=max_det, cap=cap, scratch=ws,
               nbytes=need, frame_f64=one, ht=_hp(t_in), dt=one, bases=one, cbytes=1 << 20):
        return L.vti_measure_checker_frames_native(ctx, table, n_cams, index, masks, bases, cbytes, dets, one, one, one, ht, dt, B,
                                                   max_det, cap, scratch, nbytes, frame_f64, one, None, None, None)

    for call, fn in ((cameras, b"vti_measure_checker_cameras:"), (frames, b"vti_measure_checker_frames:"),
                     (ragged, b"vti_measure_checker_frames_native:")):
        is_native = call is ragged

        def refused(needle=b"", rc=ARG, **kw):
            got = call(**kw)
            assert got == rc and err().startswith(fn) and needle in err(), (fn, kw, got, err())

        assert call(ctx=None) == ARG
        refused(b"null ctx, camera table or camera index", table=None)
        refused(b"null ctx, camera table or camera index", index=None)
        refused(b"n_cams", n_cams=0)
        refused(b"n_cams", n_cams=-1)
        refused(b"16-byte aligned", table=C.c_void_p(4096 + 8))
        refused(b"4-byte aligned", index=C.c_void_p(4096 + 2))
        refused(b"scratch smaller than vti_measure_scratch_bytes()", nbytes=need - 1)
        refused(b"256-byte aligned", scratch=C.c_void_p((1 << 20) + 64))
        refused(b"256-byte aligned", scratch=None)
        refused(b"8-byte aligned" if is_native else b"16-byte aligned", masks=C.c_void_p(4096 + (4 if is_native else 8)))
        refused(b"null pointer", masks=None)
        refused(b"null pointer", dets=None)
        refused(b"null pointer", frame_f64=None)
        refused(b"bad shape", max_det=0)
        refused(b"bad shape", cap=-1)
        refused(b"VTI_MEASURE_MAX_DET", max_det=vti_amd._lib.VTI_MEASURE_MAX_DET + 1)      # VTI_ERR_ARG, as vti_measure_checker
        if call is cameras:
            refused(b"bad shape", B=-1)
            refused(b"bad shape", native=2)
            refused(b"8-byte aligned", native=1, masks=C.c_void_p(4096 + 4))
            assert call(B=0, cap=0, masks=None, nbytes=0, scratch=None) == 0               # nothing to do: no launch
            assert call(B=0, cap=0, masks=None, nbytes=0, scratch=None, table=None) == ARG
            continue
        # the frame table pair: revalidated row by row at the call
        refused(b"", ht=None)
        refused(b"", dt=None)
        refused(b"", dt=C.c_void_p(4096 + 8))
        refused(b"another B", B=3)
        other, _, _ = vti_amd.Engine("n", 2, H=64, W=96, max_batch=4).pack_frames(SHAPES, device="cpu")
        refused(b"another canvas", ht=_hp(other))
        corrupt = t_in.host.clone()
        corrupt[64] = 1                                                      # row 0's byte offset is no longer a multiple of 16
        refused(b"frame 0 of host_table", ht=C.c_void_p(corrupt.data_ptr()))
        if call is frames:
            refused(b"native masks need frames of one size (vti_measure_checker_cameras)", rc=UNSUPPORTED, native=1)
            refused(b"bad shape", native=2)
        else:
            refused(b"null dev_mask_bases", bases=None)
            refused(b"8-byte aligned", bases=C.c_void_p(4096 + 4))
            refused(b"capacity_bytes", cbytes=-1)
    # what IS accepted up to the device check: without a GPU the call then stops with the HIP status, never with an argument error
    for call in (cameras, frames, ragged):
        assert call() not in (ARG, UNSUPPORTED)
    # the twins they are modelled on keep their refusals
    rc = L.vti_measure_frames(eng._ctx, one, 3, one, one, 1, one, one, one, one, _hp(t_in), one, B, max_det, cap, ws, need, one, one, None,
                              None, None)
    assert rc == UNSUPPORTED and err() == b"vti_measure_frames: native masks need frames of one size (vti_measure_cameras)"


def test_the_picture_calls_check_every_argument_before_any_hip_call(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    eng = vti_amd.Engine("n", 2, H=736, W=960, max_batch=4)
    B, max_det, cap, mp = 4, 200, 800, 4096
    sel = [3, 0, 3]
    t_in, _, _ = eng.pack_frames(SHAPES, device="cpu")
    t_out, _, _ = eng.pack_frames([SHAPES[b] for b in sel], device="cpu")
    need_f = L.vti_annotate_frames_scratch_bytes(eng._ctx, _hp(t_out), max_det, mp)
    need_c = eng.annotate_scratch_bytes(3, max_det, 960, 1280, mp)
    one, ws = C.c_void_p(4096), C.c_void_p(1 << 20)
    good_sel = (C.c_int32 * 3)(*sel)
    err = lambda: L.vti_last_error(eng._ctx)

    def cameras(ctx=eng._ctx, frames=one, B=B, H0=960, W0=1280, cams=one, n_cams=2, cof=one, masks=one, native=0, dets=one, xyxy=one,
                counts=one, offsets=one, max_det=max_det, cap=cap, fi=one, sf=one, si=one, hsel=good_sel, dsel=one, n_sel=3, mp=mp,
                out=one, status=one, scratch=ws, nbytes=need_c):
        return L.vti_annotate_checker_cameras(ctx, frames, B, H0, W0, cams, n_cams, cof, masks, native, dets, xyxy, counts, offsets,
                                              max_det, cap, fi, sf, si, hsel, dsel, n_sel, mp, out, status, scratch, nbytes, None)

    def tables(ctx=eng._ctx, frames=one, ht=_hp(t_in), dt=one, B=B, cams=one, n_cams=2, cof=one, masks=one, native=0, dets=one, xyxy=one,
               counts=one, offsets=one, max_det=max_det, cap=cap, fi=one, sf=one, si=one, hsel=good_sel, dsel=one, n_sel=3, mp=mp,
               hot=_hp(t_out), dot=one, out=one, status=one, scratch=ws, nbytes=need_f):
        return L.vti_annotate_checker_frames(ctx, frames, ht, dt, B, cams, n_cams, cof, masks, native, dets, xyxy, counts, offsets, max_det,
                                             cap, fi, sf, si, hsel, dsel, n_sel, mp, hot, dot, out, status, scratch, nbytes, None)

    for call, fn in ((cameras, b"vti_annotate_checker_cameras:"), (tables, b"vti_annotate_checker_frames")):
        def refused(needle=b"", rc=ARG, **kw):
            got = call(**kw)
            assert got == rc and err().startswith(fn) and needle in err(), (fn, kw, got, err())

        assert call(ctx=None) == ARG
        for name in ("frames", "cams", "masks", "dets", "xyxy", "counts", "offsets", "fi", "sf", "si", "hsel", "dsel", "out", "status"):
            refused(b"null pointer", **{name: None})
        refused(b"256-byte aligned", scratch=None)
        refused(b"256-byte aligned", scratch=C.c_void_p((1 << 20) + 64))
        refused(b"scratch smaller", nbytes=(need_c if call is cameras else need_f) - 1)
        refused(b"bad size", n_cams=0)
        refused(b"bad size", max_det=0)
        refused(b"bad size", max_det=vti_amd._lib.VTI_MEASURE_MAX_DET + 1)
        refused(b"bad size", cap=-1)
        refused(b"bad size", mp=-1)
        refused(b"bad size", native=2)
        refused(b"host_select[1] = -1", hsel=(C.c_int32 * 3)(3, -1, 3))
        refused(b"host_select[2] = 4", hsel=(C.c_int32 * 3)(3, 0, B))
        refused(b"16-byte aligned", cams=C.c_void_p(4096 + 8))
        refused(b"4-byte aligned", cof=C.c_void_p(4096 + 2))
        refused(b"4-byte aligned", dsel=C.c_void_p(4096 + 2))
        refused(b"16-byte aligned", masks=C.c_void_p(4096 + 8))
        refused(b"misaligned", sf=C.c_void_p(4096 + 4))
        assert call(cof=None) not in (ARG, UNSUPPORTED)                      # NULL index: row 0 for every frame
        assert call(cap=0, masks=None) not in (ARG, UNSUPPORTED)
        assert call() not in (ARG, UNSUPPORTED)
    assert cameras(native=1, masks=C.c_void_p(4096 + 4)) == ARG and b"8-byte" in err()
    assert cameras(native=1) not in (ARG, UNSUPPORTED)
    assert cameras(H0=8193, nbytes=1 << 40) == ARG and b"8192" in err()
    assert cameras(n_sel=0) == ARG and cameras(B=0) == ARG
    # the table pairs, revalidated row by row; the out table against the selection
    assert tables(native=1) == UNSUPPORTED and b"native masks need frames of one size (vti_annotate_checker_cameras)" in err()
    for name in ("ht", "dt", "hot", "dot"):
        assert tables(**{name: None}) == ARG, name
    assert tables(dt=C.c_void_p(4096 + 8)) == ARG and tables(dot=C.c_void_p(4096 + 8)) == ARG
    assert tables(B=3) == ARG and b"another B" in err()
    other = vti_amd.Engine("n", 2, H=64, W=96, max_batch=4)
    assert tables(ht=_hp(other.pack_frames(SHAPES, device="cpu")[0])) == ARG and b"another canvas" in err()
    assert tables(hot=_hp(other.pack_frames([SHAPES[b] for b in sel], device="cpu")[0])) == ARG
    assert b"another canvas" in err() and err().startswith(b"vti_annotate_checker_frames (out table):")
    assert tables(n_sel=2, hsel=(C.c_int32 * 2)(3, 0)) == ARG and b"another B" in err()
    assert tables(n_sel=0) == ARG
    corrupt = t_out.host.clone()
    corrupt[64 + 64] = 1                                                     # row 1 of the out table
    assert tables(hot=C.c_void_p(corrupt.data_ptr())) == ARG and b"frame 1 of host_table" in err()
    assert tables(hsel=(C.c_int32 * 3)(3, 1, 3)) == ARG and b"row 1 of the out table" in err()
    assert tables(hsel=(C.c_int32 * 3)(3, 0, 0)) == ARG and b"row 2 of the out table" in err()
    wide = [(960, 1280), (8200, 480), (720, 960), (1080, 1920)]
    t_wide, _, _ = eng.pack_frames(wide, device="cpu")
    t_wide_out, _, _ = eng.pack_frames([wide[b] for b in (3, 1, 3)], device="cpu")
    assert tables(ht=_hp(t_wide), hot=_hp(t_wide_out), hsel=(C.c_int32 * 3)(3, 1, 3), nbytes=1 << 40) == ARG
    assert b"frame 1" in err() and b"8192" in err()
    assert tables(ht=_hp(t_wide)) not in (ARG, UNSUPPORTED)                  # ... not selected: served
    assert tables(frames=C.c_void_p(4096 + 8)) == ARG and tables(out=C.c_void_p(4096 + 8)) == ARG
    # vti_annotate_frames keeps its own refusal
    rc = L.vti_annotate_frames(eng._ctx, one, _hp(t_in), one, B, one, 2, one, one, 1, one, one, one, one, max_det, cap, one, one, one,
                               good_sel, one, 3, mp, _hp(t_out), one, one, one, ws, need_f, None)
    assert rc == UNSUPPORTED and err() == b"vti_annotate_frames: native masks need frames of one size (vti_annotate)"


def _fake_out(torch, B, max_det=8, cap=4):
    return dict(dets=torch.zeros((B, max_det, 38)), xyxy=torch.zeros((B, max_det, 4)), counts=torch.zeros(B, dtype=torch.int32),
                offsets=torch.zeros(B + 1, dtype=torch.int32), masks=torch.zeros((cap, 64, 8), dtype=torch.uint8))


def test_engine_refuses_bad_input_before_it_touches_a_device(lib_built):
    import torch
    vti_amd = lib_built
    eng = vti_amd.Engine("n", 2, H=64, W=64, max_batch=2)
    out = _fake_out(torch, 2)
    p = vti_amd.CheckerParams(*CALIB)
    row = int(vti_amd.lib().vti_measure_cameras_bytes(1))
    table = torch.zeros(3 * row, dtype=torch.uint8)
    for params in (table, [p, p, p]):
        for cams in ([0, 3], [-1, 0], [0], [0, 1, 2], [0.5, 1.0]):             # out of range; lengths that differ; no integers
            with pytest.raises(ValueError, match="cameras|camera index"):
                eng.measure_checker(out, params, 48, 64, cameras=cams)
    with pytest.raises(ValueError, match="pack_checker_cameras"):
        eng.measure_checker(out, table[:row + 1], 48, 64, cameras=[0, 0])
    with pytest.raises(ValueError, match="H0 and W0"):
        eng.measure_checker(out, p)
    ft, _, total = eng.pack_frames([(48, 64), (32, 40)], device="cpu")
    with pytest.raises(ValueError, match="not both"):
        eng.measure_checker(out, table, 48, 64, cameras=[0, 0], frames=ft)
    with pytest.raises(ValueError, match="mask_bases"):                       # native=True needs the ragged set
        eng.measure_checker(out, table, cameras=[0, 0], frames=ft, native=True)
    with pytest.raises(ValueError, match="describes 2 frames"):
        eng.measure_checker(_fake_out(torch, 3), table, cameras=[0, 0, 0], frames=ft)
    # the picture
    meas = dict(frame_i32=torch.zeros((2, 6), dtype=torch.int32), stitch_f64=torch.zeros((4, 7), dtype=torch.float64),
                stitch_i32=torch.zeros((4, 2), dtype=torch.int32))
    frames = torch.zeros((2, 48, 64, 3), dtype=torch.uint8)
    buf = torch.zeros(total, dtype=torch.uint8)
    with pytest.raises(ValueError, match="camera index"):
        eng.annotate_checker(frames, out, meas, [p, p], [0], cameras=[0, 2])
    with pytest.raises(ValueError, match="cameras must be 2 integers"):
        eng.annotate_checker(frames, out, meas, [p, p], [0], cameras=[0])
    with pytest.raises(ValueError, match="flat uint8"):
        eng.annotate_checker(frames, out, meas, [p], [0], table=ft)
    with pytest.raises(ValueError, match="native"):
        eng.annotate_checker(buf, out, meas, [p], [0], table=ft, native=True)
    with pytest.raises(ValueError, match="frame index"):
        eng.annotate_checker(buf, out, meas, [p], [2], table=ft)
    with pytest.raises(ValueError, match="device batch"):                      # a good call on host memory stops at the device check
        eng.annotate_checker(buf, out, meas, [p], [1, 0], table=ft, cameras=[0, 0])
    with pytest.raises(ValueError, match="device batch"):
        eng.annotate_checker(frames, out, meas, [p, p], [0], cameras=[0, 1])


def test_multi_camera_checker_refuses_bad_input_before_it_predicts(lib_built, monkeypatch):
    import inspect
    vti_amd = lib_built
    model = vti_amd.YOLO(None, scale="n", nc=2, seed=3)
    p = vti_amd.CheckerParams(*CALIB)
    mc = vti_amd.MultiCameraChecker(model, [p, dc.replace(p, min_stitches=2)])
    with pytest.raises(ValueError, match="at least one camera"):
        vti_amd.MultiCameraChecker(model, [])
    frames = np.zeros((3, 48, 64, 3), np.uint8)
    mixed = [frames[0], np.zeros((32, 64, 3), np.uint8), frames[1]]

    def no_predict(*a, **k):
        raise AssertionError("predict was reached")
    monkeypatch.setattr(model, "_predict_outputs", no_predict)
    monkeypatch.setattr(model, "_predict_outputs_frames", no_predict)
    with pytest.raises(ValueError, match="camera index outside"):
        mc.process_frames(frames, [0, 1, 2])
    with pytest.raises(ValueError, match="camera index outside"):
        mc.process_frames(mixed, [0, -1, 0])
    with pytest.raises(ValueError, match="3 frames but 2 cameras"):
        mc.process_frames(frames, [0, 1])
    with pytest.raises(ValueError, match="3 frames but 4 cameras"):
        mc.process_frames(mixed, [0, 1, 0, 1])
    with pytest.raises(ValueError, match="integers"):
        mc.process_frames(frames, [0.0, 1.0, 0.5])
    with pytest.raises(ValueError, match="annotate needs frames of one size"):
        mc.process_frames(mixed, [0, 1, 0], annotate="all")
    with pytest.raises(ValueError, match="retina_masks=True needs frames of one size"):
        mc.process_frames(mixed, [0, 1, 0], retina_masks=True)
    with pytest.raises(ValueError, match="retina_masks=True needs frames of one size"):
        mc.process_frames(mixed, [0, 1, 0], retina_masks=True, annotate="all", mixed=True)
    with pytest.raises(ValueError, match="encode needs annotate"):
        mc.process_frames(frames, [0, 1, 0], encode="jpeg")
    with pytest.raises(ValueError, match="encode needs annotate"):
        mc.process_frames(mixed, [0, 1, 0], encode="jpeg", mixed=True)
    with pytest.raises(ValueError, match='encode must be None or "jpeg"'):
        mc.process_frames(frames, [0, 1, 0], annotate="all", encode="png")
    with pytest.raises(ValueError, match="extra_text needs burn_text"):
        mc.process_frames(frames, [0, 1, 0], annotate="all", extra_text={0: []})
    sig = inspect.signature(vti_amd.MultiCameraChecker.process_frames)
    assert list(sig.parameters) == ["self", "frames", "cameras", "conf", "iou", "max_det", "imgsz", "retina_masks", "rows", "annotate",
                                    "encode", "jpeg_quality", "mixed", "burn_text", "extra_text", "rasterise"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[3:]] == [0.20, 0.45, 200, 640, False, False, None, None, 95, False,
                                                                            False, None, None]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("mixed", "burn_text", "extra_text", "rasterise"))
    # StitchDistanceChecker keeps its refusal of a mixed list
    ck = vti_amd.StitchDistanceChecker(model, p)
    with pytest.raises(ValueError, match="needs frames of one size"):
        ck.process_frames(mixed)


def test_every_camera_keeps_its_own_pair_of_deques(lib_built, monkeypatch):
    """_frame_records stubbed to canned (f64, i32): the records are those of one StitchDistanceChecker per camera that only ever sees
    its own frames, in the same order, with a `camera` key added."""
    vti_amd = lib_built
    fb = 3
    p = vti_amd.CheckerParams(*CALIB)
    params = [p, dc.replace(p, min_stitches=5), dc.replace(p, min_stitches=1)]
    model = types.SimpleNamespace(drop_empty_masks=True)
    mc = vti_amd.MultiCameraChecker(model, params, frame_buffer=fb)
    assert all(x.drop_empty and x.frame_buffer == fb for x in mc.params)
    singles = [vti_amd.StitchDistanceChecker(model, x, frame_buffer=fb) for x in params]
    rng = np.random.default_rng(5)
    canned = {}
    for who in [mc] + singles:
        monkeypatch.setattr(who, "_frame_records", lambda frames, *a, **k: canned[id(frames)])
    seen = 0
    for _ in range(12):
        B = int(rng.integers(1, 9))
        cams = rng.integers(0, len(params), B)
        f64 = np.where(rng.uniform(size=(B, 2)) < 0.3, np.nan, rng.uniform(1, 15, (B, 2)))
        i32 = np.stack([rng.choice([0, 0, 0, 1, 2, 3], B), np.full(B, 5), np.ones(B, int), np.full(B, 4), rng.integers(0, 9, B),
                        rng.integers(0, 9, B)], 1).astype(np.int32)
        frames = np.zeros((B, 8, 8, 3), np.uint8)
        canned[id(frames)] = (f64, i32)
        got = mc.process_frames(frames, cams)
        assert [g["camera"] for g in got] == cams.tolist()
        for c in range(len(params)):
            mine = np.flatnonzero(cams == c)
            if not mine.size:
                continue
            sub = np.zeros((mine.size, 8, 8, 3), np.uint8)
            canned[id(sub)] = (f64[mine], i32[mine])
            one = singles[c].process_frames(sub)
            for b, e in zip(mine, one):
                g = got[b]
                assert {k: v for k, v in g.items() if k not in ("timestamp", "camera")} == {k: v for k, v in e.items() if k != "timestamp"}
                seen += g["edge_distance_mm"] is not None
    assert seen >= 10
    assert [(len(d), len(w)) for d, w in mc.buffers] == [(len(s.frame_buf_dist), len(s.frame_buf_width)) for s in singles]


def test_the_refusals_run_clean_in_a_stand_alone_program_under_the_host_sanitizers(lib_built, tmp_path):
    """tests/checker_rig_args_main.cpp: its own main, built with -fsanitize=address,undefined, linked against libvti.so and run
    directly (nothing is loaded into Python, nothing is preloaded).  Every call it makes is refused before the first HIP call."""
    vti_amd = lib_built
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    lib_dir = os.path.dirname(vti_amd.LIB_PATH)
    exe = str(tmp_path / "checker_rig_args_main")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx).startswith("g++") else []    # no link-order rule to meet
    subprocess.run([cxx, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static, "-I",
                    os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "checker_rig_args_main.cpp"), "-L", lib_dir, "-lvti",
                    "-Wl,-rpath," + lib_dir, "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and re.fullmatch(r"ok \d+\n", run.stdout) and run.stderr == "", (run.returncode, run.stdout, run.stderr)
    assert int(run.stdout.split()[1]) >= 60
