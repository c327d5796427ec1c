"""vti_mask_polygons_frames without a GPU: the two entry points are declared with their marker, exported and bound with the
documented argument lists; the scratch query; every argument check comes before the first HIP call (fake pointers, never
dereferenced; without a GPU a call that gets past them ends with the HIP status instead); Engine and YOLO.predict refuse bad input
before they touch a device; and the stand-alone program tests/polygons_frames_args_main.cpp repeats the refusals clean under the
host sanitizers.  The GPU parity tests are in test_gpu_polygons_frames.py."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vti_mask_polygons_frames_scratch_bytes", "vti_mask_polygons_frames")
SHAPES = [(960, 1280), (481, 333), (720, 960), (1080, 1920)]
ARG = -1


def _hp(t):
    return C.c_void_p(t.host.data_ptr())


def _args(hdr, name):
    decl = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, hdr).group(1)
    return [" ".join(a.split()) for a in decl.split(",")]


def test_the_two_entry_points_are_declared_with_the_marker_exported_and_bound(lib_built):
    vti_amd = lib_built
    hdr = open(os.path.join(ROOT, "include", "vti.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", vti_amd.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert re.search(r"^#define VTI_POLYGONS_FRAMES_API$", hdr, re.M)
    marked = re.findall(r"^VTI_POLYGONS_FRAMES_API (?:int32_t|int64_t)\s+(vti_\w+)\s*\(", hdr, re.M)
    assert tuple(marked) == NAMES
    assert hdr.index("#define VTI_POLYGONS_FRAMES_API") > hdr.index("int32_t vti_mask_polygons(")      # the section after vti_mask_polygons
    for name in NAMES:
        assert re.search(r"\bT %s$" % name, exported, re.M), name
    assert _args(hdr, NAMES[0]) == ["const vti_ctx* ctx", "const void* host_table", "int32_t native"]
    assert _args(hdr, NAMES[1]) == ["vti_ctx* ctx", "const uint8_t* dev_masks", "int32_t native", "const int64_t* dev_mask_bases",
                                    "int64_t capacity_bytes", "const int32_t* dev_offsets", "const void* host_table",
                                    "const void* dev_table", "int32_t B", "int32_t capacity", "int32_t strategy", "void* dev_scratch",
                                    "size_t scratch_bytes", "int32_t* dev_point_offsets", "float* dev_points", "int64_t max_points",
                                    "void* stream"]
    P, I32, I64 = C.c_void_p, C.c_int32, C.c_int64
    assert vti_amd.SIGNATURES[NAMES[0]] == (I64, [P, P, I32])
    assert vti_amd.SIGNATURES[NAMES[1]] == (I32, [P, P, I32, P, I64, P, P, P, I32, I32, I32, P, C.c_size_t, P, P, I64, P])
    assert callable(vti_amd.Engine.mask_polygons_frames) and callable(vti_amd.Engine.mask_polygons_frames_scratch_bytes)
    sig = inspect.signature(vti_amd.Engine.mask_polygons_frames)
    assert list(sig.parameters) == ["self", "out", "table", "native", "strategy"]
    assert sig.parameters["native"].default is False and sig.parameters["strategy"].default == "largest"
    sig = inspect.signature(vti_amd.YOLO.predict)
    names = list(sig.parameters)
    assert sig.parameters["polygons"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["polygons"].default is False
    assert names.index("polygons") == len(names) - 2 and sig.parameters[names[-1]].kind is inspect.Parameter.VAR_KEYWORD
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "and the two polygon calls for a frame table, marked `VTI_POLYGONS_FRAMES_API`" in readme
    assert all(name in readme for name in NAMES[1:])


def test_the_scratch_query(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    eng = vti_amd.Engine("n", 2, H=736, W=960, max_batch=4)
    t, _, _ = eng.pack_frames(SHAPES, device="cpu")
    q = lambda table, native, ctx=eng._ctx: L.vti_mask_polygons_frames_scratch_bytes(ctx, table, native)
    # letterbox masks: every slot has the canvas' geometry
    assert q(_hp(t), 0) == eng.mask_polygons_scratch_bytes(736, 960, 120) == eng.mask_polygons_frames_scratch_bytes(t, False)
    # native rows: the largest frame of the table; 1080 x 1920 needs the scratch form (1080 * 30 * 8 B > 156 KiB) and every part of it
    # is the largest here
    per = [eng.mask_polygons_scratch_bytes(h, w, 8 * ((w + 63) // 64)) for h, w in SHAPES]
    assert q(_hp(t), 1) == max(per) == per[3] == eng.mask_polygons_frames_scratch_bytes(t, True)
    small, _, _ = eng.pack_frames(SHAPES[:3], device="cpu")
    assert q(_hp(small), 1) == max(per[:3]) == per[0]                         # all in LDS: no image part
    assert per[0] == 256 + 128 * (2 * 4 * 960 * 640 + ((4 * 961 + 255) & ~255))
    # each part of an area is the largest any frame needs: 4000 x 64 has the most rows, 960 x 1280 the most runs, neither an image part
    odd, _, _ = eng.pack_frames([(960, 1280), (4000, 64)], device="cpu")
    assert q(_hp(odd), 1) == 256 + 128 * (2 * 4 * 960 * 640 + ((4 * 4001 + 255) & ~255))
    order, _, _ = eng.pack_frames(SHAPES[::-1], device="cpu")
    assert q(_hp(order), 1) == q(_hp(t), 1)                                   # the order of the frames does not matter
    # 0: NULL, native outside {0, 1}, junk, a table of another canvas, a native frame above 2^26 pixels
    assert q(None, 0) == 0 and q(_hp(t), 0, ctx=None) == 0
    assert q(_hp(t), 2) == 0 and q(_hp(t), -1) == 0
    junk = (C.c_uint8 * t.host.numel())(*([0xA5] * t.host.numel()))
    assert q(junk, 0) == 0 and q(junk, 1) == 0
    other = vti_amd.Engine("n", 2, H=64, W=96, max_batch=4)
    assert q(_hp(other.pack_frames(SHAPES, device="cpu")[0]), 0) == 0
    big, _, _ = eng.pack_frames([(960, 1280), (8200, 8200)], device="cpu")    # the table allows it, vti_mask_polygons does not
    assert q(_hp(big), 1) == 0 and q(_hp(big), 0) == q(_hp(t), 0)
    one_too_many = vti_amd.Engine("n", 2, H=736, W=960, max_batch=3)
    assert L.vti_mask_polygons_frames_scratch_bytes(one_too_many._ctx, _hp(t), 0) == 0      # B above max_batch


def test_every_argument_check_comes_before_any_hip_call(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    eng = vti_amd.Engine("n", 2, H=736, W=960, max_batch=4)
    B, cap = 4, 20
    t, _, _ = eng.pack_frames(SHAPES, device="cpu")
    need = {0: eng.mask_polygons_frames_scratch_bytes(t, False), 1: eng.mask_polygons_frames_scratch_bytes(t, True)}
    one, ws = C.c_void_p(4096), C.c_void_p(1 << 20)
    err = lambda: L.vti_last_error(eng._ctx)
    fn = b"vti_mask_polygons_frames:"

    def call(ctx=eng._ctx, masks=one, native=0, bases="auto", cbytes=1 << 20, offsets=one, ht=_hp(t), dt=one, B=B, cap=cap, strategy=0,
             scratch=ws, nbytes=None, po=one, points=one, mp=100):
        if bases == "auto":
            bases = one if native == 1 else None
        return L.vti_mask_polygons_frames(ctx, masks, native, bases, cbytes, offsets, ht, dt, B, cap, strategy, scratch,
                                          need.get(native, need[0]) if nbytes is None else nbytes, po, points, mp, None)

    def refused(needle=b"", **kw):
        got = call(**kw)
        assert got == ARG and err().startswith(fn) and needle in err(), (kw, got, err())

    assert call(ctx=None) == ARG
    for native in (0, 1):
        refused(b"null pointer", native=native, masks=None)
        refused(b"null pointer", native=native, offsets=None)
        refused(b"null pointer", native=native, po=None)
        refused(b"null pointer", native=native, points=None)
        refused(b"capacity_bytes", native=native, cbytes=-1)
        refused(b"capacity and max_points", native=native, cap=-1)
        refused(b"capacity and max_points", native=native, mp=-1)
        refused(b"strategy", native=native, strategy=2)
        refused(b"strategy", native=native, strategy=-1)
        refused(b"another B", native=native, B=0)
        refused(b"another B", native=native, B=-1)
        refused(b"another B", native=native, B=3)
        refused(b"scratch smaller than vti_mask_polygons_frames_scratch_bytes()", native=native, nbytes=need[native] - 1)
        refused(b"256-byte aligned", native=native, scratch=C.c_void_p((1 << 20) + 64))
        refused(b"256-byte aligned", native=native, scratch=None)
        refused(b"4-byte aligned", native=native, offsets=C.c_void_p(4096 + 2))
        refused(b"4-byte aligned", native=native, po=C.c_void_p(4096 + 2))
        refused(b"4-byte aligned", native=native, points=C.c_void_p(4096 + 2))
        # the frame table pair: revalidated row by row at the call
        refused(b"null frame table", native=native, ht=None)
        refused(b"null frame table", native=native, dt=None)
        refused(b"16-byte aligned", native=native, dt=C.c_void_p(4096 + 8))
        other = vti_amd.Engine("n", 2, H=64, W=96, max_batch=4).pack_frames(SHAPES, device="cpu")[0]
        refused(b"another canvas", native=native, ht=_hp(other))
        corrupt = t.host.clone()
        corrupt[64 + 64] = 1                                                   # row 1's byte offset is no longer a multiple of 16
        refused(b"frame 1 of host_table", native=native, ht=C.c_void_p(corrupt.data_ptr()))
        junk = (C.c_uint8 * t.host.numel())(*([0xA5] * t.host.numel()))
        refused(b"not a table of vti_pack_frames", native=native, ht=junk)
        # what IS accepted up to the device check: without a GPU the call then stops with the HIP status, never an argument error
        assert call(native=native) != ARG
        assert call(native=native, cap=0, masks=None) != ARG                   # no slots: dev_masks may be NULL
        assert call(native=native, mp=0, points=None) != ARG
        assert call(native=native, strategy=1) != ARG
    refused(b"native must be 0 or 1", native=2)
    refused(b"native must be 0 or 1", native=-1)
    refused(b"dev_mask_bases must be NULL with native = 0", native=0, bases=one)
    refused(b"null dev_mask_bases", native=1, bases=None)
    refused(b"16-byte aligned", native=0, masks=C.c_void_p(4096 + 8))
    refused(b"8-byte aligned", native=1, masks=C.c_void_p(4096 + 4))
    assert call(native=1, masks=C.c_void_p(4096 + 8)) != ARG
    refused(b"dev_mask_bases must be 8-byte aligned", native=1, bases=C.c_void_p(4096 + 4))
    big, _, _ = eng.pack_frames([(960, 1280), (481, 333), (8200, 8200), (1080, 1920)], device="cpu")
    refused(b"frame 2 of host_table: H0 * W0 above 2^26", native=1, ht=_hp(big), nbytes=1 << 40)
    assert call(native=0, ht=_hp(big)) != ARG                                  # letterbox masks are traced at the canvas size
    small = vti_amd.Engine("n", 2, H=736, W=960, max_batch=3)
    assert L.vti_mask_polygons_frames(small._ctx, one, 0, None, 0, one, _hp(t), one, 4, cap, 0, ws, need[0], one, one, 100, None) == ARG
    assert b"B above max_batch" in L.vti_last_error(small._ctx)


def _fake_out(torch, B, max_det=8, cap=4, H=64, W=64):
    return dict(dets=torch.zeros((B, max_det, 38)), xyxy=torch.zeros((B, max_det, 4)), counts=torch.zeros(B, dtype=torch.int32),
                offsets=torch.zeros(B + 1, dtype=torch.int32), masks=torch.zeros((cap, H, W // 8), dtype=torch.uint8))


def test_engine_refuses_bad_input_before_it_touches_a_device(lib_built):
    import torch
    vti_amd = lib_built
    eng = vti_amd.Engine("n", 2, H=64, W=64, max_batch=2)
    ft, _, _ = eng.pack_frames([(48, 64), (32, 40)], device="cpu")
    out = _fake_out(torch, 2)
    with pytest.raises(ValueError, match="strategy"):
        eng.mask_polygons_frames(out, ft, strategy="all")
    with pytest.raises(ValueError, match=r"mask_polygons_frames: native masks for frames of differing sizes need "
                                         r"alloc_outputs\(\.\.\., native_frames=table\)"):       # _check_ragged's wording
        eng.mask_polygons_frames(out, ft, native=True)
    ragged = dict(out, masks=torch.zeros(1024, dtype=torch.uint8), mask_bases=torch.zeros(3, dtype=torch.int64),
                  native_shapes=((48, 64), (32, 48)))
    with pytest.raises(ValueError, match="other frame shapes"):
        eng.mask_polygons_frames(ragged, ft, native=True)
    with pytest.raises(ValueError, match="describes 2 frames"):
        eng.mask_polygons_frames(_fake_out(torch, 3), ft)
    with pytest.raises(ValueError, match="FrameTable"):
        eng.mask_polygons_frames(out, None)
    with pytest.raises(ValueError, match="letterbox bit masks"):
        eng.mask_polygons_frames(_fake_out(torch, 2, H=48), ft)
    other = vti_amd.Engine("n", 2, H=64, W=96, max_batch=2)
    with pytest.raises(ValueError, match="canvas"):
        other.mask_polygons_frames(_fake_out(torch, 2, W=96), ft)
    with pytest.raises(ValueError, match="FrameTable"):
        eng.mask_polygons_frames_scratch_bytes(None, False)


@pytest.mark.parametrize("value", ["yes", 1, 0, None])
def test_predict_refuses_a_polygons_value_that_is_no_bool_before_it_predicts(lib_built, monkeypatch, value):
    vti_amd = lib_built
    model = vti_amd.YOLO(None, scale="n", nc=2, seed=3)

    def no_predict(*a, **k):
        raise AssertionError("predict was reached")
    monkeypatch.setattr(model, "_predict_outputs", no_predict)
    monkeypatch.setattr(model, "_predict_outputs_frames", no_predict)
    frames = np.zeros((2, 48, 64, 3), np.uint8)
    mixed = [frames[0], np.zeros((32, 64, 3), np.uint8)]
    for source in (frames, mixed):
        with pytest.raises(ValueError, match="polygons must be True or False"):
            model.predict(source, polygons=value)
    with pytest.raises(AssertionError, match="predict was reached"):           # a bool passes the check
        model.predict(frames, polygons=True)


def test_the_refusals_run_clean_in_a_stand_alone_program_under_the_host_sanitizers(lib_built, tmp_path):
    """tests/polygons_frames_args_main.cpp: its own main, built with -fsanitize=address,undefined, linked against libvti.so and run
    directly (nothing is loaded into Python, nothing is preloaded).  Every call it makes is refused before the first HIP call."""
    vti_amd = lib_built
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    lib_dir = os.path.dirname(vti_amd.LIB_PATH)
    exe = str(tmp_path / "polygons_frames_args_main")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx).startswith("g++") else []    # no link-order rule to meet
    subprocess.run([cxx, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static, "-I",
                    os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "polygons_frames_args_main.cpp"), "-L", lib_dir, "-lvti",
                    "-Wl,-rpath," + lib_dir, "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and re.fullmatch(r"ok \d+\n", run.stdout) and run.stderr == "", (run.returncode, run.stdout, run.stderr)
    assert int(run.stdout.split()[1]) >= 40
