"""Predict on a window of each frame, without a GPU: the entry points are declared with their marker, exported and bound; the packer
refuses every bad window and names the first failing frame, is deterministic, and a whole-frame row is the frame table's row; the
bytes query equals the frames query; every *_windows call refuses bad arguments before a device is touched (fake pointers, never
dereferenced); the Python surface raises ValueError before an engine exists; and the stand-alone program tests/windows_args_main.cpp
repeats the refusals clean under the host sanitizers.  The GPU parity tests are in test_gpu_windows.py."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from test_oracle_geometry import load_calib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vti_window_table_bytes", "vti_pack_windows", "vti_window_table_info", "vti_letterbox_windows", "vti_scale_boxes_windows",
         "vti_mask_native_windows_bytes", "vti_masks_native_windows", "vti_predict_windows")
ARG, STATE, UNSUPPORTED = -1, -2, -6
SHAPES = [(140, 200), (135, 241), (480, 640)]
GOOD = [(3, 5, 131, 97), (0, 0, 241, 135), (639, 479, 1, 1)]


def test_the_entry_points_are_declared_with_the_marker_exported_and_bound(lib_built):
    vti_amd = lib_built
    hdr = open(os.path.join(ROOT, "include", "vti.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", vti_amd.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert re.search(r"^#define VTI_WINDOWS_API$", hdr, re.M)
    marked = re.findall(r"^VTI_WINDOWS_API (?:int32_t|int64_t)\s+(vti_\w+)\s*\(", hdr, re.M)
    assert tuple(marked) == NAMES
    assert sorted(n for n in vti_amd.SIGNATURES if n.endswith("_windows") or "_window_" in n or "_windows_" in n) == sorted(NAMES)
    assert sorted(set(re.findall(r"\bT (vti_\w*window\w*)$", exported, re.M))) == sorted(NAMES)
    for name in NAMES:
        assert hasattr(vti_amd.lib(), name)
    S, P, I32, I64 = vti_amd.SIGNATURES, C.c_void_p, C.c_int32, C.c_int64
    assert S["vti_window_table_bytes"] == (I64, [I32])
    assert S["vti_pack_windows"] == (I32, [P, I32, I32, P, P, P, P, I32, I64, P, C.c_size_t])
    assert S["vti_letterbox_windows"] == S["vti_letterbox_frames"] and S["vti_scale_boxes_windows"] == S["vti_scale_boxes_frames"]
    assert S["vti_mask_native_windows_bytes"] == S["vti_mask_native_frames_bytes"]
    assert S["vti_predict_windows"] == S["vti_predict_frames_native"]
    res, args = S["vti_masks_native_windows"]
    assert res is I32 and len(args) == 15 and args[11] is I64                      # vti_masks_native_frames' without dev_xyxy
    decl = lambda name: [" ".join(a.split()) for a in re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, hdr).group(1).split(",")]
    assert len(decl("vti_predict_windows")) == 23 and len(decl("vti_masks_native_windows")) == 15 and len(decl("vti_pack_windows")) == 11
    assert decl("vti_pack_windows")[6] == "const int32_t* windows"
    assert "WindowTable" in vti_amd.__all__ and hasattr(vti_amd, "WindowTable")
    for meth in ("pack_windows", "letterbox_windows", "scale_boxes_windows", "mask_native_windows_bytes", "masks_native_windows",
                 "predict_windows_into"):
        assert callable(getattr(vti_amd.Engine, meth)), meth
    sig = inspect.signature(vti_amd.YOLO.predict)
    assert sig.parameters["window"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["window"].default is None
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "VTI_WINDOWS_API" in readme and "vti_predict_windows" in readme


def _pack(vti_amd, eng, windows, shapes=SHAPES, short=0, ctx=True, null=None, B=None, H=None, W=None):
    """-> (rc, message, bytes); the frames lie back to back at multiples of 16 as pack_frames puts them."""
    L = vti_amd.lib()
    n = len(shapes)
    offs, total = [], 0
    for h, w in shapes:
        offs.append(total)
        total = (total + 3 * h * w + 15) & ~15
    arrs = dict(H0=(C.c_int32 * n)(*[h for h, _ in shapes]), W0=(C.c_int32 * n)(*[w for _, w in shapes]), off=(C.c_int64 * n)(*offs),
                win=(C.c_int32 * (4 * n))(*[v for w in windows for v in w]))
    nbytes = int(L.vti_window_table_bytes(n))
    buf = (C.c_uint8 * nbytes)(*([0x5A] * nbytes))
    arrs["table"] = buf
    if null:
        arrs[null] = None
    c = eng._ctx if ctx else None
    rc = L.vti_pack_windows(c, eng.H if H is None else H, eng.W if W is None else W, arrs["H0"], arrs["W0"], arrs["off"], arrs["win"],
                            n if B is None else B, total, arrs["table"], nbytes - short)
    return rc, (L.vti_last_error(c) or b"").decode(), bytes(buf)


def test_the_packer_refuses_every_bad_window_and_names_the_first_failing_frame(lib_built):
    vti_amd = lib_built
    eng = vti_amd.Engine("n", 2, H=64, W=96, max_batch=4)
    rc, msg, good = _pack(vti_amd, eng, GOOD)
    assert rc == 0, msg
    cases = [(0, (70, 5, 131, 97), "inside its frame"), (0, (3, 44, 131, 97), "inside its frame"),          # past the right / bottom edge
             (1, (-1, 0, 241, 135), "inside its frame"), (2, (0, -1, 1, 1), "inside its frame"),
             (1, (241, 0, 1, 1), "inside its frame"), (2, (639, 479, 2, 1), "inside its frame"),
             (0, (3, 5, 0, 97), ">= 1"), (1, (0, 0, 241, 0), ">= 1"), (2, (0, 0, -4, 1), ">= 1"),           # w < 1, h < 1
             (2, (0, 0, 640, 1), "below 1 px"), (0, (0, 0, 1, 140), "below 1 px"),                            # resized below 1 px
             (1, (0, 0, 1 << 30, 1 << 30), "inside its frame")]
    for frame, w, needle in cases:
        windows = list(GOOD)
        windows[frame] = w
        rc, msg, _ = _pack(vti_amd, eng, windows)
        assert rc == ARG and re.match(r"vti_pack_windows: frame %d: .*%s" % (frame, needle), msg), (frame, w, rc, msg)
    windows = [GOOD[0], (0, 0, 0, 1), (0, 0, 1, 0)]
    assert "frame 1:" in _pack(vti_amd, eng, windows)[1]                        # the FIRST failing frame is the one named
    for kw, needle in ((dict(short=1), "smaller than"), (dict(null="table"), "null"), (dict(null="win"), "null"), (dict(null="H0"), "null"),
                       (dict(null="W0"), "null"), (dict(null="off"), "null"), (dict(B=0), "B < 1"), (dict(B=-2), "B < 1"),
                       (dict(H=60), "multiples of 32"), (dict(W=0), "multiples of 32")):
        rc, msg, _ = _pack(vti_amd, eng, GOOD, **kw)
        assert rc == ARG and msg.startswith("vti_pack_windows:") and needle in msg, (kw, rc, msg)
    # vti_pack_frames' checks of the frames come with it
    rc, msg, _ = _pack(vti_amd, eng, [(0, 0, 1, 1)] * 2, shapes=[(140, 200), (0, 5)])
    assert rc == ARG and "frame 1: H0 and W0 must be >= 1" in msg
    rc, msg, _ = _pack(vti_amd, eng, [(0, 0, 1, 1)], shapes=[(20000, 8)])
    assert rc == ARG and "frame 0:" in msg and "16384" in msg
    assert _pack(vti_amd, eng, GOOD, ctx=False)[0] == 0                        # ctx only receives the text
    assert _pack(vti_amd, eng, [(0, 0, 1, 1)] * 3, ctx=False)[0] == 0          # upscaled single pixels are fine
    # B > max_batch: refused with a ctx; without one the table packs (as a frame table does) and every device call refuses it
    big = [(64, 96)] * 5
    rc, msg, _ = _pack(vti_amd, eng, [(0, 0, 96, 64)] * 5, shapes=big)
    assert rc == ARG and msg == "vti_pack_windows: B above the ctx's max_batch", msg
    assert _pack(vti_amd, eng, [(0, 0, 96, 64)] * 4, shapes=big[:4])[0] == 0
    rc, msg, tab = _pack(vti_amd, eng, [(0, 0, 96, 64)] * 5, shapes=big, ctx=False)
    assert rc == 0, msg
    L = vti_amd.lib()
    one = C.c_void_p(4096)
    host = (C.c_uint8 * len(tab)).from_buffer_copy(tab)
    assert L.vti_letterbox_windows(eng._ctx, one, host, one, 5, one, None) == ARG and b"max_batch" in L.vti_last_error(eng._ctx)
    assert L.vti_predict_windows(eng._ctx, one, host, one, 5, 0, 0.25, 0.7, 10, 0, 0, 1, one, one, one, one, one, one, 1 << 16, one, one,
                                 one, None) == ARG
    assert L.vti_mask_native_windows_bytes(eng._ctx, host, 5) == 0
    with pytest.raises(vti_amd.VtiError, match="frame 2: the window does not lie inside its frame"):
        eng.pack_windows(SHAPES, [GOOD[0], GOOD[1], (639, 479, 2, 2)], device="cpu")
    with pytest.raises(ValueError, match="one .x0, y0, w, h. per frame"):
        eng.pack_windows(SHAPES, GOOD[:2], device="cpu")


def test_pack_is_deterministic_and_a_whole_frame_row_is_the_frame_tables_row(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    eng = vti_amd.Engine("n", 2, H=64, W=96, max_batch=4)
    a, b = _pack(vti_amd, eng, GOOD)[2], _pack(vti_amd, eng, GOOD)[2]
    assert a == b and 0x5A not in set(a)                                       # every byte of the table is written
    assert _pack(vti_amd, eng, [GOOD[0], GOOD[1], (638, 479, 1, 1)])[2] != a
    wt = eng.pack_windows(SHAPES, GOOD, device="cpu")
    assert isinstance(wt, vti_amd.WindowTable) and bytes(wt.host.numpy()) == a and wt.B == 3 and wt.windows == GOOD
    assert wt.frames.shapes == SHAPES and (wt.H, wt.W) == (64, 96)
    whole = eng.pack_windows(SHAPES, [(0, 0, w, h) for h, w in SHAPES], device="cpu")
    for k in range(3):
        row, ref = whole.row(k), whole.frames.row(k)
        assert {key: row[key] for key in ref} == ref                            # the geometry vti_frame_table_info reports
        assert (row["x0"], row["y0"], row["frame_H0"], row["frame_W0"]) == (0, 0) + SHAPES[k]
    crops = [(h, w) for _, _, w, h in GOOD]
    ct, _, _ = eng.pack_frames(crops, device="cpu")
    for k, (x0, y0, w, h) in enumerate(GOOD):                                   # a proper window's row is the crop's, but for the offset
        row, ref = wt.row(k), ct.row(k)
        assert {key: row[key] for key in ref if key != "offset"} == {key: ref[key] for key in ref if key != "offset"}
        assert row["offset"] == wt.frames.byte_offsets[k] + 3 * (y0 * SHAPES[k][1] + x0)
        assert (row["x0"], row["y0"], row["frame_H0"], row["frame_W0"]) == (x0, y0) + SHAPES[k]
    i32 = (C.c_int32 * 12)()
    host = C.c_void_p(wt.host.data_ptr())
    assert L.vti_window_table_info(host, -1, i32, None) == 0 and list(i32[:5]) == [3, 64, 96, 480, 640]
    assert (i32[6] & 0xFFFFFFFF) | (i32[7] << 32) == wt.total_bytes
    assert L.vti_window_table_info(host, 3, i32, None) == ARG and L.vti_window_table_info(host, -2, i32, None) == ARG
    assert L.vti_window_table_info(None, 0, i32, None) == ARG and L.vti_window_table_info(host, 0, None, None) == ARG
    assert L.vti_window_table_info(C.c_void_p(wt.frames.host.data_ptr()), 0, i32, None) == ARG       # a frame table is no window table
    assert L.vti_frame_table_info(host, 0, i32, None) == ARG


def test_the_size_queries(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    for n in (0, -1, -(1 << 31)):
        assert L.vti_window_table_bytes(n) == 0
    one, two = L.vti_window_table_bytes(1), L.vti_window_table_bytes(2)
    assert one > two - one > 0 and (two - one) % 16 == 0 and (2 * one - two) % 16 == 0
    eng = vti_amd.Engine("n", 2, H=64, W=96, max_batch=4)
    wt = eng.pack_windows(SHAPES, GOOD, device="cpu")
    host, fhost = C.c_void_p(wt.host.data_ptr()), C.c_void_p(wt.frames.host.data_ptr())
    for max_det in (1, 7, 300):
        want = L.vti_mask_native_frames_bytes(eng._ctx, fhost, max_det)
        assert want == sum(max_det * h * 8 * -(-w // 64) for h, w in SHAPES)
        assert L.vti_mask_native_windows_bytes(eng._ctx, host, max_det) == want == eng.mask_native_windows_bytes(wt, max_det)
    assert L.vti_mask_native_windows_bytes(eng._ctx, host, 0) == 0 and L.vti_mask_native_windows_bytes(None, host, 5) == 0
    assert L.vti_mask_native_windows_bytes(eng._ctx, None, 5) == 0 and L.vti_mask_native_windows_bytes(eng._ctx, fhost, 5) == 0
    other = vti_amd.Engine("n", 2, H=64, W=64, max_batch=4)
    assert L.vti_mask_native_windows_bytes(other._ctx, host, 5) == 0


def test_every_windows_call_refuses_bad_arguments_without_a_gpu(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    eng = vti_amd.Engine("n", 2, H=64, W=96, max_batch=4)
    t = eng.pack_windows(SHAPES, GOOD, device="cpu")
    other_canvas = vti_amd.Engine("n", 2, H=64, W=64, max_batch=4).pack_windows(SHAPES, GOOD, device="cpu")
    other_b = eng.pack_windows(SHAPES[:2], GOOD[:2], device="cpu")
    host = lambda x: C.c_void_p(x.host.data_ptr())
    one = C.c_void_p(4096)                                        # never dereferenced
    B, max_det = 3, 10
    BITS, U8 = vti_amd._lib.VTI_PACK_BITS, vti_amd._lib.VTI_PACK_U8
    err = lambda: L.vti_last_error(eng._ctx)
    hdr = 2 * L.vti_window_table_bytes(1) - L.vti_window_table_bytes(2)
    row = L.vti_window_table_bytes(2) - L.vti_window_table_bytes(1)

    def table_checks(call, fn):
        assert call(ctx=None) == ARG
        assert call(host_table=None) == ARG and call(dev_table=None) == ARG and b"null window table" in err()
        assert call(dev_table=C.c_void_p(4096 + 8)) == ARG and b"16-byte aligned" in err()
        assert call(host_table=host(other_canvas)) == ARG and b"another canvas" in err()
        assert call(host_table=host(other_b)) == ARG and b"another B" in err()
        assert call(B=2) == ARG and b"another B" in err() and call(B=0) == ARG and call(B=-1) == ARG
        junk = (C.c_uint8 * t.host.numel())()
        assert call(host_table=junk) == ARG and b"vti_pack_windows" in err()
        assert call(host_table=host(t.frames)) == ARG and b"vti_pack_windows" in err()          # a frame table is refused
        for at, value, needle in ((64 + 16, 500, b"inside its frame"),        # frame 1's x0
                                  (64 + 12, 100, b"inside its frame"),        # frame 1's W0 shrinks under its window
                                  (12, 0, b">= 1"),                           # the crop's w
                                  (0, 7, b"first byte")):                     # the crop's offset no longer follows from the origin
            bent = (C.c_uint8 * t.host.numel()).from_buffer_copy(bytes(t.host.numpy()))
            C.cast(bent, C.POINTER(C.c_int32))[(hdr + row + at) // 4] = value
            assert call(host_table=bent) == ARG and b"frame 1 of host_table" in err() and needle in err(), (at, err())
            assert err().startswith(fn.encode() + b":")

    def lb(ctx=eng._ctx, frames=one, host_table=host(t), dev_table=one, B=B, out=one):
        return L.vti_letterbox_windows(ctx, frames, host_table, dev_table, B, out, None)
    table_checks(lb, "vti_letterbox_windows")
    assert lb(frames=None) == ARG and lb(out=None) == ARG
    assert lb(frames=C.c_void_p(4096 + 8)) == ARG and b"16-byte" in err()
    assert lb(out=C.c_void_p(4096 + 2)) == ARG and b"4-byte" in err()
    small = vti_amd.Engine("n", 2, H=64, W=96, max_batch=2)
    assert lb(ctx=small._ctx) == ARG and b"max_batch" in L.vti_last_error(small._ctx)

    def sb(ctx=eng._ctx, dets=one, counts=one, host_table=host(t), dev_table=one, B=B, max_det=max_det, xyxy=one):
        return L.vti_scale_boxes_windows(ctx, dets, counts, host_table, dev_table, B, max_det, xyxy, None)
    table_checks(sb, "vti_scale_boxes_windows")
    for k in ("dets", "counts", "xyxy"):
        assert sb(**{k: None}) == ARG, k
    assert sb(max_det=0) == ARG and sb(xyxy=C.c_void_p(4096 + 4)) == ARG

    def mk(ctx=eng._ctx, dets=one, counts=one, proto=one, host_table=host(t), dev_table=one, B=B, max_det=max_det, mode=0, packing=BITS,
           masks=one, cap_bytes=1 << 16, offsets=one, bases=one):
        return L.vti_masks_native_windows(ctx, dets, counts, proto, host_table, dev_table, B, max_det, mode, packing, masks, cap_bytes, offsets,
                                          bases, None)
    table_checks(mk, "vti_masks_native_windows")
    for k in ("dets", "counts", "proto", "offsets", "bases", "masks"):
        assert mk(**{k: None}) == ARG, k
    assert mk(masks=None, cap_bytes=0) == STATE and b"workspace not set" in err()    # no masks needed for capacity 0: every check passed
    assert mk(masks=C.c_void_p(4096 + 4)) == ARG and b"8-byte aligned" in err()
    assert mk(bases=C.c_void_p(4096 + 4)) == ARG and mk(offsets=C.c_void_p(4096 + 2)) == ARG
    assert mk(packing=U8) == UNSUPPORTED and b"VTI_PACK_BITS" in err()
    assert mk(packing=7) == ARG and mk(mode=5) == ARG
    assert mk(max_det=0) == ARG and mk(cap_bytes=-1) == ARG and b"capacity_bytes" in err()
    assert mk(ctx=small._ctx) == ARG
    eng16 = vti_amd.Engine("n", 2, nm=16, H=64, W=96, max_batch=4)
    assert mk(ctx=eng16._ctx) == UNSUPPORTED and b"nm == 32" in L.vti_last_error(eng16._ctx)
    assert mk() == STATE and b"workspace not set" in err()            # every argument was accepted; no device has been touched

    def pr(ctx=eng._ctx, frames=one, host_table=host(t), dev_table=one, B=B, mode=0, packing=BITS, scratch=one, pred=one, proto=one,
           dets=one, counts=one, masks=one, cap_bytes=1 << 16, offsets=one, bases=one, xyxy=one, max_det=max_det):
        return L.vti_predict_windows(ctx, frames, host_table, dev_table, B, 0, 0.25, 0.7, max_det, 0, mode, packing, scratch, pred, proto,
                                     dets, counts, masks, cap_bytes, offsets, bases, xyxy, None)
    table_checks(pr, "vti_predict_windows")
    for k in ("frames", "scratch", "pred", "proto", "dets", "counts", "masks", "offsets", "bases", "xyxy"):
        assert pr(**{k: None}) == ARG, k
    assert b"dev_xyxy is required" in err()
    assert pr(frames=C.c_void_p(4096 + 8)) == ARG and pr(xyxy=C.c_void_p(4096 + 4)) == ARG
    assert pr(masks=C.c_void_p(4096 + 4)) == ARG and pr(cap_bytes=-8) == ARG and pr(max_det=0) == ARG
    assert pr(packing=U8) == UNSUPPORTED and pr(mode=5) == ARG
    assert pr(ctx=eng16._ctx) == UNSUPPORTED
    assert pr(ctx=small._ctx) == ARG
    assert pr() == STATE and b"weights not loaded" in err()           # every argument was accepted; no device has been touched
    assert pr(mode=vti_amd._lib.VTI_MASK_NATIVE | 1) == STATE         # the flag is implied
    # the *_frames calls do not take a window table, and stop where they did
    assert L.vti_letterbox_frames(eng._ctx, one, host(t), one, B, one, None) == ARG and b"vti_pack_frames" in err()
    assert L.vti_letterbox_frames(eng._ctx, one, host(t.frames), one, B, one, None) in (0, STATE, -3, -4, -5)   # past the checks: a HIP error here


def test_the_python_surface_refuses_before_an_engine_exists(lib_built, monkeypatch):
    vti_amd = lib_built
    model = vti_amd.YOLO(None, scale="n", nc=2, seed=3)
    frame = np.zeros((48, 64, 3), np.uint8)
    batch = np.zeros((2, 48, 64, 3), np.uint8)
    mixed = [np.zeros((48, 64, 3), np.uint8), np.zeros((64, 40, 3), np.uint8)]
    bad = [(0, 0, 65, 48), (0, 0, 64, 49), (-1, 0, 10, 10), (0, -1, 10, 10), (10, 10, 10, 20), (10, 10, 20, 10), (30, 5, 20, 40),
           (0, 0, 10), (0, 0, 10, 10, 10), (0.0, 0, 10, 10), "roi", (True, 0, 10, 10), 7, [], ("0", "0", "8", "8")]
    for w in bad:
        with pytest.raises(ValueError, match="window"):
            model.predict(frame, window=w, imgsz=64)
        with pytest.raises(ValueError, match="window"):
            model.predict(batch, window=[None, w], imgsz=64)
    with pytest.raises(ValueError, match="window has 3 entries but the batch has 2 frames"):
        model.predict(batch, window=[None, None, None], imgsz=64)
    with pytest.raises(ValueError, match="window of frame 1"):
        model.predict(mixed, window=(0, 0, 64, 48), imgsz=64)               # fits frame 0, not the 64x40 frame 1
    with pytest.raises(ValueError, match="window of frame 1"):
        model.predict(mixed, window=[None, (0, 0, 41, 64)], imgsz=64)
    assert model._engines == {}                                               # nothing was built, nothing uploaded

    def reached(*a, **k):
        raise AssertionError("predict was reached")
    monkeypatch.setattr(model, "_predict_outputs_windows", reached)
    monkeypatch.setattr(model, "_to_device_batch", lambda s: s)
    for good in ((0, 0, 64, 48), (63, 47, 64, 48), [None, (1, 2, 3, 4)], np.array([0, 0, 8, 8]), [np.int64(0), 0, 8, 8]):
        with pytest.raises(AssertionError, match="predict was reached"):
            model.predict(batch, window=good, imgsz=64)
    with pytest.raises(AssertionError, match="predict was reached"):
        model.predict(mixed, window=[(0, 0, 64, 48), (0, 0, 40, 64)], imgsz=64)
    assert vti_amd.YOLO._windows_arg((1, 2, 30, 40), [(48, 64)] * 2) == [(1, 2, 29, 38)] * 2
    assert vti_amd.YOLO._windows_arg([None, (1, 2, 30, 40)], [(48, 64)] * 2) == [(0, 0, 64, 48), (1, 2, 29, 38)]

    # the measurers: window / windows and window_margin, refused before the predict; the checkers do not take the keyword
    p = vti_amd.MeasureParams(*load_calib())
    sm = vti_amd.StitchMeasurer(model, p)
    rig = vti_amd.MultiCameraMeasurer(model, [p, p])
    for w in ((0, 0, 65, 48), "all", (0, 0, 10), [None]):
        with pytest.raises(ValueError, match="window"):
            sm.process_frames(batch, window=w, imgsz=64)
    with pytest.raises(ValueError, match="window_margin"):
        sm.process_frames(batch, window="roi", window_margin=-1, imgsz=64)
    with pytest.raises(ValueError, match="one entry per camera"):
        rig.process_frames(batch, [0, 1], windows=[None], imgsz=64)
    with pytest.raises(ValueError, match="window of frame 1"):
        rig.process_frames(batch, [0, 1], windows=[None, (0, 0, 65, 48)], imgsz=64)
    with pytest.raises(ValueError, match="retina_masks=True needs frames of one size"):
        rig.process_frames(mixed, [0, 1], windows="roi", imgsz=64, annotate="all", mixed=True)
    with pytest.raises(AssertionError, match="predict was reached"):
        sm.process_frames(batch, window="roi", imgsz=64)
    with pytest.raises(AssertionError, match="predict was reached"):
        rig.process_frames(batch, [0, 1], windows=["roi", (0, 0, 8, 8)], imgsz=64)
    cp = vti_amd.CheckerParams(*load_calib())
    with pytest.raises(TypeError):
        vti_amd.StitchDistanceChecker(model, cp).process_frames(batch, window="roi")
    with pytest.raises(TypeError):
        vti_amd.MultiCameraChecker(model, [cp]).process_frames(batch, [0, 0], windows="roi")
    assert model._engines == {}
    # "roi": the clamped ROI (inclusive bounds) grown by the margin and clipped to the frame; disabled: the whole frame
    fw = vti_amd.measure._DeviceStage._frame_windows
    q = vti_amd.MeasureParams(*load_calib(), roi=(10, 300, 1270, 760))
    assert fw("roi", 32, [(960, 1280)], lambda b: q) == [(0, 268, 1280, 525)]
    assert fw("roi", 0, [(960, 1280)], lambda b: q) == [(10, 300, 1261, 461)]
    assert fw("roi", 32, [(480, 640)], lambda b: q) == [(0, 268, 640, 212)]       # the ROI is clamped to the frame first
    off = vti_amd.MeasureParams(*load_calib(), roi_enabled=False)
    assert fw("roi", 32, [(960, 1280)], lambda b: off) == [(0, 0, 1280, 960)]
    assert fw(["roi", None, (1, 2, 3, 4)], 8, [(960, 1280)] * 3, lambda b: q) == [(2, 292, 1277, 477), (0, 0, 1280, 960), (1, 2, 2, 2)]

    eng = vti_amd.Engine("n", 2, H=64, W=96, max_batch=4)
    wt = eng.pack_windows(SHAPES, GOOD, device="cpu")
    with pytest.raises(ValueError, match="WindowTable"):
        eng.letterbox_windows(torch.zeros(wt.total_bytes, dtype=torch.uint8), wt.frames)
    with pytest.raises(ValueError, match="WindowTable"):
        eng.predict_windows_into(torch.zeros(wt.total_bytes, dtype=torch.uint8), wt.frames, {})
    with pytest.raises(ValueError, match="frame buffer"):
        eng.letterbox_windows(torch.zeros(wt.total_bytes - 1, dtype=torch.uint8), wt)
    plain = dict(dets=torch.zeros((3, 10, 38)), xyxy=torch.zeros((3, 10, 4)), counts=torch.zeros(3, dtype=torch.int32),
                 offsets=torch.zeros(4, dtype=torch.int32), masks=torch.zeros((0, 64, 8), dtype=torch.uint8))
    with pytest.raises(ValueError, match="native_frames"):
        eng.predict_windows_into(torch.zeros(wt.total_bytes, dtype=torch.uint8), wt, plain)
    ragged = eng.alloc_outputs(3, 10, 0, device="cpu", native_frames=wt.frames)
    assert ragged["masks"].shape == (eng.mask_native_windows_bytes(wt, 10),)
    other = eng.pack_windows(SHAPES[:2] + [(100, 100)], GOOD[:2] + [(0, 0, 1, 1)], device="cpu")
    with pytest.raises(ValueError, match="other frame shapes"):
        eng.predict_windows_into(torch.zeros(other.total_bytes, dtype=torch.uint8), other, ragged)


def test_the_refusals_run_clean_in_a_stand_alone_program_under_the_host_sanitizers(lib_built, tmp_path):
    """tests/windows_args_main.cpp: its own main, built with -fsanitize=address,undefined, linked against libvti.so and run
    directly (nothing is loaded into Python, nothing is preloaded).  Every refusal comes before the first HIP call."""
    vti_amd = lib_built
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    lib_dir = os.path.dirname(vti_amd.LIB_PATH)
    exe = str(tmp_path / "windows_args_main")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx).startswith("g++") else []    # no link-order rule to meet
    subprocess.run([cxx, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static, "-I",
                    os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "windows_args_main.cpp"), "-L", lib_dir, "-lvti",
                    "-Wl,-rpath," + lib_dir, "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and re.fullmatch(r"ok \d+\n", run.stdout) and run.stderr == "", (run.returncode, run.stdout, run.stderr)
    assert int(run.stdout.split()[1]) >= 90
