"""Frame-resolution masks for frames of differing sizes (the ragged mask buffer), without a GPU: the new entry points exist with
their signatures, the worst-case size is the sum of vti_mask_native_layout's slots, every argument check of the three device calls
comes before the first HIP call (fake pointers, never dereferenced), and the Python surface refuses before it touches a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_oracle_geometry import load_calib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vti_mask_native_frames_bytes", "vti_masks_native_frames", "vti_predict_frames_native", "vti_measure_frames_native")
SHAPES = [(90, 120), (481, 333), (640, 640), (1080, 1920)]


def test_the_entry_points_are_declared_exported_and_bound(lib_built):
    vti_amd = lib_built
    hdr = open(os.path.join(ROOT, "include", "vti.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", vti_amd.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"\bT %s$" % name, exported, re.M), name
        assert name in vti_amd.SIGNATURES
    S, P, I32, I64 = vti_amd.SIGNATURES, C.c_void_p, C.c_int32, C.c_int64
    assert S["vti_mask_native_frames_bytes"] == (I64, [P, P, I32])
    res, args = S["vti_masks_native_frames"]
    assert res is I32 and len(args) == 16 and args[12] is I64 and args[7:11] == [I32] * 4       # capacity_bytes is 64-bit
    res, args = S["vti_predict_frames_native"]
    assert res is I32 and len(args) == 23 and args[18] is I64
    res, args = S["vti_measure_frames_native"]
    assert res is I32 and len(args) == 23 and args[6] is I64 and args[17] is C.c_size_t
    for meth in ("mask_native_frames_bytes", "masks_native_frames", "frame_masks"):
        assert hasattr(vti_amd.Engine, meth)


def test_the_worst_case_is_the_sum_of_the_frames_slots(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    eng = vti_amd.Engine("n", 2, H=640, W=640, max_batch=4)
    t, _, _ = eng.pack_frames(SHAPES, device="cpu")
    host = C.c_void_p(t.host.data_ptr())
    for max_det in (1, 7, 300):
        want = 0
        for H0, W0 in SHAPES:
            lay = eng.mask_native_layout(H0, W0, "bits")
            assert lay["row_bytes"] == 8 * -(-W0 // 64) and lay["slot_bytes"] == H0 * lay["row_bytes"]
            want += max_det * lay["slot_bytes"]
        assert L.vti_mask_native_frames_bytes(eng._ctx, host, max_det) == want == eng.mask_native_frames_bytes(t, max_det)
    assert L.vti_mask_native_frames_bytes(eng._ctx, host, 0) == 0 and L.vti_mask_native_frames_bytes(eng._ctx, host, -3) == 0
    assert L.vti_mask_native_frames_bytes(None, host, 5) == 0 and L.vti_mask_native_frames_bytes(eng._ctx, None, 5) == 0
    junk = (C.c_uint8 * t.host.numel())()
    assert L.vti_mask_native_frames_bytes(eng._ctx, junk, 5) == 0
    other, _, _ = vti_amd.Engine("n", 2, H=640, W=672, max_batch=4).pack_frames(SHAPES, device="cpu")
    assert L.vti_mask_native_frames_bytes(eng._ctx, C.c_void_p(other.host.data_ptr()), 5) == 0          # another canvas
    bent = (C.c_uint8 * t.host.numel()).from_buffer_copy(bytes(t.host.numpy()))
    hdr = L.vti_frame_table_bytes(1) - (L.vti_frame_table_bytes(2) - L.vti_frame_table_bytes(1))
    C.cast(bent, C.POINTER(C.c_int32))[(hdr + 64) // 4 + 2] = 0                                           # frame 1's H0
    assert L.vti_mask_native_frames_bytes(eng._ctx, bent, 5) == 0


def _tables(vti_amd, nm=32):
    eng = vti_amd.Engine("n", 2, nm=nm, H=64, W=64, max_batch=4)
    shapes = [(48, 64), (64, 40), (100, 130)]
    t, _, _ = eng.pack_frames(shapes, device="cpu")
    other_canvas, _, _ = vti_amd.Engine("n", 2, H=64, W=96, max_batch=4).pack_frames(shapes, device="cpu")
    other_b, _, _ = eng.pack_frames(shapes[:2], device="cpu")
    return eng, t, other_canvas, other_b


def test_every_argument_check_runs_without_a_gpu(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    eng, t, other_canvas, other_b = _tables(vti_amd)
    host = lambda x: C.c_void_p(x.host.data_ptr())
    one, ws = C.c_void_p(4096), C.c_void_p(1 << 20)               # never dereferenced
    B, max_det, cap = 3, 10, 20
    BITS, U8 = vti_amd._lib.VTI_PACK_BITS, vti_amd._lib.VTI_PACK_U8
    err = lambda: L.vti_last_error(eng._ctx)

    def table_checks(call):
        assert call(ctx=None) == -1
        assert call(host_table=None) == -1 and call(dev_table=None) == -1
        assert call(dev_table=C.c_void_p(4096 + 8)) == -1
        assert call(host_table=host(other_canvas)) == -1 and b"another canvas" in err()
        assert call(host_table=host(other_b)) == -1 and b"another B" in err()
        assert call(B=2) == -1 and b"another B" in err()
        junk = (C.c_uint8 * t.host.numel())()
        assert call(host_table=junk) == -1 and b"vti_pack_frames" in err()
        bent = (C.c_uint8 * t.host.numel()).from_buffer_copy(bytes(t.host.numpy()))
        hdr = L.vti_frame_table_bytes(1) - (L.vti_frame_table_bytes(2) - L.vti_frame_table_bytes(1))
        C.cast(bent, C.POINTER(C.c_int64))[(hdr + 64) // 8] = 1 << 40         # frame 1's offset, past total_bytes
        assert call(host_table=bent) == -1 and b"frame 1" in err()

    def mk(ctx=eng._ctx, dets=one, xyxy=one, counts=one, proto=one, host_table=host(t), dev_table=one, B=B, max_det=max_det, mode=0,
           packing=BITS, masks=one, cap_bytes=1 << 16, offsets=one, bases=one):
        return L.vti_masks_native_frames(ctx, dets, xyxy, counts, proto, host_table, dev_table, B, max_det, mode, packing, masks,
                                         cap_bytes, offsets, bases, None)
    table_checks(mk)
    for k in ("dets", "xyxy", "counts", "proto", "offsets", "bases", "masks"):
        assert mk(**{k: None}) == -1, k
    assert mk(masks=None, cap_bytes=0) == -2 and b"workspace not set" in err()      # no masks needed for capacity 0: every check passed
    assert mk(masks=C.c_void_p(4096 + 4)) == -1 and b"8-byte aligned" in err()
    assert mk(bases=C.c_void_p(4096 + 4)) == -1
    assert mk(packing=U8) == -6 and b"VTI_PACK_BITS" in err()
    assert mk(packing=7) == -1 and mk(mode=5) == -1
    assert mk(max_det=0) == -1 and mk(cap_bytes=-1) == -1 and b"capacity_bytes" in err()
    small = vti_amd.Engine("n", 2, H=64, W=64, max_batch=2)
    assert mk(ctx=small._ctx) == -1
    eng16, t16, _, _ = _tables(vti_amd, nm=16)
    assert mk(ctx=eng16._ctx, host_table=host(t16)) == -6 and b"nm == 32" in L.vti_last_error(eng16._ctx)
    assert mk() == -2 and b"workspace not set" in err()            # every argument was accepted; no device has been touched

    def pr(ctx=eng._ctx, frames=one, host_table=host(t), dev_table=one, B=B, mode=0, packing=BITS, scratch=one, pred=one, proto=one,
           dets=one, counts=one, masks=one, cap_bytes=1 << 16, offsets=one, bases=one, xyxy=one, max_det=max_det):
        return L.vti_predict_frames_native(ctx, frames, host_table, dev_table, B, 0, 0.25, 0.7, max_det, 0, mode, packing, scratch, pred,
                                           proto, dets, counts, masks, cap_bytes, offsets, bases, xyxy, None)
    table_checks(pr)
    for k in ("frames", "scratch", "pred", "proto", "dets", "counts", "masks", "offsets", "bases", "xyxy"):
        assert pr(**{k: None}) == -1, k
    assert b"dev_xyxy is required" in err()
    assert pr(frames=C.c_void_p(4096 + 8)) == -1 and pr(xyxy=C.c_void_p(4096 + 4)) == -1
    assert pr(masks=C.c_void_p(4096 + 4)) == -1 and pr(cap_bytes=-8) == -1 and pr(max_det=0) == -1
    assert pr(packing=U8) == -6 and pr(mode=5) == -1
    assert pr(ctx=eng16._ctx, host_table=host(t16)) == -6
    assert pr() == -2 and b"weights not loaded" in err()          # every argument was accepted; no device has been touched
    assert pr(mode=vti_amd._lib.VTI_MASK_NATIVE | 1) == -2        # the flag is implied

    need = eng.measure_scratch_bytes(B, cap, t.max_W0)
    assert need > eng.measure_scratch_bytes(B, cap, 64)

    def ms(ctx=eng._ctx, cams=one, n_cams=2, index=one, masks=one, bases=one, cap_bytes=1 << 16, dets=one, host_table=host(t),
           dev_table=one, B=B, max_det=max_det, cap=cap, scratch=ws, nbytes=need, frame_f64=one):
        return L.vti_measure_frames_native(ctx, cams, n_cams, index, masks, bases, cap_bytes, dets, one, one, one, host_table, dev_table,
                                           B, max_det, cap, scratch, nbytes, frame_f64, one, None, None, None)
    table_checks(ms)
    assert ms(cams=None) == -1 and ms(index=None) == -1 and ms(n_cams=0) == -1
    assert ms(cams=C.c_void_p(4096 + 8)) == -1 and ms(index=C.c_void_p(4096 + 2)) == -1
    assert ms(bases=None) == -1 and ms(bases=C.c_void_p(4096 + 4)) == -1 and ms(cap_bytes=-1) == -1
    assert ms(nbytes=need - 1) == -1 and b"scratch" in err()      # one byte short for the LARGEST W0 of the table
    assert ms(nbytes=eng.measure_scratch_bytes(B, cap, 64)) == -1
    assert ms(scratch=C.c_void_p(4096 + 64)) == -1 and ms(scratch=None) == -1
    assert ms(masks=C.c_void_p(4096 + 4)) == -1 and ms(masks=None) == -1 and ms(dets=None) == -1 and ms(frame_f64=None) == -1
    assert ms(max_det=0) == -1 and ms(cap=-1) == -1
    assert ms(max_det=vti_amd._lib.VTI_MEASURE_MAX_DET + 1) == -6
    # the refusals of the calls this one stands beside are as they were
    assert L.vti_measure_frames(eng._ctx, one, 2, one, one, 1, one, one, one, one, host(t), one, B, max_det, cap, ws, need, one, one,
                                None, None, None) == -6
    assert L.vti_predict_frames(eng._ctx, one, host(t), one, B, 0, 0.25, 0.7, max_det, 0, vti_amd._lib.VTI_MASK_NATIVE, 1, one, one, one,
                                one, one, one, cap, one, one, None) == -6


def test_python_surface_refuses_before_touching_a_device(lib_built):
    import torch
    vti_amd = lib_built
    frames = [np.zeros((48, 64, 3), np.uint8), np.zeros((64, 40, 3), np.uint8)]
    model = vti_amd.YOLO(None, scale="n", nc=2)
    for bad in ("yes", 1, None):
        with pytest.raises(ValueError, match="mixed must be True or False"):
            model.predict(frames, retina_masks=True, mixed=bad, imgsz=64)
    with pytest.raises(ValueError, match="retina_masks"):
        model.predict(frames, retina_masks=True, mixed=False, imgsz=64)
    assert not model._engines                                     # nothing was built, nothing uploaded
    p = vti_amd.MeasureParams(*load_calib())
    with pytest.raises(ValueError, match="retina_masks=True needs frames of one size"):
        vti_amd.MultiCameraMeasurer(model, [p]).process_frames(frames, [0, 0], imgsz=64, retina_masks=True, annotate="all", mixed=True)
    eng, t, other_canvas, other_b = _tables(vti_amd)
    B, max_det = 3, 10
    plain = dict(dets=torch.zeros((B, max_det, 38)), xyxy=torch.zeros((B, max_det, 4)), counts=torch.zeros(B, dtype=torch.int32),
                 offsets=torch.zeros(B + 1, dtype=torch.int32), masks=torch.zeros((0, 64, 8), dtype=torch.uint8))
    with pytest.raises(ValueError, match="native_frames"):
        eng.predict_frames_into(torch.zeros(t.total_bytes, dtype=torch.uint8), t, plain, native=True)
    ragged = eng.alloc_outputs(B, max_det, 0, device="cpu", native_frames=t)
    assert ragged["masks"].shape == (eng.mask_native_frames_bytes(t, max_det),) and ragged["mask_bases"].shape == (B + 1,)
    assert ragged["mask_bases"].dtype == torch.int64
    with pytest.raises(ValueError, match="other frame shapes"):
        eng.predict_frames_into(torch.zeros(other_b.total_bytes, dtype=torch.uint8), other_b, ragged, native=True)
    row = int(vti_amd.lib().vti_measure_cameras_bytes(1))
    cams = torch.zeros(2 * row, dtype=torch.uint8)
    with pytest.raises(ValueError, match="native"):
        eng.measure(plain, cams, cameras=[0, 1, 0], frames=t, native=True)       # not a ragged set: as before
    with pytest.raises(ValueError, match="device memory") as ei:
        eng.measure(ragged, cams, cameras=[0, 1, 0], frames=t, native=True)      # accepted as ragged; stops at the device check
    assert "native" not in str(ei.value)
    with pytest.raises(ValueError):
        eng.alloc_outputs(B, max_det, 0, device="cpu", native_frames=t, native_hw=(48, 64))
    with pytest.raises(ValueError):
        eng.alloc_outputs(2, max_det, 0, device="cpu", native_frames=t)
