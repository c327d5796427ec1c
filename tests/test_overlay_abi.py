"""vti_overlay's C ABI without a GPU: the two entry points exist, the scratch size, every argument check (all before the first HIP
call: fake pointers, never dereferenced), and the Python surface refuses what it cannot serve before it touches a device.  The GPU
parity tests are in test_gpu_overlay.py."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vti_overlay_scratch_bytes", "vti_overlay")


def test_the_entry_points_are_declared_exported_and_bound(lib_built):
    vti_amd = lib_built
    hdr = open(os.path.join(ROOT, "include", "vti.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", vti_amd.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"\bT %s$" % name, exported, re.M), name
        assert name in vti_amd.SIGNATURES
    # the header's argument list and the ctypes signature have the same length
    decl = re.search(r"int32_t vti_overlay\((.*?)\);", hdr, re.S).group(1)
    assert len(decl.split(",")) == len(vti_amd.SIGNATURES["vti_overlay"][1]) == 29
    assert hasattr(vti_amd.Engine, "overlay") and "overlay" in vti_amd.__all__
    L = vti_amd._lib
    assert (L.VTI_OVERLAY_DRAW, L.VTI_OVERLAY_BLEND, L.VTI_OVERLAY_BOTH, L.VTI_OVERLAY_OUTLINE_SKIPPED) == (1, 2, 3, 1)
    assert re.search(r"VTI_OVERLAY_DRAW\s*=\s*1,\s*VTI_OVERLAY_BLEND\s*=\s*2,\s*VTI_OVERLAY_BOTH\s*=\s*3", hdr)
    assert re.search(r"VTI_OVERLAY_OUTLINE_SKIPPED\s*=\s*1", hdr)
    O = vti_amd.overlay
    assert (O.DRAW, O.BLEND, O.BOTH, O.OUTLINE_SKIPPED) == (1, 2, 3, 1)


def test_scratch_bytes_is_zero_on_bad_arguments_and_monotone(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    eng = vti_amd.Engine("n", 2, H=736, W=960, max_batch=1)
    f = lambda n_sel=8, max_det=200, H0=960, W0=1280, mp=4096, ctx=eng._ctx: L.vti_overlay_scratch_bytes(ctx, n_sel, max_det, H0, W0, mp)
    base = f()
    assert base > 0 and base % 256 == 0
    # per frame at least: the contour vertices, the owner planes of a frame-size slot and one bitmap per labelling area
    assert base >= 8 * (16 * 4096 + 960 * 40 * 32 + 16 * 960 * 20 * 8)
    assert f(ctx=None) == 0 and f(n_sel=0) == 0 and f(n_sel=-1) == 0 and f(max_det=0) == 0 and f(max_det=1001) == 0
    assert f(H0=0) == 0 and f(W0=0) == 0 and f(H0=8193) == 0 and f(W0=8193) == 0 and f(mp=-1) == 0
    assert f(mp=0) > 0 and f(max_det=1000) > 0 and f(H0=8192, W0=8192, n_sel=1) > 0
    sizes = [f(n_sel=n) for n in (1, 2, 8, 64)]
    assert sizes == sorted(sizes) and len(set(sizes)) == 4
    sizes = [f(mp=m) for m in (0, 1, 100, 4096, 1 << 20)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
    assert eng.overlay_scratch_bytes(8, 200, 960, 1280, 4096) == base
    # a small frame still has room for the owner planes of the engine's letterbox canvas (736 x 960 bits)
    assert f(n_sel=1, max_det=1, H0=8, W0=8, mp=0) >= 736 * (960 // 32) * 32


def test_overlay_argument_checks_come_before_any_hip_call(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    eng = vti_amd.Engine("n", 2, H=736, W=960, max_batch=4)
    B, H0, W0, max_det, cap, n_sel, mp = 4, 960, 1280, 200, 800, 3, 4096
    need = eng.overlay_scratch_bytes(n_sel, max_det, H0, W0, mp)
    one, ws = C.c_void_p(4096), C.c_void_p(1 << 20)            # never dereferenced
    good_sel = (C.c_int32 * n_sel)(3, 0, 3)
    pal = (C.c_uint8 * 18)(*range(18))
    nan, inf = float("nan"), float("inf")

    def call(ctx=eng._ctx, frames=one, B=B, H0=H0, W0=W0, masks=one, native=0, dets=one, xyxy=one, counts=one, offsets=one,
             max_det=max_det, cap=cap, plates=one, pal=pal, nc=6, alpha=0.3, beta=0.7, hsel=good_sel, dsel=one, n_sel=n_sel, mode=3,
             ann=None, mp=mp, out=one, status=one, scratch=ws, nbytes=need):
        return L.vti_overlay(ctx, frames, B, H0, W0, masks, native, dets, xyxy, counts, offsets, max_det, cap, plates, pal, nc, alpha,
                             beta, hsel, dsel, n_sel, mode, ann, mp, out, status, scratch, nbytes, None)

    err = lambda: L.vti_last_error(eng._ctx)
    assert call(ctx=None) == -1
    for name in ("frames", "dets", "xyxy", "counts", "offsets", "pal", "hsel", "dsel", "out", "status", "scratch"):
        assert call(**{name: None}) == -1, name
        assert b"null pointer" in err() or b"scratch" in err(), name
    assert call(masks=None) == -1                               # capacity > 0 needs the masks
    for mode in (0, 4, -1, 7):
        assert call(mode=mode) == -1 and b"mode" in err()
    for nc in (0, 17, -3):
        assert call(nc=nc) == -1 and b"n_colours" in err()
    for kw in (dict(alpha=nan), dict(beta=nan), dict(alpha=inf), dict(beta=-inf)):
        assert call(**kw) == -1 and b"finite" in err(), kw
    assert call(mode=2) == -1 and b"dev_annotated" in err()     # BLEND needs the picture ...
    assert call(mode=3, ann=one) == -1 and b"dev_annotated" in err()        # ... and only BLEND takes one
    assert call(mode=1, ann=one) == -1 and b"dev_annotated" in err()
    assert call(n_sel=0) == -1 and call(n_sel=-2) == -1
    assert call(hsel=(C.c_int32 * 3)(0, -1, 1)) == -1
    assert b"host_select[1] = -1" in err()
    assert call(hsel=(C.c_int32 * 3)(0, 1, B)) == -1
    assert b"host_select[2] = 4" in err()
    assert call(native=2) == -1 and call(native=-1) == -1
    assert call(masks=C.c_void_p(4096 + 8)) == -1 and b"16-byte" in err()   # letterbox bits: 16-byte aligned
    assert call(native=1, masks=C.c_void_p(4096 + 4)) == -1     # native rows: 8-byte aligned
    assert call(plates=C.c_void_p(4096 + 8)) == -1 and b"dev_plates" in err()
    assert call(dsel=C.c_void_p(4096 + 2)) == -1 and call(status=C.c_void_p(4096 + 2)) == -1
    assert call(scratch=C.c_void_p((1 << 20) + 64)) == -1 and b"scratch" in err()
    assert call(nbytes=need - 1) == -1 and b"scratch" in err()
    assert call(max_det=1001) == -1 and call(max_det=0) == -1
    assert call(mp=-1) == -1
    assert call(B=0) == -1 and call(cap=-1) == -1
    assert call(H0=0) == -1 and call(W0=8193, nbytes=1 << 40) == -1
    # what IS accepted up to the device check: no plates, no masks when the capacity is 0, native rows at 8 bytes, BLEND with its
    # picture (which may be dev_out itself), one colour, sixteen.  Without a GPU the call then stops at the device check, with the HIP
    # status, never with VTI_ERR_ARG.
    for kw in (dict(plates=None), dict(cap=0, masks=None), dict(native=1, masks=C.c_void_p(4096 + 8)), dict(mode=2, ann=one),
               dict(mode=1), dict(nc=1), dict(nc=16, pal=(C.c_uint8 * 48)()), dict(hsel=(C.c_int32 * 3)(2, 2, 2)), dict(alpha=0.0, beta=-2.5)):
        assert call(**kw) != -1, kw


def _fake_out(torch, B, max_det=8, cap=4):
    return dict(dets=torch.zeros((B, max_det, 38)), xyxy=torch.zeros((B, max_det, 4)), counts=torch.zeros(B, dtype=torch.int32),
                offsets=torch.zeros(B + 1, dtype=torch.int32), masks=torch.zeros((cap, 64, 8), dtype=torch.uint8))


def test_engine_overlay_refuses_bad_input_before_it_touches_a_device(lib_built):
    import torch
    vti_amd = lib_built
    eng = vti_amd.Engine("n", 2, H=64, W=64, max_batch=2)
    B = 2
    out = _fake_out(torch, B)
    frames = torch.zeros((B, 48, 64, 3), dtype=torch.uint8)         # a host batch: the shape and value checks come first
    with pytest.raises(ValueError, match="uint8"):
        eng.overlay(frames.float(), out, [0])
    for sel in ([B], [-1], [0, 1, 2], [], [[0]], [0.5]):
        with pytest.raises(ValueError, match="select|frame index"):
            eng.overlay(frames, out, sel)
    with pytest.raises(ValueError, match="frames but an output set"):
        eng.overlay(frames, _fake_out(torch, 3), [0])
    with pytest.raises(ValueError, match="mode"):
        eng.overlay(frames, out, [0], mode="tint")
    with pytest.raises(ValueError, match="annotated"):
        eng.overlay(frames, out, [0], mode="blend")
    with pytest.raises(ValueError, match="annotated"):
        eng.overlay(frames, out, [0], mode="both", annotated=frames[:1])
    with pytest.raises(ValueError, match="palette"):
        eng.overlay(frames, out, [0], palette=[(0, 0, 0)] * 17)
    with pytest.raises(ValueError, match="finite"):
        eng.overlay(frames, out, [0], alpha=float("nan"))
    with pytest.raises(ValueError, match="masks"):
        eng.overlay(frames, out, [0], native=True)                  # the set's masks are letterbox bits
    with pytest.raises(ValueError, match="device batch"):          # a good call on host memory stops at the device check
        eng.overlay(frames, out, [0])
