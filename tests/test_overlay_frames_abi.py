"""vti_overlay_frames' C ABI without a GPU: the two entry points exist, the scratch size is vti_overlay's at the largest selected
frame, every refusal comes before the first HIP call (fake pointers, never dereferenced; without a GPU a call that reaches HIP ends
with the HIP status instead), and Engine.overlay(table=) refuses what it cannot serve before it touches a device.  The GPU parity
tests are in test_gpu_overlay_frames.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vti_overlay_frames_scratch_bytes", "vti_overlay_frames")
SHAPES = [(960, 1280), (481, 333), (720, 960), (1080, 1920)]
ARG, UNSUPPORTED = -1, -6


def _hp(t):
    return C.c_void_p(t.host.data_ptr())


def test_the_entry_points_are_declared_exported_and_bound(lib_built):
    vti_amd = lib_built
    hdr = open(os.path.join(ROOT, "include", "vti.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", vti_amd.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"\bT %s$" % name, exported, re.M), name
        assert name in vti_amd.SIGNATURES, name
        # the header's argument list and the ctypes signature have the same length
        decl = re.search(r"int(?:32|64)_t %s\((.*?)\);" % name, hdr, re.S).group(1)
        assert len(decl.split(",")) == len(vti_amd.SIGNATURES[name][1]), name
    assert len(vti_amd.SIGNATURES["vti_overlay_frames"][1]) == 33 and len(vti_amd.SIGNATURES["vti_overlay_frames_scratch_bytes"][1]) == 4
    # the uniform call's header no longer names the frames form as missing; only text on the device stays out
    doc = hdr[hdr.index("the model-check viewer's picture on device"):hdr.index("int64_t vti_overlay_scratch_bytes(")]
    assert "Not covered: batches" not in doc and "text on the device" in doc
    assert "annotate_results" in vti_amd.overlay.__all__ and "annotate_result" in vti_amd.overlay.__all__
    assert callable(vti_amd.overlay.annotate_results)


def test_scratch_bytes_is_vti_overlays_at_the_largest_selected_frame(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    eng = vti_amd.Engine("n", 2, H=736, W=960, max_batch=4)
    f = lambda t, max_det=200, mp=4096, ctx=eng._ctx: L.vti_overlay_frames_scratch_bytes(ctx, _hp(t) if t is not None else None, max_det, mp)
    for sel in ([0, 1, 2, 3], [1, 2], [1], [3, 3, 0], [2, 1, 1]):
        shapes = [SHAPES[b] for b in sel]
        t, _, _ = eng.pack_frames(shapes, device="cpu")
        mh, mw = max(h for h, _ in shapes), max(w for _, w in shapes)       # the largest H0 and W0 need not be of one frame
        want = eng.overlay_scratch_bytes(len(sel), 200, mh, mw, 4096)
        assert want > 0 and f(t) == want, (sel, f(t), want)
    t, _, _ = eng.pack_frames(SHAPES, device="cpu")
    assert f(t, ctx=None) == 0 and f(None) == 0 and f(t, max_det=0) == 0 and f(t, max_det=1001) == 0 and f(t, mp=-1) == 0
    big, _, _ = eng.pack_frames([(8200, 480)], device="cpu")                # the table allows it, the raster does not
    assert f(big) == 0
    junk = np.zeros(256, np.uint8)
    assert L.vti_overlay_frames_scratch_bytes(eng._ctx, C.c_void_p(junk.ctypes.data), 200, 4096) == 0


def test_every_refusal_comes_before_any_hip_call(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    eng = vti_amd.Engine("n", 2, H=736, W=960, max_batch=4)
    B, max_det, cap, mp = 4, 200, 800, 4096
    sel = [3, 0, 3]
    t_in, _, _ = eng.pack_frames(SHAPES, device="cpu")
    t_out, _, _ = eng.pack_frames([SHAPES[b] for b in sel], device="cpu")
    need = L.vti_overlay_frames_scratch_bytes(eng._ctx, _hp(t_out), max_det, mp)
    assert need > 0
    one, ws = C.c_void_p(4096), C.c_void_p(1 << 20)                # never dereferenced
    good_sel = (C.c_int32 * 3)(*sel)
    pal = (C.c_uint8 * 18)(*range(18))
    err = lambda: L.vti_last_error(eng._ctx)

    def call(ctx=eng._ctx, frames=one, ht=_hp(t_in), dt=one, B=B, masks=one, native=0, bases=None, cbytes=0, dets=one, xyxy=one,
             counts=one, offsets=one, max_det=max_det, cap=cap, plates=one, pal=pal, nc=6, alpha=0.3, beta=0.7, hsel=good_sel, dsel=one,
             n_sel=3, mode=3, ann=None, mp=mp, hot=_hp(t_out), dot=one, out=one, status=one, scratch=ws, nbytes=need):
        return L.vti_overlay_frames(ctx, frames, ht, dt, B, masks, native, bases, cbytes, dets, xyxy, counts, offsets, max_det, cap,
                                    plates, pal, nc, alpha, beta, hsel, dsel, n_sel, mode, ann, mp, hot, dot, out, status, scratch,
                                    nbytes, None)

    assert call(ctx=None) == ARG
    for name in ("frames", "ht", "dt", "dets", "xyxy", "counts", "offsets", "pal", "hsel", "dsel", "hot", "dot", "out", "status", "scratch"):
        assert call(**{name: None}) == ARG, name
    assert call(masks=None) == ARG                                  # capacity > 0 needs the masks
    # an out-table row whose size differs from select[k]'s: names k
    assert call(hsel=(C.c_int32 * 3)(3, 1, 3)) == ARG
    assert b"row 1 of the out table" in err(), err()
    assert call(hsel=(C.c_int32 * 3)(3, 0, 0)) == ARG and b"row 2 of the out table" in err()
    # a table for another canvas, or for another B -- the input table and the out table alike
    other = vti_amd.Engine("n", 2, H=64, W=96, max_batch=4)
    other_canvas, _, _ = other.pack_frames(SHAPES, device="cpu")
    assert call(ht=_hp(other_canvas)) == ARG and b"another canvas" in err()
    assert call(B=3) == ARG and b"another B" in err()
    oc_out, _, _ = other.pack_frames([SHAPES[b] for b in sel], device="cpu")
    assert call(hot=_hp(oc_out)) == ARG and b"another canvas" in err()
    assert call(n_sel=2, hsel=(C.c_int32 * 2)(3, 0)) == ARG and b"another B" in err()      # out table of 3 rows, n_sel = 2
    assert call(hot=_hp(t_in)) == ARG                                # 4 rows
    assert call(n_sel=0) == ARG
    corrupt = t_in.host.clone()
    corrupt[64] = 1                                                  # row 0's byte offset is no longer a multiple of 16
    assert call(ht=C.c_void_p(corrupt.data_ptr())) == ARG and b"frame 0 of host_table" in err()
    corrupt = t_out.host.clone()
    corrupt[64 + 64] = 1                                             # row 1 of the out table
    assert call(hot=C.c_void_p(corrupt.data_ptr())) == ARG and b"frame 1 of host_table" in err() and b"out table" in err()
    # a selected frame of 8200 columns (the table allows 16384): names the frame
    wide = [(960, 1280), (480, 8200), (720, 960), (1080, 1920)]
    t_wide, _, _ = eng.pack_frames(wide, device="cpu")
    t_wide_out, _, _ = eng.pack_frames([wide[b] for b in (3, 1, 3)], device="cpu")
    assert call(ht=_hp(t_wide), hot=_hp(t_wide_out), hsel=(C.c_int32 * 3)(3, 1, 3), nbytes=1 << 40) == ARG
    assert b"frame 1" in err() and b"8192" in err(), err()
    assert call(ht=_hp(t_wide)) not in (ARG, UNSUPPORTED)           # ... the same table with that frame NOT selected is served
    # dev_mask_bases: given with native = 0, missing with native = 1; capacity_bytes
    assert call(bases=one) == ARG and b"dev_mask_bases" in err()
    assert call(native=1) == ARG and b"dev_mask_bases" in err()
    assert call(native=1, bases=one, cbytes=-1) == ARG and b"capacity_bytes" in err()
    assert call(cbytes=-1) == ARG and b"capacity_bytes" in err()
    assert call(native=1, bases=C.c_void_p(4096 + 4), cbytes=1 << 20) == ARG and b"dev_mask_bases" in err()
    assert call(native=2, bases=one) == ARG and call(native=-1) == ARG
    # BLEND without a picture, DRAW or BOTH with one
    assert call(mode=2) == ARG and b"dev_annotated" in err()
    assert call(mode=1, ann=one) == ARG and b"dev_annotated" in err()
    assert call(mode=3, ann=one) == ARG and b"dev_annotated" in err()
    for mode in (0, 4, -1, 7):
        assert call(mode=mode) == ARG and b"mode" in err()
    # misaligned buffers
    assert call(frames=C.c_void_p(4096 + 8)) == ARG and b"16-byte" in err()
    assert call(out=C.c_void_p(4096 + 8)) == ARG and b"16-byte" in err()
    assert call(mode=2, ann=C.c_void_p(4096 + 8)) == ARG and b"16-byte" in err()
    assert call(dt=C.c_void_p(4096 + 8)) == ARG and call(dot=C.c_void_p(4096 + 8)) == ARG
    assert call(masks=C.c_void_p(4096 + 8)) == ARG and b"16-byte" in err()           # letterbox bits
    assert call(native=1, bases=one, cbytes=1 << 20, masks=C.c_void_p(4096 + 4)) == ARG     # native rows: 8-byte aligned
    assert call(plates=C.c_void_p(4096 + 8)) == ARG and b"dev_plates" in err()
    assert call(dsel=C.c_void_p(4096 + 2)) == ARG and call(status=C.c_void_p(4096 + 2)) == ARG
    # a short or misaligned scratch
    assert call(nbytes=need - 1) == ARG and b"scratch smaller" in err()
    assert call(scratch=C.c_void_p((1 << 20) + 64)) == ARG and b"scratch" in err()
    # the selection and the other size rules of vti_overlay
    assert call(hsel=(C.c_int32 * 3)(3, -1, 3)) == ARG and b"host_select[1] = -1" in err()
    assert call(hsel=(C.c_int32 * 3)(3, 0, B)) == ARG and b"host_select[2] = 4" in err()
    assert call(max_det=1001) == ARG and call(max_det=0) == ARG and call(mp=-1) == ARG and call(cap=-1) == ARG
    for nc in (0, 17, -3):
        assert call(nc=nc) == ARG and b"n_colours" in err()
    for kw in (dict(alpha=float("nan")), dict(beta=float("inf"))):
        assert call(**kw) == ARG and b"finite" in err(), kw
    # what IS accepted up to the device check: without a GPU the call then stops with the HIP status, never with an argument error
    for kw in (dict(), dict(plates=None), dict(cap=0, masks=None), dict(mode=2, ann=one), dict(mode=2, ann=one, out=one), dict(mode=1),
               dict(native=1, bases=one, cbytes=1 << 20, masks=C.c_void_p(4096 + 8)), dict(native=1, bases=one, cbytes=0, masks=None),
               dict(hsel=(C.c_int32 * 3)(3, 0, 3)), dict(nc=16, pal=(C.c_uint8 * 48)())):
        assert call(**kw) not in (ARG, UNSUPPORTED), kw


def _fake_out(torch, B, max_det=8, cap=4):
    return dict(dets=torch.zeros((B, max_det, 38)), xyxy=torch.zeros((B, max_det, 4)), counts=torch.zeros(B, dtype=torch.int32),
                offsets=torch.zeros(B + 1, dtype=torch.int32), masks=torch.zeros((cap, 64, 8), dtype=torch.uint8))


def test_engine_overlay_with_a_table_refuses_bad_input_before_it_touches_a_device(lib_built):
    import torch
    vti_amd = lib_built
    eng = vti_amd.Engine("n", 2, H=64, W=64, max_batch=2)
    table, offs, total = eng.pack_frames([(48, 64), (32, 40)], device="cpu")
    out = _fake_out(torch, 2)
    buf = torch.zeros(total, dtype=torch.uint8)
    with pytest.raises(ValueError, match="flat uint8"):
        eng.overlay(torch.zeros((2, 48, 64, 3), dtype=torch.uint8), out, [0], table=table)      # a 4-D batch with a table
    with pytest.raises(ValueError, match="flat uint8"):
        eng.overlay(buf.view(1, -1), out, [0], table=table)
    with pytest.raises(ValueError, match="FrameTable"):
        eng.overlay(buf, out, [0], table=object())
    for sel in ([2], [-1], [], [0.5]):
        with pytest.raises(ValueError, match="select|frame index"):
            eng.overlay(buf, out, sel, table=table)
    with pytest.raises(ValueError, match="frames but an output set"):
        eng.overlay(buf, _fake_out(torch, 3), [0], table=table)
    # annotated: a flat buffer of the out table's size (here 3 * 32 * 40 and 3 * 48 * 64, each rounded up to 16)
    size = 3 * 32 * 40 + 3 * 48 * 64
    for wrong in (torch.zeros(size - 16, dtype=torch.uint8), torch.zeros(size + 16, dtype=torch.uint8),
                  torch.zeros((1, size), dtype=torch.uint8), torch.zeros(size, dtype=torch.int8)):
        with pytest.raises(ValueError, match=f"annotated must be a flat uint8 buffer of the out table's {size} bytes"):
            eng.overlay(buf, out, [1, 0], mode="blend", annotated=wrong, table=table)
    with pytest.raises(ValueError, match="annotated"):
        eng.overlay(buf, out, [1, 0], mode="both", annotated=torch.zeros(size, dtype=torch.uint8), table=table)
    with pytest.raises(ValueError, match="annotated"):
        eng.overlay(buf, out, [1, 0], mode="blend", table=table)
    # native rows of differing sizes are the ragged set: a flat buffer with its bases
    with pytest.raises(ValueError, match="mask_bases"):
        eng.overlay(buf, out, [0], native=True, table=table)
    ragged = dict(out, masks=torch.zeros(4096, dtype=torch.uint8), mask_bases=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="capacity_bytes"):
        eng.overlay(buf, ragged, [0], native=True, table=table, capacity_bytes=4097)
    with pytest.raises(ValueError, match="mask_bases and capacity_bytes"):
        eng.overlay(buf, out, [0], table=table, capacity_bytes=16)                              # letterbox masks take neither
    with pytest.raises(ValueError, match="mask_bases and capacity_bytes"):
        eng.overlay(torch.zeros((2, 48, 64, 3), dtype=torch.uint8), out, [0], mask_bases=ragged["mask_bases"])
    # a good call on host memory stops at the device check, in each form
    with pytest.raises(ValueError, match="device batch"):
        eng.overlay(buf, out, [1, 0], table=table)
    with pytest.raises(ValueError, match="device batch"):
        eng.overlay(buf, out, [1, 0], mode="blend", annotated=torch.zeros(size, dtype=torch.uint8), table=table)
    with pytest.raises(ValueError, match="device batch"):
        eng.overlay(buf, ragged, [1, 0], native=True, table=table)


def _fake_result(torch, vti_amd, eng, n, bits_shape, W, hw):
    from vti_amd.model import Boxes, Masks, Results
    data = torch.zeros((n, 6))
    data[:, 2:4] = 10.0
    r = Results(hw, {}, Boxes(data, hw), Masks(torch.zeros((n,) + bits_shape, dtype=torch.uint8), W, hw, eng), torch.zeros((n, 38)))
    r._engine = eng
    return r


def test_annotate_results_takes_a_canvas_sized_frame_in_either_mask_form_and_refuses_a_real_mix(lib_built):
    """A 640 x 640 frame on the 640 x 640 canvas has ONE mask layout, [n, 640, 80]: it sits in a letterbox list and in a frame-size list
    alike.  Without a device the accepted lists get as far as Engine.overlay's device check."""
    import torch
    vti_amd = lib_built
    O = vti_amd.overlay
    eng = vti_amd.Engine("n", 2, H=640, W=640, max_batch=2)
    frames = [np.zeros((640, 640, 3), np.uint8), np.zeros((480, 640, 3), np.uint8)]
    square = _fake_result(torch, vti_amd, eng, 2, (640, 80), 640, (640, 640))
    letterbox = _fake_result(torch, vti_amd, eng, 3, (640, 80), 640, (480, 640))
    native = _fake_result(torch, vti_amd, eng, 3, (480, 80), 640, (480, 640))
    for other in (letterbox, native):
        with pytest.raises(ValueError, match="device batch"):
            O.annotate_results(frames, [square, other], labels=False)
    with pytest.raises(ValueError, match="device batch"):
        O.annotate_results(frames[:1], [square], labels=False)
    three = frames + [np.zeros((480, 640, 3), np.uint8)]
    with pytest.raises(ValueError, match="mix letterbox masks and frame-size masks"):
        O.annotate_results(three, [square, letterbox, native], labels=False)
    with pytest.raises(ValueError, match="2 frames but 1 results"):
        O.annotate_results(frames, [square], labels=False)
    del native._engine
    with pytest.raises(RuntimeError, match="Engine"):
        O.annotate_results(frames, [square, native], labels=False)
