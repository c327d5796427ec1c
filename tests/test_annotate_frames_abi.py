"""vti_annotate_frames' C ABI without a GPU: the two entry points exist, the scratch size is vti_annotate's at the largest selected
frame, every refusal comes before the first HIP call (fake pointers, never dereferenced; without a GPU a call that reaches HIP
ends with the HIP status instead), and process_frames keeps refusing a mixed list unless mixed=True.  The GPU parity tests are in
test_gpu_annotate_frames.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_oracle_geometry import load_calib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vti_annotate_frames_scratch_bytes", "vti_annotate_frames")
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
        assert name in vti_amd.SIGNATURES
    assert "not supported" not in hdr[hdr.index("process_frame's annotated frame on device"):hdr.index("vti_annotate_scratch_bytes(")]


def test_scratch_bytes_is_vti_annotates_at_the_largest_selected_frame(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    eng = vti_amd.Engine("n", 2, H=736, W=960, max_batch=4)
    f = lambda t, max_det=200, mp=4096, ctx=eng._ctx: L.vti_annotate_frames_scratch_bytes(ctx, _hp(t) if t is not None else None, max_det, mp)
    for sel in ([0, 1, 2, 3], [1, 2], [1], [3, 3, 0], [2, 1, 1]):
        shapes = [SHAPES[b] for b in sel]
        t, _, _ = eng.pack_frames(shapes, device="cpu")
        mh, mw = max(h for h, _ in shapes), max(w for _, w in shapes)       # the largest H0 and W0 need not be of one frame
        want = eng.annotate_scratch_bytes(len(sel), 200, mh, mw, 4096)
        assert want > 0 and f(t) == want, (sel, f(t), want)
    t, _, _ = eng.pack_frames(SHAPES, device="cpu")
    assert f(t, ctx=None) == 0 and f(None) == 0 and f(t, max_det=0) == 0 and f(t, max_det=1001) == 0 and f(t, mp=-1) == 0
    big, _, _ = eng.pack_frames([(8200, 480)], device="cpu")                # the table allows it, the raster does not
    assert f(big) == 0
    junk = np.zeros(256, np.uint8)
    assert L.vti_annotate_frames_scratch_bytes(eng._ctx, C.c_void_p(junk.ctypes.data), 200, 4096) == 0


def test_every_refusal_comes_before_any_hip_call(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    eng = vti_amd.Engine("n", 2, H=736, W=960, max_batch=4)
    B, max_det, cap, mp = 4, 200, 800, 4096
    sel = [3, 0, 3]
    t_in, _, _ = eng.pack_frames(SHAPES, device="cpu")
    t_out, _, _ = eng.pack_frames([SHAPES[b] for b in sel], device="cpu")
    need = L.vti_annotate_frames_scratch_bytes(eng._ctx, _hp(t_out), max_det, mp)
    one, ws = C.c_void_p(4096), C.c_void_p(1 << 20)                # never dereferenced
    good_sel = (C.c_int32 * 3)(*sel)
    err = lambda: L.vti_last_error(eng._ctx)

    def call(ctx=eng._ctx, frames=one, ht=_hp(t_in), dt=one, B=B, cams=one, n_cams=2, cof=one, masks=one, native=0, dets=one, xyxy=one,
             counts=one, offsets=one, max_det=max_det, cap=cap, fi=one, sf=one, si=one, hsel=good_sel, dsel=one, n_sel=3, mp=mp,
             hot=_hp(t_out), dot=one, out=one, status=one, scratch=ws, nbytes=need):
        return L.vti_annotate_frames(ctx, frames, ht, dt, B, cams, n_cams, cof, masks, native, dets, xyxy, counts, offsets, max_det, cap,
                                     fi, sf, si, hsel, dsel, n_sel, mp, hot, dot, out, status, scratch, nbytes, None)

    assert call(ctx=None) == ARG
    # NULL pointers
    for name in ("frames", "ht", "dt", "cams", "dets", "xyxy", "counts", "offsets", "fi", "sf", "si", "hsel", "dsel", "hot", "dot", "out",
                 "status", "scratch"):
        assert call(**{name: None}) == ARG, name
    assert call(masks=None) == ARG                                  # capacity > 0 needs the masks
    # a table for another canvas, or for another B -- the input table and the out table alike
    other_canvas, _, _ = vti_amd.Engine("n", 2, H=64, W=96, max_batch=4).pack_frames(SHAPES, device="cpu")
    assert call(ht=_hp(other_canvas)) == ARG and b"another canvas" in err()
    assert call(B=3) == ARG and b"another B" in err()
    oc_out, _, _ = vti_amd.Engine("n", 2, H=64, W=96, max_batch=4).pack_frames([SHAPES[b] for b in sel], device="cpu")
    assert call(hot=_hp(oc_out)) == ARG and b"another canvas" in err()
    assert call(n_sel=2, hsel=(C.c_int32 * 2)(3, 0)) == ARG and b"another B" in err()      # out table of 3 rows, n_sel = 2
    assert call(hot=_hp(t_in)) == ARG                                # 4 rows
    assert call(n_sel=0) == ARG
    corrupt = t_in.host.clone()
    corrupt[64] = 1                                                  # row 0's byte offset is no longer a multiple of 16
    assert call(ht=C.c_void_p(corrupt.data_ptr())) == ARG and b"frame 0 of host_table" in err()
    assert call(dt=C.c_void_p(4096 + 8)) == ARG and call(dot=C.c_void_p(4096 + 8)) == ARG
    # a short or misaligned scratch
    assert call(nbytes=need - 1) == ARG and b"scratch smaller" in err()
    assert call(scratch=C.c_void_p((1 << 20) + 64)) == ARG
    # native masks
    assert call(native=1) == UNSUPPORTED and b"native" in err()
    assert call(native=2) == ARG
    # a selection outside [0, B)
    assert call(hsel=(C.c_int32 * 3)(3, -1, 3)) == ARG and b"host_select[1] = -1" in err()
    assert call(hsel=(C.c_int32 * 3)(3, 0, B)) == ARG and b"host_select[2] = 4" in err()
    # out-table row k of another size than input row select[k]: names k
    assert call(hsel=(C.c_int32 * 3)(3, 1, 3)) == ARG
    assert b"row 1 of the out table" in err(), err()
    assert call(hsel=(C.c_int32 * 3)(3, 0, 0)) == ARG and b"row 2 of the out table" in err()
    # a selected frame above 8192 (the table allows 16384): names the frame
    wide = [(960, 1280), (8200, 480), (720, 960), (1080, 1920)]
    t_wide, _, _ = eng.pack_frames(wide, device="cpu")
    t_wide_out, _, _ = eng.pack_frames([wide[b] for b in (3, 1, 3)], device="cpu")
    assert call(ht=_hp(t_wide), hot=_hp(t_wide_out), hsel=(C.c_int32 * 3)(3, 1, 3), nbytes=1 << 40) == ARG
    assert b"frame 1" in err() and b"8192" in err(), err()
    # ... while the same table with that frame NOT selected is served
    assert call(ht=_hp(t_wide)) not in (ARG, UNSUPPORTED)
    # the other size and alignment rules of vti_annotate
    assert call(max_det=1001) == ARG and call(max_det=0) == ARG and call(mp=-1) == ARG and call(n_cams=0) == ARG and call(cap=-1) == ARG
    assert call(masks=C.c_void_p(4096 + 8)) == ARG and call(cams=C.c_void_p(4096 + 8)) == ARG and call(dsel=C.c_void_p(4096 + 2)) == ARG
    assert call(frames=C.c_void_p(4096 + 8)) == ARG and call(out=C.c_void_p(4096 + 8)) == ARG
    # what IS accepted up to the device check: without a GPU the call then stops with the HIP status, never with an argument error
    for kw in (dict(), dict(cof=None), dict(cap=0, masks=None), dict(hsel=(C.c_int32 * 3)(3, 0, 3))):
        assert call(**kw) not in (ARG, UNSUPPORTED), kw


def _fake_out(torch, B, max_det=8, cap=4):
    return dict(dets=torch.zeros((B, max_det, 38)), xyxy=torch.zeros((B, max_det, 4)), counts=torch.zeros(B, dtype=torch.int32),
                offsets=torch.zeros(B + 1, dtype=torch.int32), masks=torch.zeros((cap, 64, 8), dtype=torch.uint8))


def test_engine_annotate_with_a_table_refuses_bad_input_before_it_touches_a_device(lib_built):
    import torch
    vti_amd = lib_built
    eng = vti_amd.Engine("n", 2, H=64, W=64, max_batch=2)
    table, _, total = eng.pack_frames([(48, 64), (32, 40)], device="cpu")
    out = _fake_out(torch, 2)
    meas = dict(frame_i32=torch.zeros((2, 6), dtype=torch.int32), stitch_f64=torch.zeros((4, 7), dtype=torch.float64),
                stitch_i32=torch.zeros((4, 2), dtype=torch.int32))
    params = vti_amd.MeasureParams(*load_calib())
    buf = torch.zeros(total, dtype=torch.uint8)
    with pytest.raises(ValueError, match="flat uint8"):
        eng.annotate(buf.view(1, -1), out, meas, params, [0], table=table)
    with pytest.raises(ValueError, match="native"):
        eng.annotate(buf, out, meas, params, [0], native=True, table=table)
    with pytest.raises(ValueError, match="FrameTable"):
        eng.annotate(buf, out, meas, params, [0], table=object())
    for sel in ([2], [-1], [], [0.5]):
        with pytest.raises(ValueError, match="select|frame index"):
            eng.annotate(buf, out, meas, params, sel, table=table)
    with pytest.raises(ValueError, match="frames but an output set"):
        eng.annotate(buf, _fake_out(torch, 3), meas, params, [0], table=table)
    with pytest.raises(ValueError, match="device batch"):              # a good call on host memory stops at the device check
        eng.annotate(buf, out, meas, params, [1, 0], table=table)


def test_process_frames_keeps_the_refusal_and_checks_mixed(lib_built, monkeypatch):
    vti_amd = lib_built
    params = vti_amd.MeasureParams(*load_calib())
    model = vti_amd.YOLO(None, scale="n", nc=2, seed=3)

    def no_predict(*a, **k):
        raise AssertionError("predict was reached")
    monkeypatch.setattr(model, "_predict_outputs", no_predict)
    monkeypatch.setattr(model, "_predict_outputs_frames", no_predict)
    sm = vti_amd.StitchMeasurer(model, params)
    mc = vti_amd.MultiCameraMeasurer(model, [params, params])
    a, b = np.zeros((48, 64, 3), np.uint8), np.zeros((32, 64, 3), np.uint8)
    # the default is today's refusal, word for word
    text = re.escape("process_frames: annotate needs frames of one size; the frames of this list differ in shape "
                     "(vti_annotate has no frame-table form)")
    with pytest.raises(ValueError, match=text):
        sm.process_frames([a, b], annotate="all")
    with pytest.raises(ValueError, match=text):
        mc.process_frames([a, b], [0, 1], annotate=[0], mixed=False)
    # mixed=True does not lift the other refusals
    with pytest.raises(ValueError, match="encode needs annotate"):
        sm.process_frames([a, b], encode="jpeg", mixed=True)
    with pytest.raises(ValueError, match="encode needs annotate"):
        mc.process_frames([a, b], [0, 1], encode="jpeg", mixed=True)
    with pytest.raises(ValueError, match="retina_masks=True needs frames of one size"):
        sm.process_frames([a, b], annotate="all", retina_masks=True, mixed=True)
    # mixed is a bool, and keyword only
    for bad in ("yes", 1, None):
        with pytest.raises(ValueError, match="mixed must be True or False"):
            sm.process_frames([a, b], annotate="all", mixed=bad)
        with pytest.raises(ValueError, match="mixed must be True or False"):
            mc.process_frames([a, b], [0, 1], annotate="all", mixed=bad)
    with pytest.raises(TypeError):
        sm.process_frames([a, b], 0.2, 0.25, 200, 960, False, "all", None, 95, True)
    # with mixed=True the list gets past the refusal, as far as the predict
    with pytest.raises(AssertionError, match="predict was reached"):
        sm.process_frames([a, b], annotate="all", mixed=True)
    with pytest.raises(AssertionError, match="predict was reached"):
        mc.process_frames([a, b], [0, 1], annotate=[1], encode="jpeg", mixed=True)
    # the flag is an argument all the way down: nothing of it stays on the measurer, and the signature is the old one
    import inspect
    assert not hasattr(sm, "_mixed") and not hasattr(mc, "_mixed")
    from vti_amd.measure import _DeviceStage
    assert "mixed" in inspect.signature(_DeviceStage._frame_records).parameters
    assert "mixed" in inspect.signature(vti_amd.StitchMeasurer._process_frames).parameters
