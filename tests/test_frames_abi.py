"""Batches whose frames differ in size, without a GPU: the entry points exist, the frame table is validated when it is packed and
holds the oracle's letterbox geometry, every argument check of the *_frames calls comes before the first HIP call (fake pointers,
never dereferenced), and the Python surface refuses what it cannot serve before it touches a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from oracle.letterbox import letterbox_geometry
from test_oracle_geometry import load_calib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vti_frame_table_bytes", "vti_pack_frames", "vti_frame_table_info", "vti_letterbox_frames", "vti_scale_boxes_frames",
         "vti_predict_frames", "vti_measure_frames")
# H0 x W0 -> (new_h, new_w, top, left) on a 960 x 960 canvas: every branch of the letterbox
SIZES = [((960, 1280), (720, 960, 120, 0)), ((640, 640), (960, 960, 0, 0)), ((480, 640), (720, 960, 120, 0)),
         ((1080, 1920), (540, 960, 210, 0)), ((1920, 1920), (960, 960, 0, 0)), ((960, 960), (960, 960, 0, 0)),
         ((481, 333), (960, 665, 0, 147)), ((1200, 1600), (720, 960, 120, 0))]


def test_the_entry_points_are_declared_exported_and_bound(lib_built):
    vti_amd = lib_built
    hdr = open(os.path.join(ROOT, "include", "vti.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", vti_amd.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"\bT %s$" % name, exported, re.M), name
        assert name in vti_amd.SIGNATURES
    assert "FrameTable" in vti_amd.__all__
    for meth in ("pack_frames", "letterbox_frames", "predict_frames_into"):
        assert hasattr(vti_amd.Engine, meth)


def _packer(vti_amd, ctx, H=960, W=960):
    L = vti_amd.lib()

    def pack(H0, W0, off, total, B=None, out="alloc", nbytes=None, ctx=ctx, canvas=(H, W)):
        B = len(H0) if B is None else B
        a = (C.c_int32 * len(H0))(*H0) if H0 is not None else None
        b = (C.c_int32 * len(W0))(*W0) if W0 is not None else None
        o = (C.c_int64 * len(off))(*off) if off is not None else None
        size = max(int(L.vti_frame_table_bytes(max(B, 1))), 1)
        buf = (C.c_uint8 * size)(*([0xA5] * size)) if out == "alloc" else out
        rc = L.vti_pack_frames(ctx, canvas[0], canvas[1], a, b, o, B, total, buf, size if nbytes is None else nbytes)
        return rc, (bytes(buf) if buf is not None else None)
    return pack


def test_pack_frames_validates_every_entry_and_is_deterministic(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    eng = vti_amd.Engine("n", 2, H=960, W=960, max_batch=4)
    pack = _packer(vti_amd, eng._ctx)
    one = L.vti_frame_table_bytes(1)
    row = L.vti_frame_table_bytes(2) - one
    assert L.vti_frame_table_bytes(0) == 0 and L.vti_frame_table_bytes(-2) == 0
    assert one > row > 0 and row % 16 == 0 and one % 16 == 0 and L.vti_frame_table_bytes(7) == one + 6 * row
    good = dict(H0=[960, 481, 1080], W0=[1280, 333, 1920])
    sizes = [3 * h * w for h, w in zip(good["H0"], good["W0"])]
    off = [0, (sizes[0] + 15) & ~15]
    off.append((off[1] + sizes[1] + 15) & ~15)
    total = off[2] + sizes[2]
    rc, a = pack(good["H0"], good["W0"], off, total)
    assert rc == 0
    rc, b = pack(good["H0"], good["W0"], off, total)
    assert rc == 0 and a == b                                      # equal inputs, equal bytes (padding included)
    assert 0xA5 not in (a[one - row + 60], a[one - 1])               # the pad words were written (zero), not left as found
    rc, c = pack(good["H0"][::-1], good["W0"][::-1], off, total + (1 << 24))
    assert rc == 0 and c != a
    hd = (C.c_int32 * 8)()
    buf = (C.c_uint8 * len(a)).from_buffer_copy(a)
    assert L.vti_frame_table_info(buf, -1, hd, None) == 0
    assert list(hd[:5]) == [3, 960, 960, 1080, 1920] and (hd[6] & 0xFFFFFFFF) | (hd[7] << 32) == total
    assert L.vti_frame_table_info(buf, 3, hd, None) == -1 and L.vti_frame_table_info(buf, -2, hd, None) == -1
    assert L.vti_frame_table_info(None, 0, hd, None) == -1

    def variants(k):
        H0, W0, o = list(good["H0"]), list(good["W0"]), list(off)
        for name, (h, w, d, t) in {
                "H0 = 0": (0, W0[k], o[k], total), "W0 = 0": (H0[k], 0, o[k], total), "H0 < 0": (-5, W0[k], o[k], total),
                "H0 above the limit": (16385, 4, o[k], 1 << 40), "W0 above the limit": (4, 16385, o[k], 1 << 40),
                "misaligned offset": (H0[k], W0[k], o[k] + 8, total + 64), "negative offset": (H0[k], W0[k], -16, total),
                "past total_bytes": (H0[k], W0[k], o[k], o[k] + 3 * H0[k] * W0[k] - 1),
                "resized below 1 px": (16000, 3, o[k], 1 << 40)}.items():
            hh, ww, oo = list(H0), list(W0), list(o)
            hh[k], ww[k], oo[k] = h, w, d
            yield name, hh, ww, oo, t

    for k in range(3):
        for name, hh, ww, oo, t in variants(k):
            # ("past total_bytes" cuts the buffer inside frame k: later frames fail too, the FIRST failing index is named)
            rc, _ = pack(hh, ww, oo, t)
            assert rc == -1, (name, k)
            msg = L.vti_last_error(eng._ctx)
            assert b"frame %d:" % k in msg, (name, k, msg)
            assert pack(hh, ww, oo, t, ctx=None)[0] == -1          # a NULL ctx only loses the text
    assert pack(None, good["W0"], off, total, B=3)[0] == -1 and pack(good["H0"], None, off, total, B=3)[0] == -1
    assert pack(good["H0"], good["W0"], None, total, B=3)[0] == -1
    assert pack(good["H0"], good["W0"], off, total, out=None)[0] == -1
    assert pack(good["H0"], good["W0"], off, total, B=0)[0] == -1 and pack(good["H0"], good["W0"], off, total, B=-1)[0] == -1
    assert pack(good["H0"], good["W0"], off, total, nbytes=one + 2 * row - 1)[0] == -1
    assert b"vti_frame_table_bytes" in L.vti_last_error(eng._ctx)
    assert pack(good["H0"], good["W0"], off, total, canvas=(960, 950))[0] == -1
    rc, d = pack(good["H0"], good["W0"], off, total, ctx=None)
    assert rc == 0 and d == a


def test_rows_hold_the_oracle_geometry_for_the_eight_sizes(lib_built):
    vti_amd = lib_built
    eng = vti_amd.Engine("n", 2, H=960, W=960, max_batch=8)
    shapes = [s for s, _ in SIZES]
    table, offs, total = eng.pack_frames(shapes, device="cpu")
    assert table.B == 8 and (table.max_H0, table.max_W0) == (1920, 1920) and (table.H, table.W) == (960, 960)
    end = 0
    for b, ((H0, W0), want) in enumerate(SIZES):
        g = letterbox_geometry(H0, W0, (960, 960), auto=False)
        assert (g["new_h"], g["new_w"], g["top"], g["left"]) == want and (g["H"], g["W"]) == (960, 960)
        r = table.row(b)
        assert (r["H0"], r["W0"], r["new_h"], r["new_w"], r["top"], r["left"]) == (H0, W0) + want, (b, r)
        assert r["offset"] == offs[b] and offs[b] % 16 == 0 and offs[b] >= end
        end = offs[b] + 3 * H0 * W0
        assert r["scale_x"] == 1.0 / (g["new_w"] / W0) and r["scale_y"] == 1.0 / (g["new_h"] / H0)
        gain = min(960 / H0, 960 / W0)                              # scale_boxes: double, then one cast to f32
        assert r["gain"] == float(np.float32(gain))
        assert r["padx"] == float(np.float32(round((960 - W0 * gain) / 2 - 0.1)))
        assert r["pady"] == float(np.float32(round((960 - H0 * gain) / 2 - 0.1)))
    assert total >= end
    # a rectangular canvas, imgsz=(h, w) likewise
    eng2 = vti_amd.Engine("n", 2, H=736, W=960, max_batch=2)
    t2, _, _ = eng2.pack_frames([(960, 1280), (481, 333)], device="cpu")
    for b, (H0, W0) in enumerate([(960, 1280), (481, 333)]):
        g, r = letterbox_geometry(H0, W0, (736, 960), auto=False), t2.row(b)
        assert (r["new_h"], r["new_w"], r["top"], r["left"]) == (g["new_h"], g["new_w"], g["top"], g["left"])
    with pytest.raises(vti_amd.VtiError, match="frame 1"):
        eng.pack_frames([(960, 960), (0, 5)], device="cpu")
    with pytest.raises(ValueError):
        eng.pack_frames([], device="cpu")


def _tables(vti_amd):
    eng = vti_amd.Engine("n", 2, H=64, W=64, max_batch=4)
    shapes = [(48, 64), (64, 40), (100, 130)]
    t, _, _ = eng.pack_frames(shapes, device="cpu")
    other_canvas, _, _ = vti_amd.Engine("n", 2, H=64, W=96, max_batch=4).pack_frames(shapes, device="cpu")
    other_b, _, _ = eng.pack_frames(shapes[:2], device="cpu")
    return eng, t, other_canvas, other_b


def test_every_argument_check_of_the_frames_calls_runs_without_a_gpu(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    eng, t, other_canvas, other_b = _tables(vti_amd)
    host = lambda x: C.c_void_p(x.host.data_ptr())
    one, ws = C.c_void_p(4096), C.c_void_p(1 << 20)               # never dereferenced
    B, max_det, cap = 3, 10, 20
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

    def lb(ctx=eng._ctx, frames=one, host_table=host(t), dev_table=one, B=B, out=one):
        return L.vti_letterbox_frames(ctx, frames, host_table, dev_table, B, out, None)
    table_checks(lb)
    assert lb(frames=None) == -1 and lb(out=None) == -1
    assert lb(frames=C.c_void_p(4096 + 4)) == -1 and lb(out=C.c_void_p(4096 + 2)) == -1
    small = vti_amd.Engine("n", 2, H=64, W=64, max_batch=2)
    assert L.vti_letterbox_frames(small._ctx, one, host(t), one, B, one, None) == -1

    def sb(ctx=eng._ctx, dets=one, counts=one, host_table=host(t), dev_table=one, B=B, max_det=max_det, xyxy=one):
        return L.vti_scale_boxes_frames(ctx, dets, counts, host_table, dev_table, B, max_det, xyxy, None)
    table_checks(sb)
    assert sb(dets=None) == -1 and sb(counts=None) == -1 and sb(xyxy=None) == -1 and sb(max_det=0) == -1
    assert sb(xyxy=C.c_void_p(4096 + 4)) == -1

    def pr(ctx=eng._ctx, frames=one, host_table=host(t), dev_table=one, B=B, mode=0, scratch=one, xyxy=one, max_det=max_det):
        return L.vti_predict_frames(ctx, frames, host_table, dev_table, B, 0, 0.25, 0.7, max_det, 0, mode, 1, scratch, one, one, one,
                                    one, one, cap, one, xyxy, None)
    table_checks(pr)
    assert pr(mode=vti_amd._lib.VTI_MASK_NATIVE) == -6 and pr(mode=vti_amd._lib.VTI_MASK_NATIVE | 1) == -6
    assert b"VTI_MASK_NATIVE" in err()
    assert pr(frames=None) == -1 and pr(scratch=None) == -1 and pr(frames=C.c_void_p(4096 + 8)) == -1
    assert pr(max_det=0) == -1
    assert pr() == -2 and b"weights not loaded" in err()          # every argument was accepted; no device has been touched

    need = eng.measure_scratch_bytes(B, cap, t.max_W0)
    assert need > eng.measure_scratch_bytes(B, cap, 64)

    def ms(ctx=eng._ctx, cams=one, n_cams=2, index=one, masks=one, native=0, dets=one, host_table=host(t), dev_table=one, B=B,
           max_det=max_det, cap=cap, scratch=ws, nbytes=need, frame_f64=one):
        return L.vti_measure_frames(ctx, cams, n_cams, index, masks, native, dets, one, one, one, host_table, dev_table, B, max_det,
                                    cap, scratch, nbytes, frame_f64, one, None, None, None)
    table_checks(ms)
    assert ms(cams=None) == -1 and ms(index=None) == -1 and ms(n_cams=0) == -1
    assert ms(cams=C.c_void_p(4096 + 8)) == -1 and ms(index=C.c_void_p(4096 + 2)) == -1
    assert ms(nbytes=need - 1) == -1 and b"scratch" in err()      # one byte short for the LARGEST W0 of the table
    assert ms(nbytes=eng.measure_scratch_bytes(B, cap, 64)) == -1
    assert ms(scratch=C.c_void_p(4096 + 64)) == -1 and ms(scratch=None) == -1
    assert ms(native=1) == -6 and ms(native=2) == -1
    assert ms(masks=C.c_void_p(4096 + 8)) == -1 and ms(masks=None) == -1 and ms(dets=None) == -1 and ms(frame_f64=None) == -1
    assert ms(max_det=0) == -1 and ms(cap=-1) == -1
    assert ms(max_det=vti_amd._lib.VTI_MEASURE_MAX_DET + 1) == -6


def test_python_surface_refuses_before_touching_a_device(lib_built):
    import torch
    vti_amd = lib_built
    frames = [np.zeros((48, 64, 3), np.uint8), np.zeros((64, 40, 3), np.uint8)]
    model = vti_amd.YOLO(None, scale="n", nc=2)
    with pytest.raises(ValueError, match="retina_masks"):
        model.predict(frames, retina_masks=True, imgsz=64)
    assert not model._engines                                     # nothing was built, nothing uploaded
    with pytest.raises(ValueError, match="HxWx3"):
        model.predict([np.zeros((48, 64, 3), np.uint8), np.zeros((64, 40), np.uint8)], imgsz=64)
    p = vti_amd.MeasureParams(*load_calib())
    with pytest.raises(ValueError, match="retina_masks"):
        vti_amd.MultiCameraMeasurer(model, [p]).process_frames(frames, [0, 0], imgsz=64, retina_masks=True)
    eng, t, other_canvas, other_b = _tables(vti_amd)
    out = dict(dets=torch.zeros((3, 10, 38)), xyxy=torch.zeros((3, 10, 4)), counts=torch.zeros(3, dtype=torch.int32),
               offsets=torch.zeros(4, dtype=torch.int32), masks=torch.zeros((0, 64, 8), dtype=torch.uint8))
    row = int(vti_amd.lib().vti_measure_cameras_bytes(1))
    cams = torch.zeros(2 * row, dtype=torch.uint8)
    with pytest.raises(ValueError, match="canvas"):
        eng.measure(out, cams, cameras=[0, 1, 0], frames=other_canvas)
    with pytest.raises(ValueError, match="3"):
        eng.measure(out, cams, cameras=[0, 1, 0], frames=other_b)
    with pytest.raises(ValueError, match="native"):
        eng.measure(out, cams, cameras=[0, 1, 0], frames=t, native=True)
    with pytest.raises(ValueError):
        eng.measure(out, cams, 48, 64, cameras=[0, 1, 0], frames=t)
    with pytest.raises(ValueError):
        eng.measure(out, cams, cameras=[0, 2, 0], frames=t)          # camera index outside the table
    with pytest.raises(ValueError):
        eng.measure(out, cams, cameras=[0, 1, 0], frames=object())
    with pytest.raises(ValueError):
        eng.measure(out, cams, cameras=[0, 1, 0])                    # neither H0, W0 nor frames
    with pytest.raises(ValueError):
        eng.scale_boxes(out["dets"], out["counts"], frames=other_b)
    with pytest.raises(ValueError):
        eng.letterbox_frames(torch.zeros(16, dtype=torch.uint8), t)  # buffer shorter than total_bytes
