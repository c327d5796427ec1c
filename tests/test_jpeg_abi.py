"""vti_encode_jpeg's C ABI without a GPU: the three entry points exist, the two size functions, every argument check (all before the
first HIP call: fake pointers, never dereferenced), and process_frames(encode=...) refuses what it cannot serve before anything is
predicted.  The GPU parity tests are in test_gpu_jpeg.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_oracle_geometry import load_calib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vti_encode_jpeg_scratch_bytes", "vti_encode_jpeg_max_bytes", "vti_encode_jpeg")


def test_the_entry_points_are_declared_exported_and_bound(lib_built):
    vti_amd = lib_built
    hdr = open(os.path.join(ROOT, "include", "vti.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", vti_amd.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"\bT %s$" % name, exported, re.M), name
        assert name in vti_amd.SIGNATURES
    assert hasattr(vti_amd.Engine, "encode_jpeg") and hasattr(vti_amd.Engine, "encode_jpeg_scratch_bytes")
    assert "jpeg" in vti_amd.__all__ and callable(vti_amd.jpeg.encode)


def test_the_size_functions_are_zero_on_bad_arguments_and_grow(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    eng = vti_amd.Engine("n", 2, H=736, W=960, max_batch=1)
    f = lambda n=8, H0=960, W0=1280, ctx=eng._ctx: L.vti_encode_jpeg_scratch_bytes(ctx, n, H0, W0)
    g = lambda n=8, H0=960, W0=1280: L.vti_encode_jpeg_max_bytes(n, H0, W0)
    base = f()
    assert base > 0 and base % 256 == 0 and eng.encode_jpeg_scratch_bytes(8, 960, 1280) == base
    # per frame at least: the coefficients (3 B/px of the MCU-padded frame) and the longest scan (1658 bits per block)
    blocks = 60 * 80 * 6
    assert base >= 8 * (blocks * 128 + blocks * 1658 // 8)
    assert base < 8 * 3.2 * 3 * 960 * 1280                  # ... and below 1.7x the raw frame for the scan, plus what is listed in vti.h
    assert f(ctx=None) == 0
    for fn in (f, g):
        assert fn(n=0) == 0 and fn(n=-1) == 0 and fn(H0=0) == 0 and fn(W0=0) == 0 and fn(H0=8193) == 0 and fn(W0=8193) == 0
        assert fn(n=1, H0=8192, W0=8192) > 0 and fn(n=1, H0=1, W0=1) > 0
        for kw in ("n", "H0", "W0"):
            sizes = [fn(**{kw: v}) for v in (1, 2, 17, 64, 1000)]
            assert sizes == sorted(sizes) and sizes[0] < sizes[-1], (fn, kw, sizes)
    # the bound covers a file whose every scan byte is stuffed, plus header and EOI
    assert g(1, 16, 16) >= 623 + 2 + 2 * (6 * 1658 // 8)
    assert g(3, 50, 70) == 3 * g(1, 50, 70)
    # any real file fits: the noisiest frame at the highest quality
    noise = np.random.Generator(np.random.PCG64(0)).integers(0, 256, (50, 70, 3), dtype=np.uint8)
    assert len(vti_amd.jpeg.encode(noise, 100)) <= g(1, 50, 70)


def test_encode_jpeg_argument_checks_come_before_any_hip_call(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    eng = vti_amd.Engine("n", 2, H=736, W=960, max_batch=4)
    n, H0, W0 = 3, 135, 241
    need = eng.encode_jpeg_scratch_bytes(n, H0, W0)
    one, ws = C.c_void_p(4096 + 1), C.c_void_p(1 << 20)            # never dereferenced; frames and out at odd addresses are fine
    off = C.c_void_p(8192)

    def call(ctx=eng._ctx, frames=one, n=n, H0=H0, W0=W0, rgb=0, quality=95, scratch=ws, nbytes=need, offsets=off, out=one,
             max_bytes=1 << 20):
        return L.vti_encode_jpeg(ctx, frames, n, H0, W0, rgb, quality, scratch, nbytes, offsets, out, max_bytes, None)

    assert call(ctx=None) == -1
    for name, message in (("frames", b"null pointer"), ("offsets", b"null pointer"), ("out", b"null pointer"),
                          ("scratch", b"scratch must be a 256-byte aligned device pointer")):
        assert call(**{name: None}) == -1, name
        assert message in L.vti_last_error(eng._ctx), (name, L.vti_last_error(eng._ctx))
    assert call(n=0) == -1 and call(n=-1) == -1
    assert call(H0=0) == -1 and call(W0=0) == -1
    assert call(H0=8193, nbytes=1 << 40) == -1 and call(W0=8193, nbytes=1 << 40) == -1
    assert b"8192" in L.vti_last_error(eng._ctx)
    assert call(quality=0) == -1 and call(quality=101) == -1
    assert b"quality" in L.vti_last_error(eng._ctx)
    assert call(rgb=2) == -1 and call(rgb=-1) == -1
    assert call(nbytes=need - 1) == -1
    assert b"scratch smaller" in L.vti_last_error(eng._ctx)
    assert call(scratch=C.c_void_p((1 << 20) + 64)) == -1
    assert b"256-byte" in L.vti_last_error(eng._ctx)
    assert call(max_bytes=-1) == -1
    assert call(offsets=C.c_void_p(8192 + 4)) == -1
    # what IS accepted up to the device check: no output buffer when there is no room for one, every quality, rgb.  Without a GPU
    # the call then stops with the HIP status, never with VTI_ERR_ARG.
    for kw in (dict(out=None, max_bytes=0), dict(quality=1), dict(quality=100), dict(rgb=1), dict(n=1, H0=1, W0=1)):
        assert call(**kw) != -1, kw


def test_engine_encode_jpeg_refuses_bad_input_before_it_touches_a_device(lib_built):
    import torch
    vti_amd = lib_built
    eng = vti_amd.Engine("n", 2, H=64, W=64, max_batch=2)
    frames = torch.zeros((2, 48, 64, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="uint8"):
        eng.encode_jpeg(frames.float())
    with pytest.raises(ValueError, match="uint8"):
        eng.encode_jpeg(frames[0])
    for q in (0, 101):
        with pytest.raises(ValueError, match="quality"):
            eng.encode_jpeg(frames, quality=q)
    with pytest.raises(ValueError, match="max_bytes"):
        eng.encode_jpeg(frames, max_bytes=-1)
    with pytest.raises(ValueError, match="geometry"):
        eng.encode_jpeg(torch.zeros((1, 8193, 1, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="device"):              # a good call on host memory stops at the device check
        eng.encode_jpeg(frames)


def test_process_frames_refuses_a_bad_encode_before_anything_is_predicted(lib_built, monkeypatch):
    vti_amd = lib_built
    params = vti_amd.MeasureParams(*load_calib())
    model = vti_amd.YOLO(None, scale="n", nc=2, seed=3)

    def no_predict(*a, **k):
        raise AssertionError("predict was reached")
    monkeypatch.setattr(model, "_predict_outputs", no_predict)
    monkeypatch.setattr(model, "_predict_outputs_frames", no_predict)
    sm = vti_amd.StitchMeasurer(model, params)
    mc = vti_amd.MultiCameraMeasurer(model, [params, params])
    frames = np.zeros((2, 48, 64, 3), np.uint8)
    for kw in (dict(encode="jpeg"), dict(encode="png", annotate="all"), dict(encode="JPEG", annotate=[0]), dict(encode=True, annotate=[0]),
               dict(encode="jpeg", annotate=[0], jpeg_quality=0), dict(encode="jpeg", annotate=[0], jpeg_quality=101),
               dict(encode="jpeg", annotate=[0], jpeg_quality=95.5)):
        with pytest.raises(ValueError, match="encode|jpeg_quality"):
            sm.process_frames(frames, **kw)
        with pytest.raises(ValueError, match="encode|jpeg_quality"):
            mc.process_frames(frames, [0, 1], **kw)
    # the keywords sit at the end of both signatures
    import inspect
    for fn in (vti_amd.StitchMeasurer.process_frames, vti_amd.MultiCameraMeasurer.process_frames):
        names = list(inspect.signature(fn).parameters)
        assert names[-2:] == ["encode", "jpeg_quality"] and names[-3] == "annotate"
