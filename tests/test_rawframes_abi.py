"""vti_convert_raw's C ABI without a GPU: the five entry points exist; vti_raw_frame_bytes and vti_pack_raw_frames (host only) size,
refuse and lay out as documented; every argument check of the launching calls, both tables revalidated row by row included, comes
before the first HIP call (a context without weights, fake device pointers that are never dereferenced); the RawFrames
constructor's errors.  The GPU parity tests are in test_gpu_rawframes.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vti_raw_frame_bytes", "vti_convert_raw", "vti_raw_table_bytes", "vti_pack_raw_frames", "vti_convert_raw_frames")
ARG = -1
SHAPES = [(6, 10), (34, 66), (2, 2), (18, 34), (64, 130)]
FMTS = [0, 2, 4, 1, 5]


def _i32(v):
    return (C.c_int32 * len(v))(*v)


def _err(L, eng):
    return L.vti_last_error(eng._ctx).decode()


def test_the_entry_points_are_declared_exported_and_bound(lib_built):
    vti_amd = lib_built
    hdr = open(os.path.join(ROOT, "include", "vti.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", vti_amd.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"\bT %s$" % name, exported, re.M), name
        assert name in vti_amd.SIGNATURES
    assert re.search(r"enum \{ VTI_RAW_YUYV = 0, VTI_RAW_UYVY, VTI_RAW_NV12, VTI_RAW_NV21, VTI_RAW_I420, VTI_RAW_YV12 \}", hdr)
    assert vti_amd.rawframes.FORMATS == {"yuyv": 0, "uyvy": 1, "nv12": 2, "nv21": 3, "i420": 4, "yv12": 5}
    for name in ("convert_raw", "pack_raw_frames", "convert_raw_frames"):
        assert callable(getattr(vti_amd.Engine, name))
    assert vti_amd.RawFrames is not None and "RawFrames" in vti_amd.__all__


def test_raw_frame_bytes_values_and_refusals(lib_built):
    L = lib_built.lib()
    R = lib_built.rawframes
    for f in range(6):
        for h, w in SHAPES + [(960, 1280), (8192, 8192), (2, 8192)]:
            assert L.vti_raw_frame_bytes(f, h, w) == (2 * h * w if f < 2 else h * w * 3 // 2) == R.frame_bytes(f, h, w)
        for h, w in ((4, 5), (0, 4), (4, 0), (1, 4), (-4, 4), (4, -4), (8194, 4), (4, 8194)):
            assert L.vti_raw_frame_bytes(f, h, w) == 0, (f, h, w)
        assert (L.vti_raw_frame_bytes(f, 5, 6) == 0) == (f >= 2)          # an odd height only for 4:2:2
    for f in (-1, 6, 100):
        assert L.vti_raw_frame_bytes(f, 4, 6) == 0
    assert L.vti_raw_frame_bytes(0, 960, 1280) == 2457600 and L.vti_raw_frame_bytes(2, 960, 1280) == 1843200
    assert L.vti_raw_table_bytes(0) == 0 and L.vti_raw_table_bytes(-1) == 0 and L.vti_raw_table_bytes(4097) == 0
    assert L.vti_raw_table_bytes(1) > 0 and L.vti_raw_table_bytes(4096) > L.vti_raw_table_bytes(4095)


def _pack(L, ctx, shapes=SHAPES, fmts=FMTS):
    n = len(shapes)
    nb = int(L.vti_raw_table_bytes(n))
    table = np.zeros(nb, np.uint8)
    off = np.full(n + 1, -1, np.int64)
    rc = L.vti_pack_raw_frames(ctx, _i32([h for h, _ in shapes]), _i32([w for _, w in shapes]), _i32(fmts), n, table.ctypes.data, nb,
                               off.ctypes.data)
    return rc, table, off


def test_pack_raw_frames_offsets_and_refusals(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    eng = vti_amd.Engine("n", 2, H=64, W=64, max_batch=5)
    rc, table, off = _pack(L, eng._ctx)
    assert rc == 0
    want, at = [], 0
    for (h, w), f in zip(SHAPES, FMTS):          # back to back, each at a multiple of 16 bytes; [n] is the buffer's size
        want.append(at)
        at = (at + int(L.vti_raw_frame_bytes(f, h, w)) + 15) & ~15
    assert off.tolist() == want + [at] and all(o % 16 == 0 for o in off)
    rc2, table2, _ = _pack(L, eng._ctx)
    assert rc2 == 0 and np.array_equal(table, table2)                    # equal inputs, equal bytes
    assert _pack(L, None)[0] == 0                                        # ctx only receives the text
    n = len(SHAPES)
    nb = table.size
    h, w, f, o = _i32([s[0] for s in SHAPES]), _i32([s[1] for s in SHAPES]), _i32(FMTS), (C.c_int64 * (n + 1))()
    for args in ((None, w, f, n, table.ctypes.data, nb, o), (h, None, f, n, table.ctypes.data, nb, o), (h, w, None, n, table.ctypes.data, nb, o),
                 (h, w, f, n, None, nb, o), (h, w, f, n, table.ctypes.data, nb, None)):
        assert L.vti_pack_raw_frames(eng._ctx, *args) == ARG
        assert "null pointer" in _err(L, eng)
    assert L.vti_pack_raw_frames(eng._ctx, h, w, f, 0, table.ctypes.data, nb, o) == ARG
    assert L.vti_pack_raw_frames(eng._ctx, h, w, f, -1, table.ctypes.data, nb, o) == ARG
    assert L.vti_pack_raw_frames(eng._ctx, h, w, f, 4097, table.ctypes.data, nb, o) == ARG
    assert L.vti_pack_raw_frames(eng._ctx, h, w, f, n, table.ctypes.data, nb - 1, o) == ARG and "table smaller" in _err(L, eng)
    for k, shape, fmt in ((3, (18, 33), 1), (1, (33, 66), 2), (4, (64, 130), 6), (0, (6, 10), -1), (2, (0, 2), 4), (2, (2, 8194), 4)):
        shapes, fmts = list(SHAPES), list(FMTS)
        shapes[k], fmts[k] = shape, fmt
        rc, _, _ = _pack(L, eng._ctx, shapes, fmts)
        assert rc == ARG and f"frame {k}:" in _err(L, eng), (k, _err(L, eng))      # the failing index
    with pytest.raises(vti_amd.VtiError, match="frame 1"):
        eng.pack_raw_frames([(6, 10), (5, 6)], ["yuyv", "nv12"], device="cpu")
    with pytest.raises(ValueError, match="formats"):
        eng.pack_raw_frames([(6, 10), (4, 6)], ["yuyv"], device="cpu")
    with pytest.raises(ValueError, match="unknown raw format"):
        eng.pack_raw_frames([(6, 10)], "rgb", device="cpu")
    rt = eng.pack_raw_frames(SHAPES, FMTS, device="cpu")                # the wrapper reports the same layout
    assert rt.raw_offsets == want and rt.raw_bytes == at and np.array_equal(rt.host.numpy(), table)


def test_convert_raw_argument_checks_come_before_any_hip_call(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    eng = vti_amd.Engine("n", 2, H=64, W=64, max_batch=1)        # no weights, no device
    src, dst = C.c_void_p(4096 + 1), C.c_void_p((1 << 20) + 3)   # any byte address

    def call(ctx=eng._ctx, raw=src, fmt=0, B=3, H0=6, W0=10, rgb=0, out=dst):
        return L.vti_convert_raw(ctx, raw, fmt, B, H0, W0, rgb, out, None)
    assert call(ctx=None) == ARG
    assert call(raw=None) == ARG and "null pointer" in _err(L, eng)
    assert call(out=None) == ARG and "null pointer" in _err(L, eng)
    for fmt in (-1, 6, 1 << 20):
        assert call(fmt=fmt) == ARG and "fmt" in _err(L, eng)
    for B in (0, -1, 4097):
        assert call(B=B) == ARG and "B" in _err(L, eng)
    for rgb in (2, -1):
        assert call(rgb=rgb) == ARG and "rgb" in _err(L, eng)
    for fmt in range(6):
        for h, w in ((6, 9), (0, 10), (6, 0), (1, 10), (8194, 10), (6, 8194), (-6, 10)):
            assert call(fmt=fmt, H0=h, W0=w) == ARG, (fmt, h, w)
        assert (call(fmt=fmt, H0=7, W0=10) == ARG) == (fmt >= 2)
    # what IS accepted up to the device check: every format, both rgb values, the largest B and frame.  Without a GPU the call then
    # stops with the HIP status, never with VTI_ERR_ARG.
    import torch
    if not torch.cuda.is_available():
        for kw in (dict(fmt=5, H0=6, W0=10), dict(rgb=1), dict(B=4096), dict(H0=8192, W0=8192, B=1)):
            assert call(**kw) != ARG, kw


def test_convert_raw_frames_argument_checks_come_before_any_hip_call(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    eng = vti_amd.Engine("n", 2, H=64, W=64, max_batch=5)
    n = len(SHAPES)
    rc, rtab, roff = _pack(L, eng._ctx)
    assert rc == 0
    ft = eng.pack_frames(SHAPES, device="cpu")[0]
    ftab = ft.host.numpy()
    raw_bytes, out_bytes = int(roff[n]), ft.total_bytes
    src, dst, drt, dft = C.c_void_p(4096 + 1), C.c_void_p(1 << 20), C.c_void_p(1 << 21), C.c_void_p(1 << 22)

    def call(ctx=eng._ctx, raw=src, raw_bytes=raw_bytes, hrt=rtab.ctypes.data, drt=drt, hft=ftab.ctypes.data, dft=dft, n=n, rgb=0, out=dst,
             out_bytes=out_bytes):
        return L.vti_convert_raw_frames(ctx, raw, raw_bytes, hrt, drt, hft, dft, n, rgb, out, out_bytes, None)
    assert call(ctx=None) == ARG
    for name in ("raw", "hrt", "drt", "out"):
        assert call(**{name: None}) == ARG, name
        assert "null pointer" in _err(L, eng), name
    assert call(hft=None) == ARG and call(dft=None) == ARG and "frame table" in _err(L, eng)
    assert call(drt=C.c_void_p((1 << 21) + 8)) == ARG and "16-byte" in _err(L, eng)
    assert call(dft=C.c_void_p((1 << 22) + 8)) == ARG and "16-byte" in _err(L, eng)
    assert call(n=0) == ARG and call(n=-1) == ARG and call(n=4097) == ARG
    assert call(n=n - 1) == ARG                                                      # tables for another n
    assert call(rgb=2) == ARG and call(rgb=-1) == ARG
    assert call(raw_bytes=raw_bytes - 1) == ARG and "raw_bytes smaller" in _err(L, eng)
    assert call(out_bytes=out_bytes - 1) == ARG and "out_bytes smaller" in _err(L, eng)
    assert call(hrt=np.zeros_like(rtab).ctypes.data) == ARG and "not a table of vti_pack_raw_frames" in _err(L, eng)
    assert call(hft=np.zeros_like(ftab).ctypes.data) == ARG and "not a table of vti_pack_frames" in _err(L, eng)
    other = vti_amd.Engine("n", 2, H=96, W=96, max_batch=5)                          # a frame table for another canvas
    assert call(hft=other.pack_frames(SHAPES, device="cpu")[0].host.numpy().ctypes.data) == ARG and "canvas" in _err(L, eng)
    # row b of the raw table against row b of the frame table
    swapped = list(SHAPES)
    swapped[1], swapped[3] = swapped[3], swapped[1]
    assert call(hft=eng.pack_frames(swapped, device="cpu")[0].host.numpy().ctypes.data) == ARG
    assert "frame 1:" in _err(L, eng) and "34x66" in _err(L, eng) and "18x34" in _err(L, eng)
    # every raw row is validated again.  A row: int64 raw_off, raw_len; int32 H0, W0, fmt
    row = 64 + 32 * 2
    for field, value, why in ((0, int(roff[2]) + 8, "multiple of 16"), (0, int(roff[1]), "ascend"), (0, -16, "ascend"), (0, 1 << 40, "runs past"),
                              (1, 0, "raw_len"), (1, 1 << 40, "raw_len")):
        t = rtab.copy()
        t[row + 8 * field:row + 8 * field + 8] = np.frombuffer(np.int64(value).tobytes(), np.uint8)
        assert call(hrt=t.ctypes.data) == ARG, (field, value)
        assert "row 2" in _err(L, eng) and why in _err(L, eng), (field, value, _err(L, eng))
    for field, value in ((0, 3), (0, 0), (0, 1 << 20), (1, 3), (1, 8194), (2, 6), (2, -1), (2, 0)):      # fmt 0 with H0 = W0 = 2: another raw_len
        t = rtab.copy()
        t[row + 16 + 4 * field:row + 20 + 4 * field] = np.frombuffer(np.int32(value).tobytes(), np.uint8)
        assert call(hrt=t.ctypes.data) == ARG, (field, value)
        assert "row 2" in _err(L, eng), (field, value, _err(L, eng))
    t = rtab.copy()                      # rows 3 and 4 exchanged (in both tables): the raw offsets no longer ascend
    t[64 + 96:64 + 128], t[64 + 128:64 + 160] = rtab[64 + 128:64 + 160], rtab[64 + 96:64 + 128]
    assert call(hrt=t.ctypes.data) == ARG and "frame 3:" in _err(L, eng)
    ft34 = eng.pack_frames(SHAPES[:3] + [SHAPES[4], SHAPES[3]], device="cpu")[0].host.numpy()
    assert call(hrt=t.ctypes.data, hft=ft34.ctypes.data) == ARG and "row 4" in _err(L, eng) and "ascend" in _err(L, eng)
    t = ftab.copy()                      # a corrupted frame-table row is the *_frames calls' error
    t[64 + 64:64 + 72] = np.frombuffer(np.int64(8).tobytes(), np.uint8)
    assert call(hft=t.ctypes.data) == ARG and "frame 1 of host_table" in _err(L, eng)
    import torch
    if not torch.cuda.is_available():
        for kw in (dict(rgb=1), dict(raw_bytes=raw_bytes + 5), dict(out_bytes=out_bytes + 1), dict(raw=C.c_void_p(1 << 12))):
            assert call(**kw) != ARG, kw


def test_rawframes_constructor_and_engine_wrappers_refuse_bad_input_before_a_device(lib_built):
    vti_amd = lib_built
    RF = vti_amd.RawFrames
    fb = 2 * 6 * 10
    data = np.arange(3 * fb, dtype=np.uint8)
    for d in (data, data.reshape(3, 6, 10, 2), data.tobytes(), bytearray(data.tobytes())):
        r = RF(d, "yuyv", 6, 10)
        assert (r.n, r.fmt, r.H0, r.W0, r.frame_bytes, len(r)) == (3, 0, 6, 10, fb, 3)
        assert np.array_equal(r.to_bgr(), vti_amd.rawframes.to_bgr(data, "yuyv", 6, 10))
    import torch
    assert RF(torch.from_numpy(data), 1, 6, 10).n == 3 and RF(data[:90].reshape(9, 10), "NV12", 6, 10).n == 1
    with pytest.raises(ValueError, match=f"multiple of {fb} bytes, got {fb + 1}"):
        RF(data[:fb + 1], "yuyv", 6, 10)
    with pytest.raises(ValueError, match="multiple of 90 bytes"):
        RF(data[:fb], "i420", 6, 10)
    with pytest.raises(ValueError, match="multiple of"):
        RF(b"", "yuyv", 6, 10)
    with pytest.raises(ValueError, match="unknown raw format"):
        RF(data, "bgr", 6, 10)
    with pytest.raises(ValueError, match="unknown raw format"):
        RF(data, 6, 6, 10)
    with pytest.raises(ValueError, match="even W0"):
        RF(data, "yuyv", 6, 9)
    with pytest.raises(ValueError, match="even H0"):
        RF(data, "nv12", 5, 10)
    with pytest.raises(ValueError, match="2..8192"):
        RF(data, "yuyv", 0, 10)
    with pytest.raises(ValueError, match="uint8"):
        RF(data.astype(np.int32), "yuyv", 6, 10)
    with pytest.raises(ValueError, match="uint8"):
        RF(torch.zeros(fb, dtype=torch.float32), "yuyv", 6, 10)
    Y = vti_amd.YOLO
    assert Y._raw_source(np.zeros((8, 8, 3), np.uint8)) is None and Y._raw_source([np.zeros((8, 8, 3), np.uint8)]) is None
    assert Y._raw_source(b"abc") is None and Y._jpeg_files(RF(data, "yuyv", 6, 10)) is None
    r = RF(data, "yuyv", 6, 10)
    assert Y._raw_source(r) == [r] and Y._raw_source([r, r]) == [r, r]
    with pytest.raises(ValueError, match="all RawFrames or none"):
        Y._raw_source([r, np.zeros((6, 10, 3), np.uint8)])
    eng = vti_amd.Engine("n", 2, H=64, W=64, max_batch=1)
    with pytest.raises(ValueError, match="120 bytes each"):
        eng.convert_raw(data[:100], "yuyv", 6, 10)
    with pytest.raises(ValueError, match="unknown raw format"):
        eng.convert_raw(data, "xyz", 6, 10)
    with pytest.raises(ValueError, match="even W0"):
        eng.convert_raw(data, "uyvy", 6, 9)
    with pytest.raises(ValueError, match="out must be"):
        eng.convert_raw(data, "yuyv", 6, 10, out=torch.zeros((3, 6, 10, 4), dtype=torch.uint8))
    with pytest.raises(ValueError, match="RawTable"):
        eng.convert_raw_frames(torch.zeros(16, dtype=torch.uint8), None, None)
