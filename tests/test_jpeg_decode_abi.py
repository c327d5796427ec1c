"""vti_decode_jpeg's C ABI without a GPU: the three entry points exist; the plan (host only) parses, refuses and lays out exactly
as documented and is deterministic; every argument check of vti_decode_jpeg, the table revalidated row by row included, comes
before the first HIP call (fake device pointers, never dereferenced).  The GPU parity tests are in test_gpu_jpeg_decode.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import jpeg_decode_util as U
import jpeg_util as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vti_decode_jpeg_table_bytes", "vti_decode_jpeg_plan", "vti_decode_jpeg")
ARG, UNSUPPORTED = -1, -6


def _files():
    return [U.own_file(J.frame("ramp", 17, 33), 95, "420"), U.own_file(J.frame("noise", 50, 70), 95, "444", restart=3),
            U.own_file(J.frame("tiles", 17, 33), 50, "422", with_dht=False)]


def test_the_entry_points_are_declared_exported_and_bound(lib_built):
    vti_amd = lib_built
    hdr = open(os.path.join(ROOT, "include", "vti.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", vti_amd.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"\bT %s$" % name, exported, re.M), name
        assert name in vti_amd.SIGNATURES
    # header == nm -D == SIGNATURES still holds for the whole library
    declared = set(re.findall(r"\b(vti_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(re.findall(r"\bT (vti_\w+)$", exported, re.M)) == set(vti_amd.SIGNATURES)
    assert "VTI_JPEG_CORRUPT = 1" in hdr
    assert hasattr(vti_amd.Engine, "decode_jpeg") and callable(vti_amd.jpeg.decode) and callable(vti_amd.jpeg.parse)


def test_the_plan_lays_the_frames_out_as_pack_frames_does_and_is_deterministic(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    assert L.vti_decode_jpeg_table_bytes(0) == 0 and L.vti_decode_jpeg_table_bytes(-1) == 0 and L.vti_decode_jpeg_table_bytes(4097) == 0
    t1, t3 = L.vti_decode_jpeg_table_bytes(1), L.vti_decode_jpeg_table_bytes(3)
    assert t1 > 0 and (t3 - t1) % 2 == 0 and (t3 - t1) // 2 == t1 - 64
    files = _files()
    rc, p = U.plan(vti_amd, files)
    assert rc == 0, p["error"]
    assert p["H0"].tolist() == [17, 50, 17] and p["W0"].tolist() == [33, 70, 33]
    eng = vti_amd.Engine("n", 2, H=64, W=64, max_batch=3)
    host = np.zeros(int(L.vti_frame_table_bytes(3)), np.uint8)
    off = [0, (3 * 17 * 33 + 15) & ~15, 0]
    off[2] = (off[1] + 3 * 50 * 70 + 15) & ~15
    total = (off[2] + 3 * 17 * 33 + 15) & ~15
    assert p["out_off"].tolist() == off + [total] and all(o % 16 == 0 for o in off)
    # ... so vti_pack_frames accepts these very offsets and this very total
    assert L.vti_pack_frames(eng._ctx, 64, 64, (C.c_int32 * 3)(17, 50, 17), (C.c_int32 * 3)(33, 70, 33), (C.c_int64 * 3)(*off), 3, total,
                             host.ctypes.data, host.size) == 0
    assert p["scratch_bytes"] > 0 and p["scratch_bytes"] % 256 == 0
    rc2, p2 = U.plan(vti_amd, files)
    assert rc2 == 0 and np.array_equal(p2["table"], p["table"]) and p2["scratch_bytes"] == p["scratch_bytes"]
    # another segment size is another table and more (or fewer) segment states
    rc16, p16 = U.plan(vti_amd, files, segment_bytes=16)
    assert rc16 == 0 and not np.array_equal(p16["table"], p["table"]) and p16["scratch_bytes"] > p["scratch_bytes"]
    # layout 1: dense, and only for files of one size
    rc, pd = U.plan(vti_amd, [files[0], files[2]], layout=1)
    assert rc == 0 and pd["out_off"].tolist() == [0, 3 * 17 * 33, 2 * 3 * 17 * 33]
    rc, pd = U.plan(vti_amd, files, layout=1)
    assert rc == ARG and "file 1" in pd["error"] and "one size" in pd["error"]
    # the Engine wrapper reports the same plan
    ep = eng.decode_jpeg_plan(files)
    assert ep["shapes"] == [(17, 33), (50, 70), (17, 33)] and ep["byte_offsets"] == off and ep["out_bytes"] == total and not ep["dense"]
    assert eng.decode_jpeg_plan([files[0], files[2]])["dense"]


def test_the_plan_refuses_bad_arguments_and_files_and_names_the_file(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    files = _files()
    eng = vti_amd.Engine("n", 2, H=64, W=64, max_batch=1)
    n = len(files)
    blob = np.frombuffer(b"".join(files), np.uint8).copy()
    offs = np.cumsum([0] + [len(f) for f in files]).astype(np.int64)
    nb = int(L.vti_decode_jpeg_table_bytes(n))
    table = np.zeros(nb, np.uint8)
    H0, W0, oo, sc = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n + 1, np.int64), C.c_int64(0)

    def call(files_p=blob.ctypes.data, offs_p=offs.ctypes.data, n=n, seg=0, layout=0, table_p=table.ctypes.data, nbytes=nb,
             h=H0.ctypes.data, w=W0.ctypes.data, o=oo.ctypes.data, s=C.byref(sc)):
        return L.vti_decode_jpeg_plan(eng._ctx, files_p, offs_p, n, seg, layout, table_p, nbytes, h, w, o, s)
    assert call() == 0
    for kw in ("files_p", "offs_p", "table_p", "h", "w", "o", "s"):
        assert call(**{kw: None}) == ARG, kw
        assert b"null pointer" in L.vti_last_error(eng._ctx)
    assert call(n=0) == ARG and call(n=-1) == ARG and call(n=4097) == ARG
    for seg in (1, 8, 15, 17, 24, 100, 8192, -16):
        assert call(seg=seg) == ARG, seg
        assert b"segment_bytes" in L.vti_last_error(eng._ctx)
    for seg in (16, 32, 64, 128, 256, 512, 1024, 2048, 4096):
        assert call(seg=seg) == 0, seg
    assert call(layout=2) == ARG and call(layout=-1) == ARG
    assert call(nbytes=nb - 1) == ARG and b"table smaller" in L.vti_last_error(eng._ctx)
    bad_offs = offs.copy()
    bad_offs[1], bad_offs[2] = offs[2], offs[1]
    assert call(offs_p=bad_offs.ctypes.data) == ARG and b"ascend" in L.vti_last_error(eng._ctx)
    # a truncated header, an empty file, no JPEG at all: VTI_ERR_ARG with the index of the first failing file
    for k, cut in ((1, 100), (2, 0), (0, 3)):
        fs = list(files)
        fs[k] = fs[k][:cut]
        rc, p = U.plan(vti_amd, fs, ctx=eng._ctx)
        assert rc == ARG and f"file {k}:" in p["error"], (k, cut, p["error"])
    rc, p = U.plan(vti_amd, [files[0], b"GIF89a" + bytes(100)], ctx=eng._ctx)
    assert rc == ARG and "file 1:" in p["error"] and "SOI" in p["error"]
    # the refused classes: VTI_ERR_UNSUPPORTED and the reason
    base = files[0]
    sof = next(a for m, a, b in U.segments(base) if m == 0xC0)
    dqt = next(a for m, a, b in U.segments(base) if m == 0xDB)
    sos = next(a for m, a, b in U.segments(base) if m == 0xDA)

    def patched(at, value):
        d = bytearray(base)
        d[at] = value
        return bytes(d)
    for name, data in (("progressive", patched(sof + 1, 0xC2)), ("arithmetic", patched(sof + 1, 0xC9)), ("12-bit", patched(sof + 4, 12)),
                       ("sampling", patched(sof + 11, 0x41)), ("16-bit quantisation", patched(dqt + 4, 0x10)),
                       ("greyscale", base[:sof + 2] + b"\x00\x0b" + base[sof + 4:sof + 9] + b"\x01\x01\x11\x00" + base[sof + 19:]),
                       ("Adobe transform 0", base[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00" + base[2:]),
                       ("multiple scans", base[:-2] + base[sos:sos + 14] + b"\x00\xff\xd9"),
                       ("8192", patched(sof + 5, 0x40))):
        rc, p = U.plan(vti_amd, [files[1], data], ctx=eng._ctx)
        assert rc == UNSUPPORTED and "file 1:" in p["error"] and name in p["error"], (name, rc, p["error"])
        with pytest.raises(vti_amd.jpeg.UnsupportedJpeg):            # the host specification refuses the same files
            vti_amd.jpeg.parse(data)
        with pytest.raises(vti_amd.VtiError) as e:                   # Engine.decode_jpeg raises before it looks for a device
            eng.decode_jpeg([files[1], data])
        assert e.value.code == UNSUPPORTED
    # what the parser accepts agrees with jpeg.parse field by field
    rc, p = U.plan(vti_amd, files)
    for k, f in enumerate(files):
        h = vti_amd.jpeg.parse(f)
        assert (h["H0"], h["W0"]) == (p["H0"][k], p["W0"][k])


def test_decode_argument_checks_come_before_any_hip_call(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    eng = vti_amd.Engine("n", 2, H=64, W=64, max_batch=1)
    files = _files()
    n = len(files)
    rc, p = U.plan(vti_amd, files)
    assert rc == 0
    table, need, room = p["table"], p["scratch_bytes"], int(p["out_off"][-1])
    one, ws, dtab, info = C.c_void_p(4096 + 1), C.c_void_p(1 << 20), C.c_void_p(1 << 21), C.c_void_p(1 << 22)

    def call(ctx=eng._ctx, files_p=one, host=table.ctypes.data, dev=dtab, n=n, rgb=1, out=one, out_bytes=room, info=info, scratch=ws,
             nbytes=need):
        return L.vti_decode_jpeg(ctx, files_p, host, dev, n, rgb, out, out_bytes, info, scratch, nbytes, None)
    assert call(ctx=None) == ARG
    for name in ("files_p", "host", "dev", "out", "info"):
        assert call(**{name: None}) == ARG, name
        assert b"null pointer" in L.vti_last_error(eng._ctx), name
    assert call(scratch=None) == ARG and b"256-byte" in L.vti_last_error(eng._ctx)
    assert call(scratch=C.c_void_p((1 << 20) + 64)) == ARG
    assert call(dev=C.c_void_p((1 << 21) + 8)) == ARG and call(info=C.c_void_p((1 << 22) + 2)) == ARG
    assert call(n=0) == ARG and call(n=-1) == ARG
    assert call(n=n - 1) == ARG and b"descriptor table" in L.vti_last_error(eng._ctx)      # a table for another n
    assert call(rgb=2) == ARG and call(rgb=-1) == ARG
    assert call(nbytes=need - 1) == ARG and b"scratch smaller" in L.vti_last_error(eng._ctx)
    assert call(out_bytes=room - 1) == ARG and b"dev_out smaller" in L.vti_last_error(eng._ctx)
    junk = np.zeros_like(table)
    assert call(host=junk.ctypes.data) == ARG and b"descriptor table" in L.vti_last_error(eng._ctx)
    short = table[:64 + (table.size - 64) // n].copy()                                    # a one-file table passed as n = 3's
    assert call(host=short.ctypes.data) == ARG
    # every row is validated again: a value a kernel would form an address from, changed in the table, is refused.  The first
    # int64 fields of a row: file_off, file_len, scan_start, scan_end, out_off, off_seg, off_coef, off_planes; then the int32s
    # H0, W0, hs, vs, mcu_rows, mcu_cols, bpm, nblk, ri, seg_bytes, nseg
    row = 64 + (table.size - 64) // n                  # row 1
    for field, value in ((0, 1 << 40), (2, 0), (3, 1 << 40), (4, 1 << 40), (4, -16), (5, 1 << 40), (6, 0), (7, 1 << 40)):
        t = table.copy()
        t[row + 8 * field:row + 8 * field + 8] = np.frombuffer(np.int64(value).tobytes(), np.uint8)
        assert call(host=t.ctypes.data) == ARG, field
        assert b"row 1" in L.vti_last_error(eng._ctx), (field, L.vti_last_error(eng._ctx))
    for field, value in ((0, 9000), (0, 0), (1, 1 << 20), (2, 3), (4, 1), (5, 1 << 20), (6, 7), (7, 1 << 28), (8, -1), (9, 24), (10, 1 << 28), (10, 0)):
        t = table.copy()
        t[row + 64 + 4 * field:row + 68 + 4 * field] = np.frombuffer(np.int32(value).tobytes(), np.uint8)
        assert call(host=t.ctypes.data) == ARG, field
        assert b"row 1" in L.vti_last_error(eng._ctx), (field, L.vti_last_error(eng._ctx))
    t = table.copy()
    t[row + 112 + 10] = t[row + 112 + 11] = 0                                              # a quantisation step of 0
    assert call(host=t.ctypes.data) == ARG
    # what IS accepted up to the device check: both rgb values, a larger scratch and output.  Without a GPU the call then stops
    # with the HIP status, never with VTI_ERR_ARG.
    for kw in (dict(rgb=0), dict(nbytes=need + 4096), dict(out_bytes=room + 1)):
        assert call(**kw) != ARG, kw


def test_engine_decode_jpeg_refuses_bad_input_before_it_touches_a_device(lib_built):
    vti_amd = lib_built
    eng = vti_amd.Engine("n", 2, H=64, W=64, max_batch=1)
    with pytest.raises(ValueError, match="at least one"):
        eng.decode_jpeg([])
    with pytest.raises(ValueError, match="bytes"):
        eng.decode_jpeg([np.zeros((8, 8, 3), np.uint8)])
    with pytest.raises(vti_amd.VtiError, match="file 0"):
        eng.decode_jpeg([b"not a jpeg"])
    with pytest.raises(vti_amd.VtiError, match="segment_bytes"):
        eng.decode_jpeg(_files(), segment_bytes=24)
    with pytest.raises(vti_amd.VtiError, match="one size"):
        eng.decode_jpeg(_files(), dense=True)
    # sources of predict: bytes, paths and lists of them are files; arrays are not; a mixed list is refused
    Y = vti_amd.YOLO
    assert Y._jpeg_files(np.zeros((8, 8, 3), np.uint8)) is None and Y._jpeg_files([np.zeros((8, 8, 3), np.uint8)]) is None
    f = _files()[0]
    assert Y._jpeg_files(f) == [f] and Y._jpeg_files([f, bytearray(f)]) == [f, f] and Y._jpeg_files((f,)) == [f]
    with pytest.raises(ValueError, match="all frames or all JPEG files"):
        Y._jpeg_files([f, np.zeros((8, 8, 3), np.uint8)])


def test_predict_reads_paths(lib_built, tmp_path):
    vti_amd = lib_built
    f = _files()[0]
    path = tmp_path / "frame.jpg"
    path.write_bytes(f)
    assert vti_amd.YOLO._jpeg_files(str(path)) == [f] and vti_amd.YOLO._jpeg_files([path, f]) == [f, f]
