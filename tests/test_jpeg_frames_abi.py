"""vti_encode_jpeg_frames' C ABI without a GPU: the three entry points exist, the two size functions (the scratch is laid out per
frame, not pitched by the largest one), and every argument check comes before the first HIP call (fake pointers, never
dereferenced).  The GPU parity tests are in test_gpu_jpeg_frames.py."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vti_encode_jpeg_frames_scratch_bytes", "vti_encode_jpeg_frames_max_bytes", "vti_encode_jpeg_frames")
SHAPES = [(135, 241), (17, 33), (480, 640)]


def _hp(t):
    return C.c_void_p(t.host.data_ptr())


def _al(v):
    return (v + 255) & ~255


def test_the_entry_points_are_declared_exported_and_bound(lib_built):
    vti_amd = lib_built
    hdr = open(os.path.join(ROOT, "include", "vti.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", vti_amd.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"\bT %s$" % name, exported, re.M), name
        assert name in vti_amd.SIGNATURES
    assert re.search(r"Ten launches", hdr)                      # the new launch count is stated


def test_the_size_functions_are_sums_over_the_frames(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    eng = vti_amd.Engine("n", 2, H=736, W=960, max_batch=4)
    for shapes in (SHAPES, [(1080, 1920), (481, 333)], [(1, 1)], [(16, 16)] * 5, [(960, 1280), (481, 333), (720, 960), (1080, 1920)] * 3):
        t, _, _ = eng.pack_frames(shapes, device="cpu")
        n = len(shapes)
        scratch = L.vti_encode_jpeg_frames_scratch_bytes(eng._ctx, _hp(t))
        singles = [L.vti_encode_jpeg_scratch_bytes(eng._ctx, 1, h, w) for h, w in shapes]
        header = 2 * _al(8 * (n + 1))                           # the two prefix arrays
        assert 0 < scratch <= sum(singles) + header and scratch % 256 == 0, (shapes, scratch, sum(singles), header)
        # per frame at least its coefficients: nothing is pitched, nothing is left out
        assert scratch >= sum(-(-h // 16) * -(-w // 16) * 6 * 128 for h, w in shapes)
        assert L.vti_encode_jpeg_frames_max_bytes(_hp(t)) == sum(L.vti_encode_jpeg_max_bytes(1, h, w) for h, w in shapes)
    # a large and a small frame: far below the pitch of the larger one
    t, _, _ = eng.pack_frames([(1080, 1920), (481, 333)], device="cpu")
    big = L.vti_encode_jpeg_scratch_bytes(eng._ctx, 1, 1080, 1920)
    assert L.vti_encode_jpeg_frames_scratch_bytes(eng._ctx, _hp(t)) < 2 * big
    assert L.vti_encode_jpeg_frames_scratch_bytes(eng._ctx, _hp(t)) < big + 2 * 1024 * 1024 + 4096      # the 333-wide frame needs under 2 MB
    # bad arguments: 0
    assert L.vti_encode_jpeg_frames_scratch_bytes(None, _hp(t)) == 0 and L.vti_encode_jpeg_frames_scratch_bytes(eng._ctx, None) == 0
    assert L.vti_encode_jpeg_frames_max_bytes(None) == 0
    junk = (C.c_uint8 * 256)()
    assert L.vti_encode_jpeg_frames_scratch_bytes(eng._ctx, junk) == 0 and L.vti_encode_jpeg_frames_max_bytes(junk) == 0
    tall, _, _ = eng.pack_frames([(480, 640), (8200, 480)], device="cpu")        # the table allows 16384, the encoder 8192
    assert L.vti_encode_jpeg_frames_scratch_bytes(eng._ctx, _hp(tall)) == 0 and L.vti_encode_jpeg_frames_max_bytes(_hp(tall)) == 0


def test_argument_checks_come_before_any_hip_call(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    eng = vti_amd.Engine("n", 2, H=736, W=960, max_batch=4)
    t, _, _ = eng.pack_frames(SHAPES, device="cpu")
    n = len(SHAPES)
    need = L.vti_encode_jpeg_frames_scratch_bytes(eng._ctx, _hp(t))
    one, ws, off = C.c_void_p(4096), C.c_void_p(1 << 20), C.c_void_p(8192)      # never dereferenced
    err = lambda: L.vti_last_error(eng._ctx)

    def call(ctx=eng._ctx, frames=one, ht=_hp(t), dt=one, n=n, rgb=0, quality=95, scratch=ws, nbytes=need, offsets=off, out=one,
             max_bytes=1 << 20):
        return L.vti_encode_jpeg_frames(ctx, frames, ht, dt, n, rgb, quality, scratch, nbytes, offsets, out, max_bytes, None)

    assert call(ctx=None) == -1
    for name in ("frames", "ht", "dt", "offsets", "out", "scratch"):
        assert call(**{name: None}) == -1, name
    assert call(quality=0) == -1 and call(quality=101) == -1 and b"quality" in err()
    assert call(rgb=2) == -1 and call(rgb=-1) == -1
    assert call(max_bytes=-1) == -1
    # a table for another n, or for another canvas
    assert call(n=2) == -1 and b"another B" in err()
    assert call(n=4) == -1 and call(n=0) == -1
    other, _, _ = vti_amd.Engine("n", 2, H=64, W=96, max_batch=4).pack_frames(SHAPES, device="cpu")
    assert call(ht=_hp(other)) == -1 and b"another canvas" in err()
    tall, _, _ = eng.pack_frames([(480, 640), (8200, 480), (17, 33)], device="cpu")
    assert call(ht=_hp(tall), nbytes=1 << 40) == -1 and b"8192" in err()
    assert call(nbytes=need - 1) == -1 and b"scratch smaller" in err()
    assert call(scratch=C.c_void_p((1 << 20) + 64)) == -1 and b"256-byte" in err()
    assert call(offsets=C.c_void_p(8192 + 4)) == -1
    assert call(dt=C.c_void_p(4096 + 8)) == -1
    # what IS accepted up to the device check: without a GPU the call then stops with the HIP status, never with VTI_ERR_ARG
    for kw in (dict(), dict(out=None, max_bytes=0), dict(quality=1), dict(quality=100), dict(rgb=1)):
        assert call(**kw) != -1, kw


def test_engine_encode_jpeg_with_a_table_refuses_bad_input_before_it_touches_a_device(lib_built):
    import torch
    vti_amd = lib_built
    eng = vti_amd.Engine("n", 2, H=64, W=64, max_batch=2)
    table, _, total = eng.pack_frames([(48, 64), (17, 33)], device="cpu")
    buf = torch.zeros(total, dtype=torch.uint8)
    with pytest.raises(ValueError, match="flat uint8"):
        eng.encode_jpeg(buf.view(1, -1), table=table)
    with pytest.raises(ValueError, match="FrameTable"):
        eng.encode_jpeg(buf, table=[(48, 64)])
    with pytest.raises(ValueError, match="quality"):
        eng.encode_jpeg(buf, quality=0, table=table)
    with pytest.raises(ValueError, match="max_bytes"):
        eng.encode_jpeg(buf, max_bytes=-1, table=table)
    with pytest.raises(ValueError, match="frame buffer"):
        eng.encode_jpeg(buf[:100], table=table)
    with pytest.raises(ValueError, match="device"):                 # a good call on host memory stops at the device check
        eng.encode_jpeg(buf, table=table)
