"""vti_mask_polygons' C ABI without a GPU: the scratch size and every argument check, which all run before the first HIP call
(Results.masks.xy on the device; the GPU parity tests are in test_gpu_polygons.py)."""
import ctypes as C

import pytest


def test_scratch_bytes_for_valid_and_bad_sizes(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    eng = vti_amd.Engine("n", 2, H=64, W=64, max_batch=1)
    ctx = eng._ctx
    lb = eng.mask_polygons_scratch_bytes(736, 960, 120)            # letterbox bits of the reference call (imgsz 960)
    nat = eng.mask_polygons_scratch_bytes(960, 1280, 160)          # retina rows of a 1280 x 960 frame
    # one labelling area per workgroup: parent + runs (4 B each per possible run, H * ceil(W/2) runs) + row starts
    assert lb >= 128 * (8 * 736 * 480 + 4 * 737) and nat >= 128 * (8 * 960 * 640 + 4 * 961)
    assert lb < 400 * 2 ** 20 and nat < 700 * 2 ** 20
    # the size depends on the geometry only: a wider row pitch with the same W needs the same scratch
    assert eng.mask_polygons_scratch_bytes(736, 960, 128) == lb
    # too big for LDS (> 156 KiB of 64-bit words): the image gets a part of each area
    tall = eng.mask_polygons_scratch_bytes(1100, 1280, 160)
    assert tall >= 128 * (8 * 1100 * 640 + 8 * 1100 * 20)
    assert eng.mask_polygons_scratch_bytes(1, 1, 1) > 0
    for H, W, rb in [(0, 8, 1), (8, 0, 1), (8, 9, 1), (8, 64, 7), (-1, 8, 1), (8, 8, 0), (16385, 8, 1), (8, 16385, 2049),
                     (16384, 8192, 1024)]:
        assert L.vti_mask_polygons_scratch_bytes(ctx, H, W, rb) == 0, (H, W, rb)
    assert L.vti_mask_polygons_scratch_bytes(None, 736, 960, 120) == 0


def test_mask_polygons_argument_checks_without_a_gpu(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    eng = vti_amd.Engine("n", 2, H=64, W=64, max_batch=1)
    n, H, W, rb, H0, W0 = 3, 48, 64, 8, 60, 80
    need = eng.mask_polygons_scratch_bytes(H, W, rb)
    one, ws = C.c_void_p(4096), C.c_void_p(1 << 20)               # never dereferenced: every check comes before any HIP call

    def call(ctx=eng._ctx, masks=one, n=n, H=H, W=W, rb=rb, H0=H0, W0=W0, strategy=0, scratch=ws, nbytes=need, offsets=one,
             points=one, max_points=100):
        return L.vti_mask_polygons(ctx, masks, n, None, H, W, rb, H0, W0, strategy, scratch, nbytes, offsets, points, max_points,
                                   None)

    assert call(ctx=None) == -1
    assert call(n=-1) == -1
    assert call(H=0) == -1 and call(W=0) == -1 and call(H0=0) == -1 and call(W0=0) == -1
    assert call(rb=7) == -1                                         # row_bytes * 8 < W
    assert b"row_bytes" in L.vti_last_error(eng._ctx)
    assert call(H=16385, W=8, rb=1, nbytes=1 << 40) == -1 and call(H=16384, W=8192, rb=1024, nbytes=1 << 40) == -1
    assert call(strategy=2) == -1 and call(strategy=-1) == -1
    assert b"strategy" in L.vti_last_error(eng._ctx)
    assert call(max_points=-1) == -1
    assert call(masks=None) == -1
    assert call(offsets=None) == -1
    assert call(points=None) == -1
    assert call(nbytes=need - 1) == -1
    assert b"scratch" in L.vti_last_error(eng._ctx)
    assert call(scratch=None) == -1
    assert call(scratch=C.c_void_p((1 << 20) + 64)) == -1           # 256-byte alignment


def test_engine_rejects_an_unknown_strategy(lib_built):
    eng = lib_built.Engine("n", 2, H=64, W=64, max_batch=1)
    with pytest.raises(ValueError):
        eng.mask_polygons(None, 64, 48, 64, strategy="all")
