"""vti_measure_cameras without a GPU: the three entry points exist, the camera table is validated when it is packed, every
argument check of the call comes before the first HIP call (fake pointers, never dereferenced), and MultiCameraMeasurer keeps one
smoothing stream per camera."""
import ctypes as C
import dataclasses as dc
import os
import re
import subprocess
import types
from collections import deque

import numpy as np
import pytest

from test_oracle_geometry import load_calib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
CALIB = load_calib()
NAMES = ("vti_measure_cameras_bytes", "vti_measure_pack_cameras", "vti_measure_cameras")


def _two_calibrations(vti_amd):
    calib = os.path.join(G, "camera_calibration.json")
    return [vti_amd.MeasureParams.from_files(calib, os.path.join(G, name)) for name in ("extrinsics.json", "camera_extrinsics.json")]


def test_the_three_entry_points_are_declared_exported_and_bound(lib_built):
    vti_amd = lib_built
    hdr = open(os.path.join(ROOT, "include", "vti.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", vti_amd.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"\bT %s$" % name, exported, re.M), name
        assert name in vti_amd.SIGNATURES
    assert re.search(r"VTI_MEASURE_BAD_CAMERA\s*=\s*3\b", hdr)
    assert vti_amd._lib.VTI_MEASURE_BAD_CAMERA == 3
    assert "MultiCameraMeasurer" in vti_amd.__all__


def test_pack_cameras_validates_every_entry_and_is_deterministic(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    eng = vti_amd.Engine("n", 2, H=64, W=64, max_batch=2)
    p, q = _two_calibrations(vti_amd)
    row = L.vti_measure_cameras_bytes(1)
    assert row > 0 and row % 16 == 0 and L.vti_measure_cameras_bytes(5) == 5 * row
    assert L.vti_measure_cameras_bytes(0) == 0 and L.vti_measure_cameras_bytes(-3) == 0

    def pack(params, n=None, out="alloc", nbytes=None):
        n = len(params) if n is None else n
        arr = (vti_amd._lib.VtiMeasureParams * max(len(params), 1))(*[x.to_c() for x in params]) if params is not None else None
        buf = (C.c_uint8 * max(row * max(n, 1), 1))(*([0xA5] * max(row * max(n, 1), 1))) if out == "alloc" else out
        rc = L.vti_measure_pack_cameras(eng._ctx, arr, n, buf, row * n if nbytes is None else nbytes)
        return rc, (bytes(buf) if buf is not None else None)

    rc, a = pack([p, q, p])
    assert rc == 0
    rc, b = pack([p, q, p])
    assert rc == 0 and a == b                                                # equal inputs, equal bytes (padding included)
    assert a[:row] == a[2 * row:3 * row] and a[:row] != a[row:2 * row]         # two calibrations, two different rows
    rc, c = pack([dc.replace(p, roi=(10, 200, 1270, 900))])
    assert rc == 0 and c[:row] != a[:row]
    # frame_buffer is the host's: validated like vti_measure does, but no part of a row
    rc, d = pack([dc.replace(p, frame_buffer=3)])
    assert rc == 0 and d[:row] == a[:row]

    bad = [dc.replace(p, envelope_neighborhood=-1), dc.replace(p, envelope_neighborhood=65), dc.replace(p, fabric_id=0),
           dc.replace(p, min_stitches=0), dc.replace(p, kmeans_iters=-1), dc.replace(p, max_px_distance=float("nan")),
           dc.replace(p, two_row_threshold_px=float("nan")), dc.replace(p, stitch_id=-1), dc.replace(p, frame_buffer=0)]
    for x in bad:
        for k in range(3):
            lst = [p, q, p]
            lst[k] = x
            assert pack(lst)[0] == -1, (x, k)
            msg = L.vti_last_error(eng._ctx)
            assert b"camera %d:" % k in msg, (k, msg)
    assert pack([p, dc.replace(p, envelope_neighborhood=65), dc.replace(p, min_stitches=0)])[0] == -1
    assert b"camera 1:" in L.vti_last_error(eng._ctx) and b"envelope_neighborhood" in L.vti_last_error(eng._ctx)
    assert pack(None, n=2)[0] == -1                                          # null list
    assert pack([p], n=0)[0] == -1 and pack([p], n=-1)[0] == -1
    assert pack([p, q], out=None)[0] == -1                                   # null table
    assert pack([p, q], nbytes=2 * row - 1)[0] == -1                         # short table
    assert b"vti_measure_cameras_bytes" in L.vti_last_error(eng._ctx)
    # a NULL ctx only loses the error text
    arr = (vti_amd._lib.VtiMeasureParams * 1)(p.to_c())
    buf = (C.c_uint8 * row)()
    assert L.vti_measure_pack_cameras(None, arr, 1, buf, row) == 0 and bytes(buf) == a[:row]


def test_measure_cameras_argument_checks_without_a_gpu(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    eng = vti_amd.Engine("n", 2, H=64, W=64, max_batch=2)
    B, max_det, cap, H0, W0 = 2, 10, 20, 48, 64
    need = eng.measure_scratch_bytes(B, cap, W0)                              # the same scratch as vti_measure
    one, ws = C.c_void_p(4096), C.c_void_p(1 << 20)            # never dereferenced: every check comes before any HIP call

    def call(ctx=eng._ctx, table=one, n_cams=4, index=one, masks=one, native=0, dets=one, B=B, max_det=max_det, cap=cap, scratch=ws,
             nbytes=need, frame_f64=one):
        return L.vti_measure_cameras(ctx, table, n_cams, index, masks, native, dets, one, one, one, B, max_det, cap, H0, W0, scratch,
                                     nbytes, frame_f64, one, None, None, None)

    assert call(ctx=None) == -1
    assert call(table=None) == -1
    assert b"vti_measure_cameras" in L.vti_last_error(eng._ctx)
    assert call(index=None) == -1
    assert call(n_cams=0) == -1 and call(n_cams=-1) == -1
    assert b"n_cams" in L.vti_last_error(eng._ctx)
    assert call(table=C.c_void_p(4096 + 8)) == -1              # rows are read with 16-byte loads
    assert call(index=C.c_void_p(4096 + 2)) == -1
    assert call(nbytes=need - 1) == -1
    assert b"scratch" in L.vti_last_error(eng._ctx)
    assert call(scratch=C.c_void_p(4096 + 64)) == -1
    assert call(scratch=None) == -1
    assert call(native=2) == -1
    assert call(masks=C.c_void_p(4096 + 8)) == -1               # letterbox bits: 16-byte loads
    assert call(masks=C.c_void_p(4096 + 4), native=1) == -1     # native rows: 8-byte loads
    assert call(masks=None) == -1
    assert call(dets=None) == -1
    assert call(frame_f64=None) == -1
    assert call(B=-1) == -1 and call(max_det=0) == -1 and call(cap=-1) == -1
    assert call(max_det=vti_amd._lib.VTI_MEASURE_MAX_DET + 1) == -6
    assert call(B=0, cap=0, masks=None, nbytes=0, scratch=None) == 0     # nothing to do: no launch
    # a null table is an error even when there is nothing to do, as a null params is for vti_measure
    assert call(B=0, cap=0, masks=None, nbytes=0, scratch=None, table=None) == -1


def test_engine_measure_range_checks_a_host_camera_list(lib_built):
    """The host sequence form of `cameras` is checked before anything touches a device: no GPU is needed to be refused."""
    import torch
    vti_amd = lib_built
    eng = vti_amd.Engine("n", 2, H=64, W=64, max_batch=2)
    out = dict(dets=torch.zeros((2, 10, 38)), xyxy=torch.zeros((2, 10, 4)), counts=torch.zeros(2, dtype=torch.int32),
               offsets=torch.zeros(3, dtype=torch.int32), masks=torch.zeros((0, 64, 8), dtype=torch.uint8))
    row = int(vti_amd.lib().vti_measure_cameras_bytes(1))
    table = torch.zeros(3 * row, dtype=torch.uint8)
    for cams in ([0, 3], [-1, 0], [0], [0, 1, 2], [0.5, 1.0]):
        with pytest.raises(ValueError):
            eng.measure(out, table, 48, 64, cameras=cams)
    with pytest.raises(ValueError):
        eng.measure(out, table[:row + 1], 48, 64, cameras=[0, 0])
    with pytest.raises(ValueError):
        eng.pack_cameras([])
    p = vti_amd.MeasureParams(*CALIB)
    with pytest.raises(vti_amd.VtiError, match="camera 1"):
        eng.pack_cameras([p, dc.replace(p, min_stitches=0)], device="cpu")
    t = eng.pack_cameras([p, p], device="cpu")
    assert t.dtype == torch.uint8 and t.numel() == 2 * row and bytes(t[:row].numpy()) == bytes(t[row:].numpy())


def test_multi_camera_smoothing_matches_independent_deques_per_camera(lib_built):
    vti_amd = lib_built
    n_cams, fb = 3, 3
    p, q = _two_calibrations(vti_amd)
    model = types.SimpleNamespace(drop_empty_masks=True)
    mc = vti_amd.MultiCameraMeasurer(model, [p, q, p], frame_buffer=fb)
    assert all(x.drop_empty and x.frame_buffer == fb for x in mc.params)
    singles = [vti_amd.StitchMeasurer(model, x, frame_buffer=fb) for x in (p, q, p)]
    dq = [(deque(maxlen=fb), deque(maxlen=fb)) for _ in range(n_cams)]
    rng = np.random.default_rng(11)
    for _ in range(12):                      # batches of mixed size; the deques carry over from batch to batch
        B = int(rng.integers(1, 9))
        cams = rng.integers(0, n_cams, B)
        f64 = np.where(rng.uniform(size=(B, 2)) < 0.3, np.nan, rng.uniform(1, 15, (B, 2)))
        i32 = np.stack([rng.choice([0, 0, 0, 1, 2, 3], B), np.full(B, 5), np.ones(B, int), np.full(B, 4), rng.integers(0, 9, B),
                        np.full(B, 5)], 1).astype(np.int32)
        got = mc._records(f64, i32, cams.tolist())
        assert [g["camera"] for g in got] == cams.tolist()
        for b, c in enumerate(cams.tolist()):
            g = got[b]
            one = singles[c]._record(f64[b], i32[b])                   # a StitchMeasurer that only ever sees camera c
            assert {k: v for k, v in g.items() if k not in ("timestamp", "camera")} == {k: v for k, v in one.items() if k != "timestamp"}
            status = int(i32[b, 0])
            if status:
                assert g["error"] == {1: "Fabric not detected", 2: "No stitches detected", 3: "Unknown camera"}[status]
                assert g["edge_distance_mm"] is None and g["stitch_width_mm"] is None and g["stitch_count"] == 0
                continue
            exp = []
            for v, d in zip(f64[b], dq[c]):
                if np.isnan(v):
                    exp.append(None)
                else:
                    d.append(float(v))
                    exp.append(float(np.median(d)))
            assert (g["edge_distance_mm"], g["stitch_width_mm"], g["stitch_count"]) == (exp[0], exp[1], int(i32[b, 4])) and "error" not in g
    assert [len(s.dist) for s in mc.streams] == [len(d[0]) for d in dq]
