"""The NMS table without a GPU: the three entry points are declared with their marker, exported and bound; the size query; the packer
names the row and the field of what it refuses, is deterministic and packs a set of every class as no set; the setter refuses on the
host (fake device pointers, never dereferenced) and clears; YOLO.predict(classes=) and the rig stages' per-camera sequences refuse
bad values before a device is touched; and the stand-alone program tests/nms_table_args_main.cpp repeats the pack and setter refusals
clean under the host sanitizers.  The GPU parity tests are in test_gpu_nms_table.py."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vti_nms_table_bytes", "vti_pack_nms_table", "vti_set_nms_table")
ARG, STATE, UNSUPPORTED = -1, -2, -6


def _args(hdr, name):
    decl = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, hdr).group(1)
    return [" ".join(a.split()) for a in decl.split(",")]


def test_the_three_entry_points_are_declared_with_the_marker_exported_and_bound(lib_built):
    vti_amd = lib_built
    hdr = open(os.path.join(ROOT, "include", "vti.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", vti_amd.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert re.search(r"^#define VTI_NMS_TABLE_API$", hdr, re.M)
    marked = re.findall(r"^VTI_NMS_TABLE_API (?:int32_t|int64_t)\s+(vti_\w+)\s*\(", hdr, re.M)
    assert tuple(marked) == NAMES
    for name in NAMES:
        assert re.search(r"\bT %s$" % name, exported, re.M), name
        assert name in vti_amd.SIGNATURES and hasattr(vti_amd.lib(), name)
    unmarked = len(re.findall(r"^(?:int32_t|int64_t|void|const char\*)\s+vti_\w+\s*\(", hdr, re.M))
    assert unmarked == 73                                               # the count the README states stays what it was
    assert _args(hdr, NAMES[0]) == ["int32_t n_rows"]
    assert _args(hdr, NAMES[1]) == ["vti_ctx* ctx", "const vti_nms_params* params", "int32_t n_rows", "void* host_table", "size_t nbytes"]
    assert _args(hdr, NAMES[2]) == ["vti_ctx* ctx", "const void* host_table", "const void* dev_table", "int32_t n_rows",
                                    "const int32_t* dev_row_of_frame"]
    struct = re.search(r"typedef struct \{([^}]*)\} vti_nms_params;", hdr).group(1)
    fields = re.findall(r"^\s*((?:const )?\w+\*?)\s+(\w+);", struct, re.M)
    assert fields == [("float", "conf"), ("int32_t", "max_det"), ("double", "iou"), ("int32_t", "agnostic"), ("int32_t", "n_classes"),
                      ("const int32_t*", "classes")]
    S = vti_amd._lib.VtiNmsParams
    assert [f[0] for f in S._fields_] == [n for _, n in fields] and C.sizeof(S) == 32 and S.iou.offset == 8 and S.classes.offset == 24
    limits = {k: int(v) for k, v in re.findall(r"(VTI_NMS_TABLE_MAX_\w+) = (\d+)", hdr)}
    assert limits == {"VTI_NMS_TABLE_MAX_ROWS": vti_amd._lib.VTI_NMS_TABLE_MAX_ROWS,
                      "VTI_NMS_TABLE_MAX_CLASSES": vti_amd._lib.VTI_NMS_TABLE_MAX_CLASSES}
    assert limits["VTI_NMS_TABLE_MAX_CLASSES"] >= 1024 and limits["VTI_NMS_TABLE_MAX_CLASSES"] % 32 == 0
    for public in ("NmsParams", "NmsTable"):
        assert public in vti_amd.__all__ and hasattr(vti_amd, public)
    for meth in ("pack_nms_table", "nms_table"):
        assert callable(getattr(vti_amd.Engine, meth))
    for meth in ("predict_into", "predict_frames_into"):
        p = inspect.signature(getattr(vti_amd.Engine, meth)).parameters
        assert list(p)[-1] == "nms" and p["nms"].default is None
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "and the three NMS-table calls, marked `VTI_NMS_TABLE_API`" in readme and all(n in readme for n in NAMES[1:])


def test_the_size_query(lib_built):
    L = lib_built.lib()
    for n in (0, -1, -(1 << 31), lib_built._lib.VTI_NMS_TABLE_MAX_ROWS + 1):
        assert L.vti_nms_table_bytes(n) == 0
    one, two, most = L.vti_nms_table_bytes(1), L.vti_nms_table_bytes(2), L.vti_nms_table_bytes(lib_built._lib.VTI_NMS_TABLE_MAX_ROWS)
    row = two - one
    assert one > row > 0 and row % 16 == 0 and (one - row) % 16 == 0          # a header and 16-byte aligned rows
    assert row >= 24 + lib_built._lib.VTI_NMS_TABLE_MAX_CLASSES // 8           # the settings and a bit per class
    assert most == one + (lib_built._lib.VTI_NMS_TABLE_MAX_ROWS - 1) * row


def _pack(vti_amd, eng, rows, short=0, table=True, n_rows=None, ctx=True):
    """rows: dicts of vti_nms_params' fields (classes: a list or None; n_classes may be forced) -> (rc, message, bytes)."""
    L = vti_amd.lib()
    S = vti_amd._lib.VtiNmsParams
    keep, arr = [], (S * max(len(rows), 1))()
    for k, r in enumerate(rows):
        ids = (C.c_int32 * len(r["classes"]))(*r["classes"]) if r.get("classes") else None
        keep.append(ids)
        arr[k] = S(r.get("conf", 0.25), r.get("max_det", 300), r.get("iou", 0.7), r.get("agnostic", 0),
                   r.get("n_classes", len(r["classes"]) if r.get("classes") else 0), C.cast(ids, C.POINTER(C.c_int32)) if ids else None)
    n = len(rows) if n_rows is None else n_rows
    nbytes = max(int(L.vti_nms_table_bytes(max(len(rows), 1))), 64)
    buf = (C.c_uint8 * nbytes)(*([0x5A] * nbytes))
    c = eng._ctx if ctx else None
    rc = L.vti_pack_nms_table(c, arr if rows else None, n, buf if table else None, nbytes - short)
    return rc, (L.vti_last_error(c) or b"").decode(), bytes(buf)


GOOD = [dict(conf=0.2, iou=0.25, max_det=200), dict(conf=0.5, iou=0.45, max_det=20, agnostic=1, classes=[1]), dict(classes=[2, 0, 2])]


def test_the_packer_names_the_row_and_the_field(lib_built):
    vti_amd = lib_built
    eng = vti_amd.Engine("n", 3, H=64, W=64, max_batch=2)
    rc, msg, _ = _pack(vti_amd, eng, GOOD)
    assert rc == 0, msg
    nan, inf = float("nan"), float("inf")
    cases = [(0, dict(conf=-0.1), "conf"), (1, dict(conf=1.5), "conf"), (2, dict(conf=nan), "conf"), (1, dict(conf=inf), "conf"),
             (0, dict(iou=-0.1), "iou"), (1, dict(iou=1.5), "iou"), (2, dict(iou=nan), "iou"), (0, dict(iou=-inf), "iou"),
             (1, dict(max_det=0), "max_det"), (2, dict(max_det=-5), "max_det"), (0, dict(agnostic=2), "agnostic"),
             (1, dict(agnostic=-1), "agnostic"), (2, dict(classes=[0, -1]), r"classes\[1\] = -1"),
             (1, dict(classes=[3]), r"classes\[0\] = 3 is outside \[0, 3\)"), (0, dict(classes=None, n_classes=2), "classes is NULL"),
             (2, dict(classes=None, n_classes=-1), "n_classes")]
    for row, change, needle in cases:
        rows = [dict(r) for r in GOOD]
        rows[row].update(change)
        rc, msg, _ = _pack(vti_amd, eng, rows)
        assert rc == ARG and re.match(r"vti_pack_nms_table: row %d: .*%s" % (row, needle), msg), (row, change, rc, msg)
    # the FIRST failing row is the one named
    rows = [dict(r) for r in GOOD]
    rows[1]["iou"], rows[2]["conf"] = 2.0, 2.0
    assert "row 1: iou" in _pack(vti_amd, eng, rows)[1]
    for kw, needle in ((dict(short=1), "smaller than"), (dict(table=False), "null"), (dict(n_rows=0), "n_rows"), (dict(n_rows=-1), "n_rows")):
        rc, msg, _ = _pack(vti_amd, eng, GOOD, **kw)
        assert rc == ARG and msg.startswith("vti_pack_nms_table:") and needle in msg, (kw, rc, msg)
    assert _pack(vti_amd, eng, [], n_rows=1)[0] == ARG                       # no params
    assert _pack(vti_amd, eng, GOOD, ctx=False)[0] == ARG                    # the ctx gives nc
    # the limits of the settings themselves are accepted
    assert _pack(vti_amd, eng, [dict(conf=0.0, iou=0.0, max_det=1), dict(conf=1.0, iou=1.0, max_det=(1 << 31) - 1, agnostic=1)])[0] == 0


def test_a_class_set_needs_a_model_the_mask_covers(lib_built):
    vti_amd = lib_built
    wide = vti_amd.Engine("s", vti_amd._lib.VTI_NMS_TABLE_MAX_CLASSES + 1, H=64, W=64, max_batch=1)
    rc, msg, _ = _pack(vti_amd, wide, [dict(), dict(classes=[5])])
    assert rc == UNSUPPORTED and msg.startswith("vti_pack_nms_table: row 1:") and "1024" in msg
    assert _pack(vti_amd, wide, [dict(), dict()])[0] == 0                    # without a class set any nc packs
    edge = vti_amd.Engine("s", vti_amd._lib.VTI_NMS_TABLE_MAX_CLASSES, H=64, W=64, max_batch=1)
    assert _pack(vti_amd, edge, [dict(classes=[0, 1023])])[0] == 0


def test_pack_is_deterministic_and_a_set_of_every_class_is_no_set(lib_built):
    vti_amd = lib_built
    eng = vti_amd.Engine("n", 3, H=64, W=64, max_batch=2)
    a, b = _pack(vti_amd, eng, GOOD)[2], _pack(vti_amd, eng, GOOD)[2]
    assert a == b and 0x5A not in set(a[:16])                                # every byte of the table is written
    rows = [dict(r) for r in GOOD]
    rows[0]["classes"] = [2, 1, 0, 1]
    assert _pack(vti_amd, eng, rows)[2] == a                                 # all three classes named == none named
    rows[2]["classes"] = [0, 2]                                              # order and duplicates do not matter
    assert _pack(vti_amd, eng, rows)[2] == a
    rows[2]["classes"] = [0, 1]
    assert _pack(vti_amd, eng, rows)[2] != a
    t = eng.pack_nms_table([vti_amd.NmsParams(0.2, 0.25, 200), vti_amd.NmsParams(0.5, 0.45, 20, True, (1,)),
                            vti_amd.NmsParams(classes=(2, 0, 2))], device="cpu")
    assert bytes(t.host.numpy()) == a[:t.host.numel()] and t.n_rows == 3 and isinstance(t, vti_amd.NmsTable)
    with pytest.raises(ValueError, match="at least one row"):
        eng.pack_nms_table([], device="cpu")
    with pytest.raises(ValueError, match="row 1: an empty class set"):
        eng.pack_nms_table([vti_amd.NmsParams(), vti_amd.NmsParams(classes=())], device="cpu")
    with pytest.raises(vti_amd.VtiError, match="row 0: conf"):
        eng.pack_nms_table([vti_amd.NmsParams(conf=2.0)], device="cpu")


def test_the_setter_refuses_on_the_host_and_clears(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    eng = vti_amd.Engine("n", 3, H=64, W=64, max_batch=2)
    other = vti_amd.Engine("n", 2, H=64, W=64, max_batch=2)
    t = eng.pack_nms_table([vti_amd.NmsParams(0.2, 0.25, 200), vti_amd.NmsParams(0.5, 0.45, 20, True, (1,))], device="cpu")
    host, dev, idx = C.c_void_p(t.host.data_ptr()), C.c_void_p(4096), C.c_void_p(8192)      # fake device pointers, never dereferenced

    def refused(ctx, *args):
        rc = L.vti_set_nms_table(ctx, *args)
        msg = (L.vti_last_error(ctx) or b"").decode()
        assert rc == ARG and msg.startswith("vti_set_nms_table:"), (rc, msg)
        return msg
    assert "16-byte" in refused(eng._ctx, host, C.c_void_p(4096 + 8), 2, idx)
    assert "dev_table" in refused(eng._ctx, host, None, 2, idx)
    assert "4-byte" in refused(eng._ctx, host, dev, 2, C.c_void_p(8192 + 2))
    assert "n_rows" in refused(eng._ctx, host, dev, 1, idx) and "n_rows" in refused(eng._ctx, host, dev, 3, idx)
    assert "n_rows" in refused(eng._ctx, host, dev, 0, idx)
    assert "class count" in refused(other._ctx, host, dev, 2, idx)
    hurt = t.host.clone()
    hurt[0] ^= 0xFF
    assert "not a table" in refused(eng._ctx, C.c_void_p(hurt.data_ptr()), dev, 2, idx)
    assert L.vti_set_nms_table(None, host, dev, 2, idx) == ARG
    one = C.c_void_p(16)

    def nms_stops_where_it_did():
        assert L.vti_nms(eng._ctx, one, 1, 0.25, 0.7, 10, 0, one, one, None) == STATE           # the workspace is not set
        assert L.vti_nms(eng._ctx, one, 5, 0.25, 0.7, 10, 0, one, one, None) == ARG             # B > max_batch
        assert L.vti_nms_scored(eng._ctx, one, None, 1, 0.25, 0.7, 10, 0, one, one, None) in (ARG, STATE)
        assert L.vti_predict(eng._ctx, one, 1, 64, 64, 1, 0.25, 0.7, 10, 0, 0, 1, one, one, one, one, one, one, 10, one, one, None) == STATE
    nms_stops_where_it_did()
    assert L.vti_set_nms_table(eng._ctx, host, dev, 2, idx) == 0
    nms_stops_where_it_did()                                                 # with a table set the calls' own checks still come first
    assert L.vti_set_nms_table(eng._ctx, host, dev, 2, None) == 0            # NULL index: row 0 for every frame
    refused(eng._ctx, host, C.c_void_p(4096 + 4), 2, idx)                    # a refused set leaves the installed table alone ...
    assert L.vti_set_nms_table(eng._ctx, None, None, 0, None) == 0           # ... and clearing works, whatever the other arguments are
    assert L.vti_set_nms_table(eng._ctx, None, dev, 7, idx) == 0
    nms_stops_where_it_did()
    with pytest.raises(ValueError, match="NmsTable"):
        with eng.nms_table(t.host):
            pass
    with pytest.raises(ValueError, match=r"row index outside \[0, 2\)"):
        with eng.nms_table(t, [0, 2]):
            pass
    with pytest.raises(ValueError, match="at most 2 integers"):
        with eng.nms_table(t, [0, 1, 0]):
            pass


def test_predict_refuses_bad_classes_before_an_engine_exists(lib_built, monkeypatch):
    vti_amd = lib_built
    model = vti_amd.YOLO(None, scale="n", nc=3, seed=3)
    frame = np.zeros((64, 64, 3), np.uint8)
    for bad in ([], (), [3], -1, 3, [0, -1], 1.0, [0.5], "1", [True], True, np.zeros((2, 2), np.int64), torch.tensor([0.0]), torch.tensor([7])):
        with pytest.raises(ValueError, match="predict: classes"):
            model.predict(frame, classes=bad)
    assert model._engines == {}

    def no_predict(*a, **k):
        assert k.get("nms") is not None
        raise AssertionError("predict was reached")
    monkeypatch.setattr(model, "_predict_outputs", no_predict)
    for good in (1, [0], (2, 0, 2), np.array([1, 2]), torch.tensor([2]), np.int64(0), range(3)):
        with pytest.raises(AssertionError, match="predict was reached"):
            model.predict(frame, classes=good)
    assert model._engines == {}
    assert vti_amd.YOLO._classes_arg((2, 0, 2), 3) == (0, 2) and vti_amd.YOLO._classes_arg(None, 3) is None

    def table_free(*a, **k):
        assert k.get("nms") is None                                          # without classes the call path is the table-free one
        raise AssertionError("predict was reached")
    monkeypatch.setattr(model, "_predict_outputs", table_free)
    with pytest.raises(AssertionError, match="predict was reached"):
        model.predict(frame)
    sig = inspect.signature(vti_amd.YOLO.predict)
    names = list(sig.parameters)
    assert sig.parameters["classes"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["classes"].default is None
    assert names.index("classes") == names.index("polygons") - 1
    assert names.index("polygons") == len(names) - 2 and sig.parameters[names[-1]].kind is inspect.Parameter.VAR_KEYWORD


def test_the_rig_stages_refuse_a_sequence_of_the_wrong_length_before_predict(lib_built, monkeypatch):
    vti_amd = lib_built
    from test_oracle_geometry import load_calib
    model = vti_amd.YOLO(None, scale="n", nc=2, seed=3)
    seen = []

    def no_predict(*a, **k):
        seen.append((a, k))
        raise AssertionError("predict was reached")
    monkeypatch.setattr(model, "_predict_outputs", no_predict)
    monkeypatch.setattr(model, "_predict_outputs_frames", no_predict)
    mp = vti_amd.MeasureParams(*load_calib())
    calib = load_calib()
    cp = vti_amd.CheckerParams(*calib)
    rigs = (vti_amd.MultiCameraMeasurer(model, [mp, mp]), vti_amd.MultiCameraChecker(model, [cp, cp]))
    frames = np.zeros((3, 48, 64, 3), np.uint8)
    for rig in rigs:
        for kw in (dict(conf=[0.2]), dict(iou=[0.25, 0.45, 0.5]), dict(max_det=[200, 20, 5]), dict(conf=[0.2, 0.5], iou=(0.1,)),
                   dict(max_det=np.array([5])), dict(conf=torch.tensor([0.1, 0.2, 0.3]))):
            with pytest.raises(ValueError, match=r"process_frames: (conf|iou|max_det) has \d entries but the rig has 2 cameras"):
                rig.process_frames(frames, [0, 1, 0], **kw)
        with pytest.raises(ValueError, match="max_det must be >= 1"):
            rig.process_frames(frames, [0, 1, 0], max_det=[0, 5])
        assert seen == []
        # sequences of the right length get as far as the predict, with one row per camera and the largest max_det as the stride
        with pytest.raises(AssertionError, match="predict was reached"):
            rig.process_frames(frames, [0, 1, 0], conf=[0.2, 0.5], iou=[0.25, 0.45], max_det=[200, 20])
        a, k = seen.pop()
        assert a[3] == 200 and callable(k["nms"])
        # scalars keep the table-free path
        with pytest.raises(AssertionError, match="predict was reached"):
            rig.process_frames(frames, [0, 1, 0], conf=0.3, iou=0.5, max_det=50)
        a, k = seen.pop()
        assert a[1:4] == (0.3, 0.5, 50) and k["nms"] is None
    rows = vti_amd.measure._DeviceStage._per_camera_nms(2, [0.2, 0.5], 0.25, (200, 20))[3]
    assert rows == (vti_amd.NmsParams(0.2, 0.25, 200, False, None), vti_amd.NmsParams(0.5, 0.25, 20, False, None))
    # the signatures are the old ones
    assert list(inspect.signature(vti_amd.MultiCameraChecker.process_frames).parameters)[:6] == ["self", "frames", "cameras", "conf", "iou", "max_det"]


def test_the_refusals_run_clean_in_a_stand_alone_program_under_the_host_sanitizers(lib_built, tmp_path):
    """tests/nms_table_args_main.cpp: its own main, built with -fsanitize=address,undefined, linked against libvti.so and run
    directly (nothing is loaded into Python, nothing is preloaded).  Pack and set are host only: no call it makes reaches HIP."""
    vti_amd = lib_built
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    lib_dir = os.path.dirname(vti_amd.LIB_PATH)
    exe = str(tmp_path / "nms_table_args_main")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx).startswith("g++") else []    # no link-order rule to meet
    subprocess.run([cxx, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static, "-I",
                    os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "nms_table_args_main.cpp"), "-L", lib_dir, "-lvti",
                    "-Wl,-rpath," + lib_dir, "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and re.fullmatch(r"ok \d+\n", run.stdout) and run.stderr == "", (run.returncode, run.stdout, run.stderr)
    assert int(run.stdout.split()[1]) >= 40
