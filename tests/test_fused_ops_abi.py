"""vti_debug_set_conv_output and vti_debug_run_op on the host: their signatures in all three layers, every refusal that needs no
device (fake pointers that are never dereferenced, as in test_misc_ops_abi.py), and the conv indices vti_debug_run_op reports per
op of the default plans.  vti_debug_run_op makes its argument checks before its state checks, so that they can be pinned here;
vti_debug_set_conv_output refuses in the reader's order (state first), and what lies behind the state checks -- `i` out of range,
a view that is not materialised -- is pinned on the device by test_gpu_fused_ops.py."""
import ctypes as C
import os
import re

import pytest

from gpu_util import plan_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = C.c_void_p(4096)        # never dereferenced
H, W, MAXB = 224, 352, 3


def _engine(vti_amd, monkeypatch, dtype, env=None):
    plan_env(monkeypatch, env or {})
    return vti_amd.Engine("n", 80, H=H, W=W, max_batch=MAXB, dtype=dtype)


def _run(vti_amd, eng, i, B=MAXB, x=ONE, pred=ONE, proto=ONE, best=None):
    L = vti_amd.lib()
    convs = (C.c_int32 * 4)(7, 7, 7, 7)
    rc = L.vti_debug_run_op(eng._ctx, i, x, B, 0, pred, proto, best, convs, None)
    return rc, (L.vti_last_error(eng._ctx) or b"").decode(), list(convs)


def test_signatures_in_all_three_layers(lib_built):
    vti_amd = lib_built
    hdr = open(os.path.join(ROOT, "include", "vti.h")).read()
    sig = vti_amd._lib.SIGNATURES
    for name, nargs in (("vti_debug_set_conv_output", 5), ("vti_debug_run_op", 10)):
        m = re.search(r"VTI_DEBUG_OPS_API int32_t " + name + r"\(([^;]*)\);", hdr)
        assert m, f"{name} is not declared VTI_DEBUG_OPS_API in vti.h"
        assert len(m.group(1).split(",")) == nargs == len(sig[name][1]) and sig[name][0] is C.c_int32
        assert hasattr(vti_amd.lib(), name)
    assert sig["vti_debug_set_conv_output"] == sig["vti_debug_conv_output"]        # the inverse: same arguments
    assert callable(vti_amd.Engine.debug_set_conv_output) and callable(vti_amd.Engine.debug_run_op)


@pytest.mark.parametrize("dtype", ["fp16", "fp32", "h2"])
def test_run_op_refusals(lib_built, monkeypatch, dtype):
    vti_amd = lib_built
    eng = _engine(vti_amd, monkeypatch, dtype)
    table = eng.conv_table()
    names = [t["name"] for t in table]
    n = len(table)
    stem, cls2, mc2, cv3 = 0, names.index("model.22.cv3.1.2"), names.index("model.22.cv4.2.2"), names.index("model.22.proto.cv3")
    mid = names.index("model.4.m.0.cv1")

    def refused(needle, code=-1, **kw):
        rc, msg, _ = _run(vti_amd, eng, **kw)
        assert rc == code and msg.startswith("vti_debug_run_op: ") and needle in msg, (kw, rc, msg)

    assert vti_amd.lib().vti_debug_run_op(None, 0, ONE, 1, 0, ONE, ONE, None, None, None) == -1
    for i in (-1, n, 1 << 30):
        refused("i out of range", i=i)
    for B in (0, -1, MAXB + 1):
        refused("B out of range", i=mid, B=B)
    refused("dev_input", i=stem, x=None)
    refused("dev_input", i=1, x=None)             # layer 1 lives in the stem's op
    refused("dev_pred", i=cls2, pred=None)
    refused("dev_pred", i=cls2 - 1, pred=None)     # the tower's 3x3: the same op
    refused("dev_pred", i=mc2, pred=None)
    refused("dev_proto", i=cv3, proto=None)
    # the argument checks come first, then vti_forward's state errors; nothing that an op does not use is asked for
    refused("weights not loaded", code=-2, i=mid, x=None, pred=None, proto=None)
    refused("weights not loaded", code=-2, i=stem, pred=None, proto=None)
    refused("weights not loaded", code=-2, i=cls2, x=None, proto=None)
    refused("weights not loaded", code=-2, i=cv3, x=None, pred=None)


def test_set_conv_output_refuses_as_the_reader_does(lib_built, monkeypatch):
    vti_amd = lib_built
    L = vti_amd.lib()
    eng = _engine(vti_amd, monkeypatch, "h2")
    assert L.vti_debug_set_conv_output(None, 0, 1, ONE, None) == L.vti_debug_conv_output(None, 0, 1, ONE, None) == -1
    for i, B in ((3, 1), (3, MAXB + 1), (3, -1), (-1, 1), (999, 1), (3, 0)):
        got = []
        for fn in ("vti_debug_conv_output", "vti_debug_set_conv_output"):
            rc = getattr(L, fn)(eng._ctx, i, B, ONE, None)
            msg = L.vti_last_error(eng._ctx).decode()
            assert msg.startswith(fn + ": "), msg
            got.append((rc, msg[len(fn):]))
        assert got[0] == got[1] and got[0][0] == (-1 if not 0 <= B <= MAXB else -2), (i, B, got)


# the ops of the default 224x352 plans by the convs they compute, per dtype: what test_gpu_fused_ops.py relies on when it names
# a family by one of its convs (absent: the dtype's plan does not fuse that family)
OPS = {
    "stem": {"h2": ["model.0", "model.1", "model.2.cv1"], "fp16": ["model.0", "model.1", "model.2.cv1"], "fp32": ["model.0", "model.1", "model.2.cv1"]},
}


@pytest.mark.parametrize("dtype", ["fp16", "fp32", "h2"])
def test_out_convs_name_the_op_in_execution_order(lib_built, monkeypatch, dtype):
    """Every conv of the plan belongs to exactly one op; asking for any conv of an op reports the same list; a list starts with
    the conv the op is named after except behind the folded ConvTranspose; fused rows follow their producer."""
    vti_amd = lib_built
    eng = _engine(vti_amd, monkeypatch, dtype)
    table = eng.conv_table()
    names = [t["name"] for t in table]
    seen = {}
    for i in range(len(table)):
        rc, msg, convs = _run(vti_amd, eng, i)
        assert rc == -2, (i, rc, msg)                  # no weights: refused after the list was written
        live = [c for c in convs if c >= 0]
        assert live and i in live and convs == live + [-1] * (4 - len(live)) and len(set(live)) == len(live), (i, convs)
        seen.setdefault(tuple(live), []).append(i)
    assert sorted(i for v in seen.values() for i in v) == list(range(len(table)))
    assert all(sorted(k) == v for k, v in seen.items()), seen          # one list per op, whichever member asks
    ops = {names[k[0]]: [names[c] for c in k] for k in seen}
    assert ops["model.0"] == OPS["stem"][dtype]
    fold = ops.get("model.22.proto.upsample")
    assert fold == ["model.22.proto.upsample", "model.22.proto.cv2", "model.22.proto.cv3"], ops
    assert ops["model.2.m.0.cv1"][:2] == ["model.2.m.0.cv1", "model.2.m.0.cv2"]
    for k in seen:
        for a, b in zip(k, k[1:]):
            assert table[b]["fused"] or names[b].endswith("proto.cv2"), (names[a], names[b])
    if dtype != "fp32":     # the closing 1x1 of model.2 in the pair's tail (the fp32 plan keeps it an op of its own)
        assert ops["model.2.m.0.cv1"] == ["model.2.m.0.cv1", "model.2.m.0.cv2", "model.2.cv2"]
    for lvl in range(3):
        for tower in ("cv2", "cv3", "cv4"):
            assert ops[f"model.22.{tower}.{lvl}.1"] == [f"model.22.{tower}.{lvl}.1", f"model.22.{tower}.{lvl}.2"]
