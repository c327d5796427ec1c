"""The refusals of the single-kernel debug entry points (vti_debug_sppf_pool, vti_debug_upsample2x, vti_debug_decode) and the
class-count limit of the full decode kernel, on the host: fake pointers that are never dereferenced, as in abi_refusal_cases.py.
Every case here is refused before the first HIP call, so nothing is launched."""
import ctypes as C

import pytest

from gpu_util import plan_env

F16, F32, H2 = 0, 1, 2


def _at(n):
    return C.c_void_p(n)


BUF, BUF2 = 1 << 20, 1 << 30          # two "device buffers" far apart


def _refused(vti_amd, name, order, base, over, needle):
    L = vti_amd.lib()
    a = dict(base, **over)
    rc = getattr(L, name)(*[a[k] for k in order])
    msg = (L.vti_last_error(None) or b"").decode()
    assert rc == -1 and msg.startswith(name + ": ") and needle in msg, (over, rc, msg)


POOL_ORDER = ["dtype", "din", "dout", "B", "H", "W", "C", "ld", "in_coff", "out_coff", "path", "stream"]
POOL_BASE = dict(dtype=F16, din=_at(BUF), dout=_at(BUF), B=2, H=7, W=11, C=32, ld=128, in_coff=0, out_coff=32, path=None, stream=None)
POOL_FAULTS = [
    (dict(dtype=3), "dtype"), (dict(dtype=-1), "dtype"), (dict(din=None), "null"), (dict(dout=None), "null"),
    (dict(din=_at(BUF + 8)), "16-byte"), (dict(dout=_at(BUF2 + 4)), "16-byte"),
    (dict(B=0), ">= 1"), (dict(H=0), ">= 1"), (dict(W=-3), ">= 1"), (dict(C=0), ">= 1"), (dict(ld=0), ">= 1"), (dict(in_coff=-8), ">= 0"),
    (dict(out_coff=-8), ">= 0"),
    (dict(C=28), "multiples"), (dict(ld=132), "multiples"), (dict(in_coff=4, out_coff=36), "multiples"), (dict(out_coff=36), "multiples"),
    (dict(dtype=F32, C=6, ld=64, out_coff=8), "multiples"), (dict(dtype=H2, C=8, ld=66, out_coff=8), "multiples"),
    (dict(dtype=H2, C=8, ld=64, in_coff=2, out_coff=16), "multiples"),
    (dict(in_coff=104, out_coff=0), "do not fit"), (dict(out_coff=40), "do not fit"), (dict(C=48, ld=128, out_coff=48), "do not fit"),
    (dict(C=1 << 30, ld=1 << 30), "do not fit"),
    (dict(out_coff=0, in_coff=64), "overlap"), (dict(in_coff=32, out_coff=0, C=16, ld=64), "overlap"), (dict(out_coff=0, in_coff=0, ld=256), "overlap"),
    (dict(dout=_at(BUF + 16)), "do not overlap"), (dict(dout=_at(BUF + 2 * 7 * 11 * 128 * 2 - 16)), "do not overlap"),
    (dict(B=1 << 15, H=1 << 8, W=1 << 8, ld=128), "2^31"),
]
UP_ORDER = ["dtype", "din", "dout", "B", "H", "W", "C", "in_ld", "in_coff", "out_ld", "out_coff", "stream"]
UP_BASE = dict(dtype=F32, din=_at(BUF), dout=_at(BUF2), B=2, H=7, W=11, C=16, in_ld=32, in_coff=8, out_ld=48, out_coff=24, stream=None)
UP_FAULTS = [
    (dict(dtype=7), "dtype"), (dict(din=None), "null"), (dict(dout=None), "null"), (dict(din=_at(BUF + 4)), "16-byte"),
    (dict(B=0), ">= 1"), (dict(H=-1), ">= 1"), (dict(W=0), ">= 1"), (dict(C=0), ">= 1"), (dict(in_ld=0), ">= 1"), (dict(out_ld=-4), ">= 1"),
    (dict(out_coff=-4), ">= 0"),
    (dict(C=18), "multiples"), (dict(in_ld=34), "multiples"), (dict(in_coff=6), "multiples"), (dict(out_ld=50), "multiples"),
    (dict(out_coff=26), "multiples"), (dict(dtype=F16, C=16, in_coff=4), "multiples"), (dict(dtype=H2, out_coff=22), "multiples"),
    (dict(in_coff=24), "do not fit"), (dict(out_coff=36), "do not fit"),
    (dict(dout=_at(BUF)), "overlap"), (dict(dout=_at(BUF + 2 * 7 * 11 * 32 * 4 - 16)), "overlap"),
    (dict(din=_at(BUF2 + 2 * 14 * 22 * 48 * 4 - 16)), "overlap"),
    (dict(B=1 << 14, H=1 << 7, W=1 << 7, out_ld=48), "2^31"),
]


def _ptrs(*v):
    return (C.c_void_p * 3)(*v)


def _i32(*v):
    return (C.c_int32 * 3)(*v)


DEC_ORDER = ["box_only", "box", "cls", "mc", "H", "W", "stride", "B", "nc", "nm", "pred", "stream"]
DEC_BASE = dict(box_only=0, box=_ptrs(BUF, BUF + 4096, BUF + 8192), cls=_ptrs(BUF2, BUF2 + 4096, BUF2 + 8192),
                mc=_ptrs(3 * BUF, 3 * BUF + 4096, 3 * BUF + 8192), H=_i32(7, 4, 2), W=_i32(11, 6, 3), stride=_i32(8, 16, 32), B=2, nc=80, nm=32,
                pred=_at(5 * BUF), stream=None)
DEC_FAULTS = [
    (dict(box_only=2), "box_only"), (dict(box_only=-1), "box_only"),
    (dict(box=None), "null"), (dict(cls=None), "null"), (dict(mc=None), "null"), (dict(H=None), "null"), (dict(W=None), "null"),
    (dict(stride=None), "null"), (dict(pred=None), "null"), (dict(box_only=1, box=None), "null"),
    (dict(box=_ptrs(BUF, 0, BUF + 8192)), "level 1: null"), (dict(cls=_ptrs(0, BUF2, BUF2)), "level 0: null"),
    (dict(mc=_ptrs(BUF2, BUF2, 0)), "level 2: null"), (dict(box_only=1, box=_ptrs(BUF, BUF, 0)), "level 2: null"),
    (dict(box=_ptrs(BUF, BUF + 2, BUF)), "4-byte"), (dict(pred=_at(5 * BUF + 1)), "4-byte"), (dict(mc=_ptrs(BUF2, BUF2, BUF2 + 3)), "4-byte"),
    (dict(B=0), ">= 1"), (dict(nc=0), ">= 1"), (dict(nm=0), ">= 1"), (dict(nm=-32), ">= 1"),
    (dict(H=_i32(7, 0, 2)), "level 1"), (dict(W=_i32(11, 6, -3)), "level 2"), (dict(stride=_i32(0, 16, 32)), "level 0"),
    (dict(nc=16288), "nc + nm = 16320 is above VTI_DECODE_MAX_CHANNELS = 16319"), (dict(nc=16256, nm=64), "VTI_DECODE_MAX_CHANNELS = 16319"),
    (dict(nc=(1 << 31) - 1, nm=(1 << 31) - 1), "VTI_DECODE_MAX_CHANNELS = 16319"),
    (dict(H=_i32(1 << 15, 4, 2), W=_i32(1 << 15, 6, 3)), "2^31"), (dict(H=_i32(1 << 16, 1 << 16, 2), W=_i32(1 << 14, 1 << 14, 3)), "2^31"),
    (dict(box_only=1, nc=1 << 30, nm=1 << 30, cls=None, mc=None), "2^31"),
]


@pytest.mark.parametrize("i", range(len(POOL_FAULTS)))
def test_sppf_pool_refusals(lib_built, i):
    _refused(lib_built, "vti_debug_sppf_pool", POOL_ORDER, POOL_BASE, *POOL_FAULTS[i])


@pytest.mark.parametrize("i", range(len(UP_FAULTS)))
def test_upsample2x_refusals(lib_built, i):
    _refused(lib_built, "vti_debug_upsample2x", UP_ORDER, UP_BASE, *UP_FAULTS[i])


@pytest.mark.parametrize("i", range(len(DEC_FAULTS)))
def test_decode_refusals(lib_built, i):
    _refused(lib_built, "vti_debug_decode", DEC_ORDER, DEC_BASE, *DEC_FAULTS[i])


def test_the_baselines_differ_from_their_faults_in_one_argument():
    """Each fault overrides the valid baseline call, which itself cannot be issued without a device: what makes it valid is stated
    here, next to the cases, so that a fault is refused for its own reason."""
    p = POOL_BASE
    assert p["C"] % 8 == 0 and p["ld"] % 8 == 0 and p["in_coff"] + p["C"] <= p["out_coff"] and p["out_coff"] + 3 * p["C"] <= p["ld"]
    u = UP_BASE
    assert u["in_coff"] + u["C"] <= u["in_ld"] and u["out_coff"] + u["C"] <= u["out_ld"] and all(u[k] % 4 == 0 for k in ("C", "in_ld", "in_coff", "out_ld", "out_coff"))
    assert DEC_BASE["nc"] + DEC_BASE["nm"] <= 16319


def test_full_decode_plans_state_their_class_limit_at_create(lib_built, monkeypatch):
    """launch_decode keeps its anchors' rows of 64 + nc + nm + 1 floats in 64 KiB of LDS: 64 anchors per workgroup up to
    nc + nm = 191, fewer above that (test_gpu_misc_ops.py runs 160 and 1025 classes), and one row has to fit: nc + nm <= 16319.
    A plan that keeps that kernel -- VTI_NO_PRED_SCATTER=1, or the default plan of 160 classes and more -- is refused above the
    limit when the engine is created, with a message that names it, not by a bare HIP error at its first forward."""
    vti_amd = lib_built          # scale s: its class towers are 128 wide whatever nc (scale n: min(nc, 100), no multiple of 16)
    for env in ({"VTI_NO_PRED_SCATTER": "1"}, {}):
        plan_env(monkeypatch, env)
        for nc, nm in ((159, 32), (160, 32), (1025, 32), (16287, 32), (16255, 64)):
            assert vti_amd.Engine("s", nc, nm=nm, H=64, W=64, max_batch=1).num_anchors == 84
        for nc, nm in ((16288, 32), (16256, 64), (100000, 32)):
            with pytest.raises(vti_amd.VtiError) as ei:
                vti_amd.Engine("s", nc, nm=nm, H=64, W=64, max_batch=1)
            assert ei.value.code == -1 and "vti_create" in str(ei.value)
            assert f"nc + nm = {nc + nm} is above VTI_DECODE_MAX_CHANNELS = 16319" in str(ei.value)
