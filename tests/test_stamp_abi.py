"""vti_stamp and vti_stamp_frames without a GPU: every argument check returns VTI_ERR_ARG with a message that names the function and
what is wrong -- the stamp's or the picture's index where there is one -- before the first HIP call (fake device pointers, never
dereferenced; every call here is refused, so none launches anything), and the stand-alone program tests/stamp_args_main.cpp drives the
packer and the same refusals clean under the host sanitizers.  The expected messages are this file's own."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import stamp_util as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(37, 53), (64, 96), (8, 8)]


def _at(n):
    return C.c_void_p(4096 + n)


def _hp(t):
    return C.c_void_p(t.data_ptr())


def _patched(host, at, fmt_value):
    """A copy of a packed host table with the int32 at byte `at` replaced."""
    c = host.clone()
    c[at:at + 4] = torch.from_numpy(np.array([fmt_value], "<i4").view(np.uint8).copy())
    return c


def _setup(vti_amd, shapes):
    eng = vti_amd.Engine("n", 2, H=64, W=96, max_batch=4)
    rng = np.random.default_rng(5)
    per = [[S.random_stamp(rng, 1, 2, 33, 4), S.random_stamp(rng, 0, 0, 5, 5)], [], [S.random_stamp(rng, 2, 2, 6, 6)]]
    return eng, eng.pack_stamps(per, shapes, device="cpu")


def _refusals(L, eng, fn, call, good, faults):
    for needle, over in faults:
        a = dict(good, **over)
        rc = call(a)
        msg = (L.vti_last_error(eng._ctx) or b"").decode()
        assert rc == -1 and msg.startswith(fn + ":") and needle in msg, (needle, over, rc, msg)


def _table_faults(t, n_pictures):
    """Single faults in the stamp table pair and the bit buffer, shared by both entry points: (needle, overrides)."""
    rec0 = 64 + 16 * n_pictures                      # the first record: offset i64, x, y, w, h, pitch, colour
    junk = (C.c_uint8 * 256)()
    keep = [_patched(t.host, rec0 + 32 + 16, 0), _patched(t.host, rec0 + 8, 60), _patched(t.host, rec0 + 64 + 24, 0),
            _patched(t.host, 64 + 8, 1), _patched(t.host, 64 + 16 + 12, 1), _patched(t.host, 8, 4), junk]
    return keep, [("null stamp table", dict(ht=None)), ("null stamp table", dict(dt=None)),
                  ("device stamp table must be 16-byte aligned", dict(dt=_at(8))), ("dev_bits must be 4-byte aligned", dict(bits=_at(2))),
                  ("null dev_bits", dict(bits=None)), ("not a table of vti_pack_stamps", dict(ht=C.cast(junk, C.c_void_p))),
                  ("another n_words", dict(n_words=t.n_words + 1)), ("another n_words", dict(n_words=0)),
                  ("stamp 1 of host_table: w and h must be >= 1", dict(ht=_hp(keep[0]))),                  # record 1: w = 0
                  ("stamp 0 of host_table: the rectangle is not inside its picture", dict(ht=_hp(keep[1]))),   # record 0: x = 60
                  ("stamp 2 of host_table: pitch must be >= ceil(w / 32)", dict(ht=_hp(keep[2]))),         # record 2: pitch = 0
                  ("picture 0 of host_table: its range of stamps", dict(ht=_hp(keep[3]))),                 # picture 0 begins at 1
                  ("picture 1 of host_table: its range of stamps", dict(ht=_hp(keep[4]))),                 # picture 1 ends before it begins
                  ("do not cover its stamps", dict(ht=_hp(keep[5])))]                                      # the header says 4 stamps


def test_vti_stamp_checks_every_argument_before_any_hip_call(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    eng, t = _setup(vti_amd, [(37, 53)] * 3)
    good = dict(ctx=eng._ctx, pics=_at(0), n=3, H0=37, W0=53, ht=_hp(t.host), dt=_at(0), bits=_at(0), n_words=t.n_words)
    call = lambda a: L.vti_stamp(a["ctx"], a["pics"], a["n"], a["H0"], a["W0"], a["ht"], a["dt"], a["bits"], a["n_words"], None)
    assert call(dict(good, ctx=None)) == -1
    keep, faults = _table_faults(t, 3)
    _refusals(L, eng, "vti_stamp", call, good, faults + [
        ("null pointer", dict(pics=None)), ("bad size", dict(n=0)), ("bad size", dict(n=4097)), ("bad size", dict(H0=0)),
        ("bad size", dict(W0=8193)), ("another number of pictures", dict(n=2)), ("another number of pictures", dict(n=4)),
        ("picture 0 of the stamp table is 37 x 53, the call's is 38 x 53", dict(H0=38)),
        ("picture 0 of the stamp table is 37 x 53, the call's is 37 x 52", dict(W0=52))])
    # a table without stamps needs no bit buffer, and is still checked
    e = eng.pack_stamps([[], []], [(5, 7)] * 2, device="cpu")
    empty = dict(good, n=2, H0=5, W0=7, ht=_hp(e.host), bits=None, n_words=0)
    _refusals(L, eng, "vti_stamp", call, empty, [("another number of pictures", dict(n=3)), ("is 5 x 7, the call's is 5 x 8", dict(W0=8))])


def test_vti_stamp_frames_checks_both_tables_before_any_hip_call(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    eng, t = _setup(vti_amd, SHAPES)
    ft, _, _ = eng.pack_frames(SHAPES, device="cpu")
    other_sizes, _, _ = eng.pack_frames([(37, 53), (64, 95), (8, 8)], device="cpu")
    other_canvas, _, _ = vti_amd.Engine("n", 2, H=96, W=96, max_batch=4).pack_frames(SHAPES, device="cpu")
    four, _, _ = eng.pack_frames(SHAPES + [(8, 8)], device="cpu")
    bad_row = ft.host.clone()
    bad_row[64 + 64 * 1] = 1                         # row 1: a byte offset that is no multiple of 16
    good = dict(ctx=eng._ctx, buf=_at(0), hft=_hp(ft.host), dft=_at(0), n=3, ht=_hp(t.host), dt=_at(0), bits=_at(0), n_words=t.n_words)
    call = lambda a: L.vti_stamp_frames(a["ctx"], a["buf"], a["hft"], a["dft"], a["n"], a["ht"], a["dt"], a["bits"], a["n_words"], None)
    assert call(dict(good, ctx=None)) == -1
    keep, faults = _table_faults(t, 3)
    _refusals(L, eng, "vti_stamp_frames", call, good, faults + [
        ("null frame table", dict(hft=None)), ("null frame table", dict(dft=None)), ("device frame table must be 16-byte aligned", dict(dft=_at(8))),
        ("packed for another B", dict(n=2)), ("packed for another B", dict(n=0)), ("packed for another B", dict(hft=_hp(four.host))),
        ("another canvas", dict(hft=_hp(other_canvas.host))), ("frame 1 of host_table", dict(hft=C.c_void_p(bad_row.data_ptr()))),
        ("null pointer", dict(buf=None)), ("dev_buf must be 16-byte aligned", dict(buf=_at(8))),
        ("picture 1 of the stamp table is 64 x 96, the call's is 64 x 95", dict(hft=_hp(other_sizes.host)))])
    # a frame above 8192 is named before the stamp table is looked at
    tall, _, _ = eng.pack_frames([(8200, 8200)], device="cpu")
    _refusals(L, eng, "vti_stamp_frames", call, dict(good, n=1, hft=_hp(tall.host)), [("frame 0 is 8200 x 8200", {})])


def test_engine_stamp_refuses_what_does_not_fit_before_it_touches_a_device(lib_built):
    vti_amd = lib_built
    eng, t = _setup(vti_amd, [(37, 53)] * 3)
    with pytest.raises(ValueError, match="StampTable"):
        eng.stamp(torch.zeros((3, 37, 53, 3), dtype=torch.uint8), None)
    with pytest.raises(ValueError, match="uint8"):
        eng.stamp(torch.zeros((3, 37, 53, 3)), t)
    for shape in ((2, 37, 53, 3), (3, 37, 54, 3)):
        with pytest.raises(ValueError, match="other sizes"):
            eng.stamp(torch.zeros(shape, dtype=torch.uint8), t)
    with pytest.raises(ValueError, match="device tensor"):                          # a good call on host memory stops at the device check
        eng.stamp(torch.zeros((3, 37, 53, 3), dtype=torch.uint8), t)
    ft, _, _ = eng.pack_frames(SHAPES, device="cpu")
    with pytest.raises(ValueError, match="other sizes"):
        eng.stamp(torch.zeros(ft.total_bytes, dtype=torch.uint8), t, table=ft)
    with pytest.raises(ValueError, match="flat uint8"):
        eng.stamp(torch.zeros((3, 37, 53, 3), dtype=torch.uint8), _setup(vti_amd, SHAPES)[1], table=ft)


def test_the_packer_and_the_refusals_run_clean_in_a_stand_alone_program_under_the_host_sanitizers(lib_built, tmp_path):
    """tests/stamp_args_main.cpp: its own main, built with -fsanitize=address,undefined, linked against libvti.so and run directly
    (nothing is loaded into Python, nothing is preloaded).  The tables it packs live in heap blocks of exactly their size; every
    vti_stamp / vti_stamp_frames call it makes is refused before the first HIP call."""
    vti_amd = lib_built
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    lib_dir = os.path.dirname(vti_amd.LIB_PATH)
    exe = str(tmp_path / "stamp_args_main")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx).startswith("g++") else []    # no link-order rule to meet
    subprocess.run([cxx, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static, "-I",
                    os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "stamp_args_main.cpp"), "-L", lib_dir, "-lvti",
                    "-Wl,-rpath," + lib_dir, "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and re.fullmatch(r"ok \d+\n", run.stdout) and run.stderr == "", (run.returncode, run.stdout, run.stderr)
    assert int(run.stdout.split()[1]) >= 40
