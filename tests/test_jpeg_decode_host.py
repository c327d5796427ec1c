"""vti_decode_jpeg's stages on the host (csrc/jpeg_decode_dev.h: plain C++ for host and device, compiled by
tests/jpeg_decode_host_cover.cpp), lane by lane on the descriptor table libvti.so's plan packs: the segment decoder, the rounds of
the self-synchronising scheme, the block-count scan with restart markers, the DC sums, IDCT, upsampling and colour conversion equal
jpeg.decode byte for byte; damaged scans end, set the status and write nothing outside their own frame, scratch and coefficients."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_decode_util as U
import jpeg_util as J
from vti_amd import jpeg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vision-textile-inspection_amd", "csrc")
POISON = 0xA5
GUARD = 4096


@pytest.fixture(scope="module")
def emulate(tmp_path_factory, lib_built):
    vti_amd = lib_built
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    cmd = [cxx, "-x", "c++"] if cxx else ["/opt/rocm/bin/hipcc", "-x", "c++"]      # the compiler build() needs is always there
    so = str(tmp_path_factory.mktemp("jcover") / "libjcover.so")
    subprocess.run(cmd + ["-O2", "-std=c++17", "-shared", "-fPIC", "-I", CSRC, "-o", so, os.path.join(ROOT, "tests", "jpeg_decode_host_cover.cpp")],
                   check=True)
    fn = ctypes.CDLL(so).jpegd_emulate
    fn.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 3 + [ctypes.c_int]
    fn.restype = None

    def run(files, segment_bytes=0, rgb=1, lanes=1024, layout=0):
        rc, p = U.plan(vti_amd, files, segment_bytes, layout)
        assert rc == 0, p["error"]
        n, total = len(files), int(p["out_off"][-1])
        out = np.full(total + GUARD, POISON, np.uint8)
        scratch = np.full(p["scratch_bytes"] + GUARD, POISON, np.uint8)
        info = np.full((n, 4), -7, np.int32)
        before = p["blob"].copy()
        fn(p["blob"].ctypes.data, p["table"].ctypes.data, n, rgb, out.ctypes.data, info.ctypes.data, scratch.ctypes.data, lanes)
        assert np.array_equal(p["blob"], before)
        assert (out[total:] == POISON).all() and (scratch[p["scratch_bytes"]:] == POISON).all()
        frames, written = [], np.zeros(total, bool)
        for k in range(n):
            a, m = int(p["out_off"][k]), 3 * int(p["H0"][k]) * int(p["W0"][k])
            frames.append(out[a:a + m].reshape(p["H0"][k], p["W0"][k], 3))
            written[a:a + m] = True
        assert (out[:total][~written] == POISON).all()          # the alignment gaps
        return frames, info
    return run


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "jpeg_decode_pillow.npz")) as z:
        return {k: z[k] for k in z.files if k != "pillow_version"}


def test_every_golden_file_at_both_segment_sizes(emulate, golden):
    for key, *_ in U.golden_cases():
        data = golden["file_" + key].tobytes()
        for seg in (16, 0):
            (got,), info = emulate([data], seg)
            assert info[0, 0] == 0 and info[0, 3] == jpeg.parse(data)["n_blocks"], (key, seg, info)
            assert np.array_equal(got, golden["rgb_" + key]), (key, seg)


def test_mixed_batches_segment_sizes_lanes_and_bgr(emulate):
    files = [U.own_file(J.frame(c, h, w), q, ss, rst, dht)
             for c, h, w, q, ss, rst, dht in (("noise", 135, 241, 100, "444", 0, True), ("ramp", 17, 33, 95, "420", 2, True),
                                              ("flat", 1, 1, 95, "422", 0, False), ("tiles", 50, 70, 10, "420", 5, False),
                                              ("zrl", 50, 70, 95, "422", 0, True), ("checker", 16, 16, 95, "444", 1, True))]
    want = [jpeg.decode(f) for f in files]
    for seg, lanes in ((16, 1024), (0, 1024), (64, 7), (4096, 64)):
        got, info = emulate(files, seg, lanes=lanes)
        for k in range(len(files)):
            assert info[k, 0] == 0 and np.array_equal(got[k], want[k]), (seg, lanes, k, info[k])
        print(f"segment_bytes {seg}: segments {info[:, 1].tolist()} rounds {info[:, 2].tolist()}")
    # 135 x 241 noise at quality 100 in 16-byte segments: blocks are several segments long, the states travel many rounds
    got, info = emulate(files[:1], 16)
    assert info[0, 1] > 1000 and info[0, 2] > 100
    bgr, _ = emulate(files, 0, rgb=0)
    assert all(np.array_equal(b, w[..., ::-1]) for b, w in zip(bgr, want))
    same, _ = emulate([files[1], files[0], files[1]])
    assert np.array_equal(same[0], same[2]) and np.array_equal(same[0], want[1])
    dense, _ = emulate([files[3], files[4]], layout=1)
    assert np.array_equal(dense[0], want[3]) and np.array_equal(dense[1], want[4])


def test_damaged_scans_end_set_the_status_and_stay_inside(emulate):
    good = U.own_file(J.frame("ramp", 50, 70), 95, "420")
    rst = U.own_file(J.frame("noise", 50, 70), 95, "422", restart=2)
    hdr, hr = jpeg.parse(good), jpeg.parse(rst)
    mid = (hdr["scan_start"] + hdr["scan_end"]) // 2
    cases = {"cut in half": good[:mid], "cut in half, EOI kept": good[:mid] + b"\xff\xd9",
             "zeros": good[:mid] + bytes(40) + good[mid + 40:], "ones": good[:mid] + b"\xff" * 40 + good[mid + 40:],
             "noise": good[:mid] + bytes(np.random.Generator(np.random.PCG64(3)).integers(1, 255, 60, dtype=np.uint8)) + good[mid + 60:],
             "no scan": good[:hdr["scan_start"]] + b"\xff\xd9"}
    at = rst.index(b"\xff\xd2", hr["scan_start"])
    cases["misnumbered RSTn"] = rst[:at + 1] + b"\xd5" + rst[at + 2:]
    cases["missing RSTn"] = rst[:at] + rst[at + 2:]
    cases["restart file cut"] = rst[:(hr["scan_start"] + hr["scan_end"]) // 2]
    want_good, want_rst = jpeg.decode(good), jpeg.decode(rst)
    for name, data in cases.items():
        for seg in (16, 0):
            got, info = emulate([good, data, rst], seg)
            assert info[:, 0].tolist() == [0, 1, 0], (name, seg, info)
            assert np.array_equal(got[0], want_good) and np.array_equal(got[2], want_rst), (name, seg)
            assert 0 <= info[1, 3] <= jpeg.parse(data)["n_blocks"] and 1 <= info[1, 2] <= max(info[1, 1], 1)
