"""jpeg.decode / jpeg.parse, the host specification of vti_decode_jpeg, against libjpeg's pixels: tests/golden/jpeg_decode_pillow.npz
holds Pillow's (libjpeg-turbo's) files and np.asarray(Image.open(file)) for the cases of jpeg_decode_util.golden_cases(); with PIL
installed a wider sweep is compared live.  The device is held to jpeg.decode in test_gpu_jpeg_decode.py, the kernels' arithmetic on
the host in test_jpeg_decode_host.py."""
import io
import os

import numpy as np
import pytest

import jpeg_decode_util as U
import jpeg_util as J
from vti_amd import jpeg

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_decode_pillow.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files if k != "pillow_version"}


def test_decode_equals_pillows_pixels(golden):
    cases = U.golden_cases()
    assert len(golden) == 2 * len(cases) and len(cases) >= 80
    seen = set()
    for key, content, h, w, ss, q, opts in cases:
        data, want = golden["file_" + key].tobytes(), golden["rgb_" + key]
        hdr = jpeg.parse(data)
        assert (hdr["H0"], hdr["W0"]) == (h, w) == want.shape[:2] and (hdr["hs"], hdr["vs"]) == U.SAMPLINGS[ss], key
        got = jpeg.decode(data)
        assert got.dtype == np.uint8 and got.shape == want.shape
        assert np.array_equal(got, want), (key, int(np.abs(got.astype(int) - want).max()), np.argwhere((got != want).any(-1))[:4].tolist())
        assert np.array_equal(jpeg.decode(data, rgb=False), want[..., ::-1]), key
        seen.add((ss, q))
        seen.update(opts)
        if hdr["restart_interval"]:
            seen.add("dri")
    # the set spans what the issue lists
    assert {(ss, q) for ss in U.SAMPLINGS for q in (95, 100, 50, 10, 1)} <= seen
    assert {"optimize", "restart_marker_blocks", "restart_marker_rows", "strip_dht", "dri"} <= seen
    assert {c[1] for c in cases} == set(J.CONTENTS)


def test_the_golden_set_reaches_the_decoders_corners(golden):
    """Restart intervals, files without DHT, optimised tables that differ from Annex K, planes too narrow for fancy upsampling."""
    k = "ramp_50x70_444_q95_nodht"
    assert b"\xff\xc4" not in golden["file_" + k].tobytes()[:400] and jpeg.parse(golden["file_" + k].tobytes())["dc"][0] == jpeg.DC0
    opt = jpeg.parse(golden["file_ramp_50x70_422_q95_opt"].tobytes())
    assert opt["ac"][0] != jpeg.AC0
    rr = jpeg.parse(golden["file_checker_135x241_420_q50_rr1"].tobytes())
    assert rr["restart_interval"] == rr["mcu_cols"] and rr["mcu_rows"] > 8          # the RSTn numbering wraps
    rb = jpeg.parse(golden["file_noise_17x33_444_q95_rb2"].tobytes())
    assert rb["restart_interval"] == 2
    assert jpeg.parse(golden["file_ramp_3x5_420_q95"].tobytes())["W0"] == 5          # 3 chroma columns: fancy; 9 x 4: 2 columns, replicated
    assert jpeg.parse(golden["file_ramp_9x4_422_q95"].tobytes())["W0"] == 4


def test_decode_of_the_packages_own_files_equals_pillows():
    PIL = pytest.importorskip("PIL.Image")
    for (h, w) in ((1, 1), (17, 33), (50, 70)):
        for q in (95, 10):
            for c in ("noise", "ramp", "tiles"):
                data = jpeg.encode(J.frame(c, h, w), q)
                want = np.asarray(PIL.open(io.BytesIO(data)))
                assert np.array_equal(jpeg.decode(data), want), (h, w, q, c)
    for ss in U.SAMPLINGS:          # and of the test generator's files (4:2:2, 4:4:4, DRI, no DHT)
        for rst, dht in ((0, True), (3, False)):
            data = U.own_file(J.frame("ramp", 17, 33), 90, ss, rst, dht)
            assert np.array_equal(jpeg.decode(data), np.asarray(PIL.open(io.BytesIO(data)))), (ss, rst, dht)


def test_live_sweep_against_pillow():
    PIL = pytest.importorskip("PIL.Image")
    rng = np.random.Generator(np.random.PCG64(7))
    n = 0
    for i in range(320):
        h, w = (int(rng.integers(1, 40)), int(rng.integers(1, 40))) if i % 8 else (int(rng.integers(40, 150)), int(rng.integers(40, 250)))
        c = J.CONTENTS[i % len(J.CONTENTS)]
        ss = list(U.SAMPLINGS)[int(rng.integers(3))]
        q = int(rng.choice([1, 5, 10, 30, 50, 75, 90, 95, 100]))
        opts = [{}, dict(optimize=True), dict(restart_marker_blocks=int(rng.integers(1, 9))), dict(restart_marker_rows=1)][int(rng.integers(4))]
        if c == "noise" and h * w > 4000:
            opts = {}                        # Pillow's encoder buffer does not hold an optimised noise file of that size
        buf = io.BytesIO()
        PIL.fromarray(np.ascontiguousarray(J.frame(c, h, w, seed=i)[..., ::-1])).save(buf, format="JPEG", quality=q,
                                                                                     subsampling=U.PIL_SUBSAMPLING[ss], **opts)
        data = buf.getvalue()
        want = np.asarray(PIL.open(io.BytesIO(data)))
        got = jpeg.decode(data)
        assert np.array_equal(got, want), (i, h, w, c, ss, q, opts, int(np.abs(got.astype(int) - want).max()))
        n += 1
    assert n == 320


def _sof(data):
    return next(a for m, a, b in U.segments(data) if m == 0xC0)


def test_parse_refuses_what_the_decoder_does_not_support(golden):
    base = golden["file_ramp_17x33_422_q95_all"].tobytes()
    sof, sos = _sof(base), next(a for m, a, b in U.segments(base) if m == 0xDA)
    dqt = next(a for m, a, b in U.segments(base) if m == 0xDB)

    def patched(at, value):
        d = bytearray(base)
        d[at] = value
        return bytes(d)
    refused = {
        "progressive": patched(sof + 1, 0xC2),
        "arithmetic": patched(sof + 1, 0xC9),
        "12-bit": patched(sof + 4, 12),
        "sampling": patched(sof + 11, 0x41),                # 4:1:1
        "chroma sampling": patched(sof + 14, 0x21),
        "16-bit quantisation": patched(dqt + 4, 0x10),
        "size": patched(sof + 5, 0x40),                     # H0 = 16401
        "spectral selection": patched(sos + 12, 5),
    }
    # Adobe transform 0 (RGB data) in an APP14 segment after SOI
    refused["Adobe transform"] = base[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00" + base[2:]
    # greyscale: one component; four components
    refused["greyscale"] = base[:sof + 2] + b"\x00\x0b" + base[sof + 4:sof + 9] + b"\x01\x01\x11\x00" + base[sof + 19:]
    refused["components"] = base[:sof + 2] + b"\x00\x14" + base[sof + 4:sof + 9] + b"\x04\x01\x11\x00\x02\x11\x01\x03\x11\x01\x04\x11\x01" + base[sof + 19:]
    # a second scan after the first
    refused["multiple scans"] = base[:-2] + base[sos:sos + 14] + b"\x00\xff\xd9"
    # a scan of one component
    refused["scan"] = base[:sos + 2] + b"\x00\x08\x01\x01\x00\x00\x3f\x00" + base[sos + 14:]
    for name, data in refused.items():
        with pytest.raises(jpeg.UnsupportedJpeg) as e:
            jpeg.parse(data)
        assert str(e.value), name
        with pytest.raises(jpeg.UnsupportedJpeg):
            jpeg.decode(data)
    assert "progressive" in str(pytest.raises(jpeg.UnsupportedJpeg, jpeg.parse, refused["progressive"]).value)
    assert "Adobe" in str(pytest.raises(jpeg.UnsupportedJpeg, jpeg.parse, refused["Adobe transform"]).value)
    assert "greyscale" in str(pytest.raises(jpeg.UnsupportedJpeg, jpeg.parse, refused["greyscale"]).value)
    assert issubclass(jpeg.UnsupportedJpeg, ValueError)
    # malformed, not unsupported
    for data in (b"", b"\xff\xd8", base[:100], base[:sos], b"\x00" + base[1:], base[:20] + b"\x00" + base[21:]):
        with pytest.raises(ValueError) as e:
            jpeg.parse(data)
        assert not isinstance(e.value, jpeg.UnsupportedJpeg), data[:8]
    # what IS accepted: COM and APPn segments, fill bytes in front of a marker
    ok = base[:2] + b"\xff\xfe\x00\x05abc" + b"\xff\xff\xff" + base[2:]
    assert np.array_equal(jpeg.decode(ok), jpeg.decode(base))


def test_pillow_writes_the_refused_classes():
    PIL = pytest.importorskip("PIL.Image")
    f = J.frame("ramp", 17, 33)
    for kw, mode in ((dict(progressive=True), "RGB"), ({}, "L"), ({}, "CMYK")):
        buf = io.BytesIO()
        PIL.fromarray(f).convert(mode).save(buf, format="JPEG", **kw)
        with pytest.raises(jpeg.UnsupportedJpeg):
            jpeg.parse(buf.getvalue())


def test_a_damaged_scan_is_reported_and_stays_in_bounds(golden):
    data = golden["file_checker_135x241_420_q95"].tobytes()
    hdr = jpeg.parse(data)
    coef, ok = jpeg.decode_coefficients(data, hdr)
    assert ok and coef.shape == (hdr["n_blocks"], 64)
    half = data[:(hdr["scan_start"] + hdr["scan_end"]) // 2]
    assert jpeg.decode_coefficients(half)[1] is False and jpeg.decode(half).shape == (135, 241, 3)
    rr = golden["file_checker_135x241_420_q50_rr1"].tobytes()
    assert jpeg.decode_coefficients(rr)[1]
    at = rr.index(b"\xff\xd3")
    assert jpeg.decode_coefficients(rr[:at + 1] + b"\xd5" + rr[at + 2:])[1] is False       # a misnumbered RSTn
