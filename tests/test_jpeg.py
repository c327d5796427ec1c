"""jpeg.py, the host restatement of vti_encode_jpeg, against libjpeg's bytes: tests/golden/jpeg_pillow.npz holds what Pillow
(libjpeg-turbo) wrote for the seeded frames of jpeg_util.py (Image.save(format="JPEG", quality=q, subsampling=2, optimize=False)),
whole files, header included.  The symbol histograms prove that the set reaches the corners of the Huffman coder; with PIL installed
a wider sweep is compared live.  The device is held to jpeg.py in test_gpu_jpeg.py."""
import io
import os

import numpy as np
import pytest

import jpeg_util as J
from vti_amd import jpeg

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_pillow.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k].tobytes() for k in z.files if k != "pillow_version"}


def _scan(b):
    return b[jpeg.HEADER_BYTES:-2]


def test_encode_equals_libjpegs_bytes(golden):
    assert len(golden) == len(J.cases()) == 60
    for c in J.cases():
        got = jpeg.encode(J.frame(*c[:3]), c[3])
        want = golden[J.key(*c)]
        assert got == want, (c, len(got), len(want), next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), None))


def test_header_is_the_files_first_623_bytes(golden):
    for c in J.cases():
        hdr = jpeg.header(c[1], c[2], c[3])
        assert len(hdr) == jpeg.HEADER_BYTES == 623 and golden[J.key(*c)].startswith(hdr), c
        assert golden[J.key(*c)].endswith(b"\xff\xd9")
    hdr = jpeg.header(960, 1280, 95)
    assert hdr[:4] == b"\xff\xd8\xff\xe0" and hdr[6:11] == b"JFIF\x00" and hdr[-14:-12] == b"\xff\xda"
    assert [i for i in range(len(hdr) - 1) if hdr[i] == 0xFF and hdr[i + 1] == 0xC4].__len__() == 4        # four DHT segments
    for bad in ((0, 8, 95), (8, 0, 95), (8, 8, 0), (8, 8, 101), (65536, 8, 95)):
        with pytest.raises(ValueError):
            jpeg.header(*bad)


def test_the_set_reaches_the_corners_of_the_huffman_coder(golden):
    """ZRL, EOB, a size-11 DC difference, a size-10 AC coefficient, stuffed bytes: asserted so the cases cannot silently go soft."""
    tot = {k: np.zeros(n, np.int64) for k, n in (("dc0", 12), ("ac0", 256), ("dc1", 12), ("ac1", 256))}
    per = {}
    for c in J.cases():
        sc = jpeg.symbol_counts(J.frame(*c[:3]), c[3])
        per[c] = sc
        for k in tot:
            assert sc[k].shape == tot[k].shape and sc[k].dtype == np.int64
            tot[k] += sc[k]
    assert tot["ac0"][0xF0] > 0 and tot["ac1"][0xF0] > 0                       # ZRL in both AC tables
    assert tot["ac0"][0x00] > 0 and tot["ac1"][0x00] > 0                       # EOB
    assert per[("checker", 17, 33, 100)]["dc0"][11] > 0                        # black next to white at Q = 1: |diff| = 2040
    assert tot["dc1"][11] > 0
    assert per[("ramp", 17, 33, 100)]["ac0"][10::16].sum() > 0                 # the comb: a size-10 AC coefficient
    assert per[("zrl", 16, 16, 95)]["ac0"][0xF0] == 12                         # 4 blocks x 3 ZRL in front of coefficient 63
    assert per[("zrl", 16, 16, 95)]["ac0"][0x00] == 0                          # ... so no EOB in them
    assert all(tot["dc0"][s] > 0 for s in range(12))                           # every DC size
    assert sum(_scan(b).count(b"\xff\x00") for b in golden.values()) >= 100     # stuffed bytes
    # one DC symbol per block and table: 17 x 33 has 2 x 3 MCUs = 24 luma and 6 + 6 chroma blocks, dummy blocks included
    sc = per[("noise", 17, 33, 95)]
    assert sc["dc0"].sum() == 24 and sc["dc1"].sum() == 12


def test_dummy_blocks_right_and_below():
    """17 x 33: 3 x 5 real luma blocks in 2 x 3 MCUs.  The right column of the last MCU column and the bottom row of the last MCU row
    are libjpeg's dummy blocks: zero AC, the DC of the block before them in the MCU."""
    coef, is_chroma = jpeg.scan_blocks(J.frame("noise", 17, 33), 95)
    coef = coef.reshape(2, 3, 6, 64)
    assert is_chroma.reshape(2, 3, 6)[0, 0].tolist() == [False] * 4 + [True] * 2
    assert coef[0, 0, :4, 1:].any(axis=1).all()                                # a full MCU: four real blocks
    right = coef[0, 2]
    assert right[0, 1:].any() and not right[1, 1:].any() and right[1, 0] == right[0, 0]
    assert right[2, 1:].any() and not right[3, 1:].any() and right[3, 0] == right[2, 0]
    below = coef[1, 0]
    assert below[0, 1:].any() and below[1, 1:].any()
    assert not below[2:4, 1:].any() and below[2, 0] == below[1, 0] and below[3, 0] == below[1, 0]
    corner = coef[1, 2]
    assert not corner[1:4, 1:].any() and (corner[1:4, 0] == corner[0, 0]).all()      # (its real block is one replicated pixel)
    assert coef[:, :2, 4:, 1:].any(axis=3).all()                               # chroma never needs them


def test_rgb_on_the_flipped_frame_gives_the_same_bytes():
    for c in (("noise", 17, 33, 95), ("ramp", 50, 70, 95), ("tiles", 17, 33, 100)):
        f = J.frame(*c[:3])
        assert jpeg.encode(np.ascontiguousarray(f[..., ::-1]), c[3], rgb=True) == jpeg.encode(f, c[3])
        assert jpeg.encode(f, c[3], rgb=True) != jpeg.encode(f, c[3]) or c[0] == "checker"


def test_quant_tables_and_bad_frames():
    qy, qc = jpeg.quant_tables(100)
    assert (qy == 1).all() and (qc == 1).all()
    qy, qc = jpeg.quant_tables(50)
    assert qy[0] == 16 and qc[0] == 17 and qy[63] == 99
    qy, qc = jpeg.quant_tables(1)
    assert (qy == 255).all()                                                   # force_baseline clamps at 255
    qy, _ = jpeg.quant_tables(95)
    assert qy[:8].tolist() == [2, 1, 1, 2, 2, 4, 5, 6]
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 3), np.float32), np.zeros((0, 4, 3), np.uint8), np.zeros((4, 4, 4), np.uint8)):
        with pytest.raises(ValueError):
            jpeg.encode(bad)


def test_live_sweep_against_pillow():
    PIL = pytest.importorskip("PIL")
    from PIL import Image
    rng = np.random.Generator(np.random.PCG64(7))
    n = 0
    for (h, w) in [(1, 1), (2, 3), (8, 8), (9, 7), (15, 31), (16, 16), (17, 33), (24, 40), (40, 56), (50, 70), (64, 64), (120, 200)]:
        for q in (100, 95, 75, 60, 50, 10, 1):
            for content in ("noise", "ramp", "tiles", "zrl", "smooth"):
                if content == "smooth":                 # low-pass noise: long zero runs and small coefficients, as camera frames have
                    f = rng.integers(0, 256, (h // 8 + 2, w // 8 + 2, 3)).astype(np.float64)
                    f = np.repeat(np.repeat(f, 8, axis=0), 8, axis=1)[:h, :w] + rng.normal(0, 3, (h, w, 3))
                    f = np.clip(np.rint(f), 0, 255).astype(np.uint8)
                else:
                    f = J.frame(content, h, w, seed=q)
                buf = io.BytesIO()
                Image.fromarray(np.ascontiguousarray(f[..., ::-1])).save(buf, format="JPEG", quality=q, subsampling=2, optimize=False)
                assert jpeg.encode(f, q) == buf.getvalue(), (PIL.__version__, h, w, q, content)
                n += 1
    assert n == 12 * 7 * 5
