"""The text of the annotated pictures as 1-bit stamps, without a GPU: annotate.stamp (the restatement vti_stamp is compared against),
annotate.text_stamps with an injected rasteriser, the host-only packer vti_pack_stamps through ctypes (a table parsed back; every
refusal names the stamp), and what process_frames refuses about burn_text before anything is predicted.  The refusals of vti_stamp
and vti_stamp_frames are in test_stamp_abi.py, the device in test_gpu_stamp.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import stamp_util as S
from test_oracle_geometry import load_calib
from vti_amd import annotate as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vti_stamp_table_bytes", "vti_pack_stamps", "vti_stamp", "vti_stamp_frames")


# ---- annotate.stamp ---------------------------------------------------------------------------------------------------------------
def test_stamp_paints_in_list_order_and_in_place():
    rng = np.random.default_rng(0)
    pic = rng.integers(0, 256, (20, 30, 3), dtype=np.uint8)
    a = (2, 3, np.ones((6, 8), bool), (1, 2, 3))
    b = (6, 5, np.ones((6, 8), bool), (9, 8, 7))
    ab, ba = pic.copy(), pic.copy()
    assert A.stamp(ab, [a, b]) is ab and A.stamp(ba, [b, a]) is ba
    assert (ab[5:9, 6:10] == (9, 8, 7)).all() and (ba[5:9, 6:10] == (1, 2, 3)).all()        # the overlap is the later stamp's
    assert (ab[3:5, 2:10] == (1, 2, 3)).all() and (ab[9:11, 6:14] == (9, 8, 7)).all()
    untouched = np.ones((20, 30), bool)
    untouched[3:9, 2:10] = untouched[5:11, 6:14] = False
    assert np.array_equal(ab[untouched], pic[untouched]) and np.array_equal(ba[untouched], pic[untouched])


def test_stamp_of_all_zeros_of_all_ones_and_of_a_pattern():
    rng = np.random.default_rng(1)
    pic = rng.integers(0, 256, (17, 23, 3), dtype=np.uint8)
    zeros = pic.copy()
    A.stamp(zeros, [(0, 0, np.zeros((17, 23), bool), (5, 5, 5))])
    assert np.array_equal(zeros, pic)
    ones = pic.copy()
    A.stamp(ones, [(0, 0, np.ones((17, 23), bool), (5, 6, 7))])
    assert (ones == (5, 6, 7)).all()
    bits = rng.integers(0, 2, (9, 11)).astype(bool)
    got = A.stamp(pic.copy(), [(12, 8, bits, (200, 100, 50))])                     # ends at the last column and the last row
    want = pic.copy()
    for r in range(9):
        for c in range(11):
            if bits[r, c]:
                want[8 + r, 12 + c] = (200, 100, 50)
    assert np.array_equal(got, want)
    assert A.stamp(pic, []) is pic
    with pytest.raises(ValueError, match="not inside"):
        A.stamp(pic.copy(), [(13, 8, bits, (1, 1, 1))])


# ---- annotate.text_stamps -----------------------------------------------------------------------------------------------------------
def _items(h, w):
    return [S.item("rect 9 5", (3, 4), (10, 20, 30)), S.item("frame 12 7", (5, 6), (40, 50, 60)),          # overlapping, in order
            S.item("diag 40", (w - 11, h - 9), (0, 0, 255)),                                              # leaves by the corner
            S.item("rect 6 6", (-3, -2), (1, 2, 3)), S.item("anti 15", (2, 5), (7, 7, 7)),                 # clipped by the top left
            S.item("rect 4 4", (w, 3), (9, 9, 9)), S.item("diag 5", (-20, -20), (9, 9, 9)),                # wholly outside
            S.item("none", (5, 5), (9, 9, 9)), S.item("frame 50 50", (w - 20, -10), (70, 80, 90)),
            S.item("Edge Dist: 3.25mm | Avg Width: 4.10mm (n_d=5, n_w=4)", (10, 30), (0, 0, 255), 0.7, 2),
            S.item("12.3", (w - 8, h + 2), (0, 0, 0), 0.6, 2), S.item("rect %d %d" % (w, h), (0, 0), (3, 3, 3)),
            S.item("rect 3 3", (4, 4), (250, 0, 0))]


@pytest.mark.parametrize("h,w", [(37, 53), (97, 131)])
def test_text_stamps_reproduce_what_the_rasteriser_drew(h, w):
    rng = np.random.default_rng(2)
    pic = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    items = _items(h, w)
    want, drew = S.painted(pic, items)
    stamps = A.text_stamps(items, h, w, S.rasterise)
    assert drew == len(items) - 3 and len(stamps) == drew                          # the three items that draw nothing give no stamp
    assert np.array_equal(A.stamp(pic.copy(), stamps), want)
    for x, y, bits, colour in stamps:                                               # cropped to the bounding box, inside the picture
        assert bits.dtype == bool and bits[0].any() and bits[-1].any() and bits[:, 0].any() and bits[:, -1].any()
        assert 0 <= x and 0 <= y and y + bits.shape[0] <= h and x + bits.shape[1] <= w
    assert [s[3] for s in stamps] == [it[4] for it in items if S.painted(pic, [it])[1]]
    # the canvas kept for this size is clean again: the same call gives the same stamps, an empty list gives none
    again = A.text_stamps(items, h, w, S.rasterise)
    assert len(again) == len(stamps) and all(a[:2] == b[:2] and np.array_equal(a[2], b[2]) for a, b in zip(again, stamps))
    assert A.text_stamps([], h, w, S.rasterise) == []
    assert not A._CANVASES[(h, w)].any()


def test_text_stamps_leave_a_clean_canvas_behind_a_rasteriser_that_raised():
    def broken(canvas, it):
        canvas[2:4, 2:4] = 1
        raise RuntimeError("no glyphs")
    with pytest.raises(RuntimeError):
        A.text_stamps([S.item("x", (0, 0), (1, 1, 1))], 11, 13, broken)
    assert A.text_stamps([S.item("none", (0, 0), (1, 1, 1))], 11, 13, S.rasterise) == []


def test_without_opencv_the_default_rasteriser_is_an_import_error():
    try:
        import cv2  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError):
            A.text_stamps([S.item("x", (5, 5), (1, 1, 1))], 20, 20)
        with pytest.raises(ImportError):
            A.put_text(np.zeros((20, 20, 3), np.uint8), [S.item("x", (5, 5), (1, 1, 1))])


# ---- the C ABI: declared, exported, bound; the packer ---------------------------------------------------------------------------------
def test_the_entry_points_are_declared_exported_and_bound(lib_built):
    vti_amd = lib_built
    hdr = open(os.path.join(ROOT, "include", "vti.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", vti_amd.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(r"\bT %s$" % name, exported, re.M) and name in vti_amd.SIGNATURES
    decl = re.search(r"int32_t\s+vti_stamp\s*\(([^)]*)\)\s*;", hdr).group(1)
    assert [" ".join(a.split()) for a in decl.split(",")] == [
        "vti_ctx* ctx", "uint8_t* dev_pictures", "int32_t n", "int32_t H0", "int32_t W0", "const void* host_table", "const void* dev_table",
        "const uint32_t* dev_bits", "int64_t n_words", "void* stream"]
    decl = re.search(r"int32_t\s+vti_stamp_frames\s*\(([^)]*)\)\s*;", hdr).group(1)
    assert [" ".join(a.split()) for a in decl.split(",")] == [
        "vti_ctx* ctx", "uint8_t* dev_buf", "const void* host_frame_table", "const void* dev_frame_table", "int32_t n",
        "const void* host_table", "const void* dev_table", "const uint32_t* dev_bits", "int64_t n_words", "void* stream"]
    assert C.sizeof(vti_amd._lib.VtiStampDesc) == 40
    limits = dict(re.findall(r"(VTI_STAMP_MAX_\w+) = ([^,}]+)", hdr))
    assert eval(limits["VTI_STAMP_MAX_PER_PICTURE"]) >= 1024 and {k: eval(v) for k, v in limits.items()} == {
        k: getattr(vti_amd._lib, k) for k in ("VTI_STAMP_MAX_PICTURES", "VTI_STAMP_MAX_PER_PICTURE", "VTI_STAMP_MAX_TOTAL", "VTI_STAMP_MAX_PITCH")}
    assert callable(A.text_stamps) and callable(A.stamp) and hasattr(vti_amd.Engine, "pack_stamps") and hasattr(vti_amd.Engine, "stamp")
    readme = open(os.path.join(ROOT, "README.md")).read()
    unmarked = len(re.findall(r"^(?:int32_t|int64_t|void|const char\*)\s+vti_\w+\s*\(", hdr, re.M))
    marked = re.findall(r"^VTI_STAMP_API (?:int32_t|int64_t)\s+(vti_\w+)\s*\(", hdr, re.M)
    assert tuple(marked) == NAMES and f"{unmarked} entry points" in readme and f"{unmarked + len(marked)} in all" in readme
    L = vti_amd.lib()
    assert L.vti_stamp_table_bytes(3, 5) == 64 + 3 * 16 + 5 * 32 and L.vti_stamp_table_bytes(1, 0) == 80
    for n, s in ((0, 1), (-1, 1), (4097, 1), (1, -1), (1, (1 << 24) + 1)):
        assert L.vti_stamp_table_bytes(n, s) == 0
    assert L.vti_stamp_table_bytes(4096, 1 << 24) > 0


SHAPES = [(131, 203), (8, 8), (37, 53), (8192, 8192)]


def _stamps(rng):
    """Per picture of SHAPES: random stamps, among them the corners, widths around a word, none at all for the second picture."""
    one = [S.random_stamp(rng, 0, 0, 17, 9), S.random_stamp(rng, 203 - 33, 131 - 4, 33, 4), S.random_stamp(rng, 5, 60, 64, 3),
           S.random_stamp(rng, 100, 20, 1, 1), S.random_stamp(rng, 7, 7, 31, 2), S.random_stamp(rng, 7, 7, 32, 2)]
    return [one, [], [S.random_stamp(rng, 0, 0, 53, 37, ones=1)], [S.random_stamp(rng, 8192 - 70, 8192 - 2, 70, 2)]]


def test_a_packed_table_reads_back_as_ranges_records_and_bits(lib_built):
    vti_amd = lib_built
    eng = vti_amd.Engine("n", 2, H=64, W=96, max_batch=1)
    rng = np.random.default_rng(3)
    per = _stamps(rng)
    for extra, fill in ((0, 0), (2, 0xDEADBEEF)):
        t = eng.pack_stamps(per, SHAPES, device="cpu", pitch_extra=extra, pad_fill=fill)
        head, pics, recs = S.read_table(t.host)
        flat = [s for p in per for s in p]
        assert head == dict(magic=0x31545356, n_pictures=4, n_stamps=len(flat), n_words=t.n_words) and t.n_stamps == len(flat)
        assert [p[:2] for p in pics] == SHAPES
        assert [(p[2], p[3]) for p in pics] == [(0, 6), (6, 6), (6, 7), (7, 8)]        # the ranges follow each other, an empty one included
        words = t.bits.numpy().view(np.uint32)
        at = 0
        for r, (x, y, bits, colour) in zip(recs, flat):
            h, w = bits.shape
            assert (r["x"], r["y"], r["w"], r["h"], r["colour"]) == (x, y, w, h, colour)
            assert r["pitch"] == -(-w // 32) + extra and r["offset"] == at
            assert np.array_equal(S.unpacked(r, words), bits)
            if fill:                                                                # the pad bits hold the pattern: they are not the stamp's
                rows = words[at:at + h * r["pitch"]].reshape(h, r["pitch"])
                assert (rows[:, -1] == fill).all()
            at += h * r["pitch"]
        assert at == t.n_words and t.up_bytes == t.host.numel() + 4 * at
        assert bytes(eng.pack_stamps(per, SHAPES, device="cpu", pitch_extra=extra, pad_fill=fill).host.numpy()) == bytes(t.host.numpy())
    empty = eng.pack_stamps([[], []], [(5, 5), (6, 6)], device="cpu")
    assert empty.n_stamps == 0 and empty.n_words == 0 and empty.bits is None and S.read_table(empty.host)[1] == [(5, 5, 0, 0), (6, 6, 0, 0)]
    with pytest.raises(ValueError):
        eng.pack_stamps([[]], [(5, 5), (6, 6)], device="cpu")


def test_every_refusal_of_the_packer_names_the_stamp(lib_built):
    vti_amd = lib_built
    L = vti_amd.lib()
    eng = vti_amd.Engine("n", 2, H=64, W=96, max_batch=1)
    D = vti_amd._lib.VtiStampDesc
    H0, W0 = (C.c_int32 * 2)(131, 37), (C.c_int32 * 2)(203, 53)
    base = [dict(picture=0, x=0, y=0, w=40, h=3, pitch=2, word_offset=0), dict(picture=0, x=163, y=128, w=40, h=3, pitch=2, word_offset=6),
            dict(picture=1, x=0, y=0, w=53, h=37, pitch=2, word_offset=12)]
    n_words = 12 + 74

    def pack(descs, n_pictures=2, n_words=n_words, ctx=eng._ctx, H0=H0, W0=W0, short=0, table=True, n_stamps=None):
        arr = (D * max(len(descs), 1))(*[D(d["picture"], d["x"], d["y"], d["w"], d["h"], d["pitch"], (C.c_uint8 * 4)(1, 2, 3, 0), 0,
                                           d["word_offset"]) for d in descs])
        ns = len(descs) if n_stamps is None else n_stamps
        nbytes = max(int(L.vti_stamp_table_bytes(max(n_pictures, 1), max(ns, 0))), 80)
        buf = (C.c_uint8 * nbytes)()
        rc = L.vti_pack_stamps(ctx, H0, W0, n_pictures, arr if descs else None, ns, n_words, buf if table else None, nbytes - short)
        return rc, (L.vti_last_error(ctx) or b"").decode()

    assert pack(base)[0] == 0
    assert pack(base, ctx=None)[0] == 0                                             # ctx only receives the text
    assert pack([], n_words=0)[0] == 0                                              # no stamps at all is a table

    def refused(needle, i, **change):
        descs = [dict(d) for d in base]
        descs[i].update(change)
        rc, msg = pack(descs)
        assert rc == -1 and msg.startswith(f"vti_pack_stamps: stamp {i}: ") and needle in msg, (change, rc, msg)

    refused("picture outside", 1, picture=2)
    refused("picture outside", 0, picture=-1)
    rc, msg = pack([base[2], base[0]])                                              # picture 1, then picture 0
    assert rc == -1 and msg.startswith("vti_pack_stamps: stamp 1: ") and "must not decrease" in msg
    refused("w and h must be >= 1", 1, w=0)
    refused("w and h must be >= 1", 2, h=0)
    refused("w and h must be >= 1", 0, h=-4)
    refused("not inside its picture", 1, x=164)                                      # one column past the right edge
    refused("not inside its picture", 1, y=129)
    refused("not inside its picture", 0, x=-1)
    refused("not inside its picture", 2, y=-1)
    refused("not inside its picture", 2, w=54)
    refused("pitch must be >= ceil(w / 32)", 0, pitch=1)
    refused("pitch must be >= ceil(w / 32)", 2, pitch=0)
    refused("VTI_STAMP_MAX_PITCH", 0, pitch=65537)
    refused("run past n_words", 2, word_offset=13)                                   # one word too far
    refused("run past n_words", 0, word_offset=-1)
    refused("run past n_words", 1, word_offset=n_words)
    # the per-picture limit: stamp 65536 of one picture is the first one too many
    many = [dict(picture=0, x=0, y=0, w=1, h=1, pitch=1, word_offset=0)] * 65537
    rc, msg = pack(many, n_pictures=1, n_words=1)
    assert rc == -1 and msg.startswith("vti_pack_stamps: stamp 65536: ") and "VTI_STAMP_MAX_PER_PICTURE" in msg
    assert pack(many[:65536], n_pictures=1, n_words=1)[0] == 0
    # what is wrong with the call as a whole names no stamp
    for needle, kw in (("n_pictures", dict(n_pictures=0)), ("n_pictures", dict(n_pictures=4097)), ("n_stamps", dict(n_stamps=-1)),
                       ("n_stamps", dict(n_stamps=(1 << 24) + 1)), ("n_words", dict(n_words=-1)), ("smaller than", dict(short=1)),
                       ("null", dict(table=False)), ("null", dict(H0=None)), ("null", dict(W0=None))):
        rc, msg = pack(base, **kw)
        assert rc == -1 and msg.startswith("vti_pack_stamps: ") and needle in msg and "stamp " not in msg.split(": ", 1)[1][:6], (kw, msg)
    rc, msg = pack(base, H0=(C.c_int32 * 2)(131, 8193))
    assert rc == -1 and "picture 1" in msg and "8192" in msg
    # a VtiError from the wrapper carries the same text
    with pytest.raises(vti_amd.VtiError, match="stamp 0: the rectangle is not inside its picture"):
        eng.pack_stamps([[(200, 0, np.ones((2, 5), bool), (1, 1, 1))]], [(131, 203)], device="cpu")


# ---- process_frames -------------------------------------------------------------------------------------------------------------------
def test_process_frames_refuses_before_anything_is_predicted(lib_built, monkeypatch):
    vti_amd = lib_built
    calib = load_calib()
    model = vti_amd.YOLO(None, scale="n", nc=2, seed=3)

    def no_predict(*a, **k):
        raise AssertionError("predict was reached")
    monkeypatch.setattr(model, "_predict_outputs", no_predict)
    monkeypatch.setattr(model, "_predict_outputs_frames", no_predict)
    frames = np.zeros((2, 48, 64, 3), np.uint8)
    extra = {0: [S.item("rect 3 3", (1, 1), (1, 2, 3))]}
    sm = vti_amd.StitchMeasurer(model, vti_amd.MeasureParams(*calib))
    mc = vti_amd.MultiCameraMeasurer(model, [vti_amd.MeasureParams(*calib)] * 2)
    ck = vti_amd.StitchDistanceChecker(model, vti_amd.CheckerParams(*calib))
    calls = (lambda **kw: sm.process_frames(frames, **kw), lambda **kw: mc.process_frames(frames, [0, 1], **kw),
             lambda **kw: mc.process_frames([frames[0], frames[1, :40]], [0, 1], mixed=True, **kw), lambda **kw: ck.process_frames(frames, **kw))
    monkeypatch.setitem(sys.modules, "cv2", None)                                  # `import cv2` is an ImportError from here on
    for call in calls:
        with pytest.raises(ValueError, match="burn_text needs annotate"):
            call(burn_text=True, rasterise=S.rasterise)
        with pytest.raises(ValueError, match="extra_text needs burn_text"):
            call(annotate="all", extra_text=extra)
        with pytest.raises(ValueError, match="extra_text needs burn_text"):
            call(extra_text={})
        with pytest.raises(ImportError):
            call(annotate="all", burn_text=True)
        with pytest.raises(AssertionError, match="predict was reached"):             # with a rasteriser the call goes on to predict
            call(annotate="all", burn_text=True, extra_text=extra, rasterise=S.rasterise)
    import inspect
    for fn in (vti_amd.StitchMeasurer._process_frames, vti_amd.MultiCameraMeasurer._process_frames, vti_amd.StitchDistanceChecker.process_frames):
        p = inspect.signature(fn).parameters
        assert [p[k].default for k in ("burn_text", "extra_text", "rasterise")] == [False, None, None]
