"""retina_masks layout (host only, no GPU): Engine.mask_native_layout against Ultralytics 8.1/8.2 scale_masks' crop, computed
here in Python double, and the bit / byte row rule of vti_masks_native."""
import numpy as np
import pytest

SHAPES = [(960, 1280, 960), (640, 640, 640), (719, 1277, 640), (1080, 1920, 640), (1080, 1920, 1280), (90, 120, 640),
          (120, 90, 640), (1, 1, 640), (3000, 17, 320)]
_rng = np.random.default_rng(7)
SHAPES += [(int(_rng.integers(1, 2200)), int(_rng.integers(1, 2200)), int(_rng.choice([320, 416, 640, 960, 1280]))) for _ in range(22)]


def _scale_masks_crop(mh, mw, H0, W0):
    gain = min(mh / H0, mw / W0)
    pad_w, pad_h = (mw - W0 * gain) / 2, (mh - H0 * gain) / 2
    return int(pad_h), int(mh - pad_h), int(pad_w), int(mw - pad_w)


_engines = {}


def _engine(vti_amd, H, W):
    if (H, W) not in _engines:
        _engines[(H, W)] = vti_amd.Engine("n", 2, H=H, W=W, max_batch=1)
    return _engines[(H, W)]


@pytest.mark.parametrize("H0,W0,imgsz", SHAPES)
def test_native_layout_matches_scale_masks(lib_built, H0, W0, imgsz):
    vti_amd = lib_built
    H, W = vti_amd.letterbox_shape(H0, W0, imgsz)
    eng = _engine(vti_amd, H, W)
    top, bottom, left, right = _scale_masks_crop(H // 4, W // 4, H0, W0)
    for packing, row_bytes in (("bits", 8 * -(-W0 // 64)), ("u8", W0)):
        got = eng.mask_native_layout(H0, W0, packing)
        assert got == dict(top=top, bottom=bottom, left=left, right=right, row_bytes=row_bytes, slot_bytes=H0 * row_bytes), (packing, got)


def test_native_layout_worked_examples(lib_built):
    vti_amd = lib_built
    ref = _engine(vti_amd, 736, 960).mask_native_layout(960, 1280, "bits")          # the reference call
    assert (ref["top"], ref["bottom"], ref["left"], ref["right"]) == (2, 182, 0, 240)
    assert ref["row_bytes"] == 160 and ref["slot_bytes"] == 960 * 160
    odd = _engine(vti_amd, *vti_amd.letterbox_shape(719, 1277, 640)).mask_native_layout(719, 1277, "bits")
    assert (odd["top"], odd["bottom"]) == (2, 93) and odd["row_bytes"] == 160
    small = _engine(vti_amd, 480, 640).mask_native_layout(90, 120, "u8")                # frame smaller than the prototype crop
    assert (small["top"], small["bottom"], small["left"], small["right"], small["slot_bytes"]) == (0, 120, 0, 160, 90 * 120)


def test_native_layout_rejects_bad_arguments(lib_built):
    vti_amd = lib_built
    eng = _engine(vti_amd, 640, 640)
    for H0, W0 in ((0, 640), (640, 0), (-5, 10)):
        with pytest.raises(vti_amd.VtiError) as ei:
            eng.mask_native_layout(H0, W0, "bits")
        assert ei.value.code == -1 and "vti_mask_native_layout" in str(ei.value)
