"""rawframes.to_bgr against OpenCV's cvtColor(COLOR_YUV2BGR_*), where cv2 imports: the pin of the restatement to the library it
restates.  Skipped where OpenCV is not installed (as tests/test_annotate_cv2.py is); the rule itself is pinned by the hand cases
of tests/test_rawframes.py."""
import numpy as np
import pytest

from vti_amd import rawframes as R

cv2 = pytest.importorskip("cv2")

CODES = {"yuyv": "COLOR_YUV2BGR_YUYV", "uyvy": "COLOR_YUV2BGR_UYVY", "nv12": "COLOR_YUV2BGR_NV12", "nv21": "COLOR_YUV2BGR_NV21",
         "i420": "COLOR_YUV2BGR_I420", "yv12": "COLOR_YUV2BGR_YV12"}
RGB_CODES = {k: v.replace("2BGR_", "2RGB_") for k, v in CODES.items()}


@pytest.mark.parametrize("fmt", sorted(CODES, key=R.FORMATS.get))
def test_to_bgr_is_cvtcolor(fmt):
    rng = np.random.Generator(np.random.PCG64(7))
    for H0, W0 in ((2, 2), (6, 10), (18, 34), (64, 130), (240, 320)):
        raw = rng.integers(0, 256, R.frame_bytes(fmt, H0, W0), dtype=np.uint8)
        src = raw.reshape(H0, W0, 2) if R.FORMATS[fmt] < 2 else raw.reshape(H0 * 3 // 2, W0)
        assert np.array_equal(R.to_bgr(raw, fmt, H0, W0)[0], cv2.cvtColor(src, getattr(cv2, CODES[fmt]))), (fmt, H0, W0)
        assert np.array_equal(R.to_bgr(raw, fmt, H0, W0, rgb=True)[0], cv2.cvtColor(src, getattr(cv2, RGB_CODES[fmt]))), (fmt, H0, W0)
