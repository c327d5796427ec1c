"""Writes tests/golden/jpeg_pillow.npz: Pillow's (libjpeg-turbo's) JPEG bytes of the seeded frames of tests/jpeg_util.py, saved as
Image.save(format="JPEG", quality=q, subsampling=2, optimize=False).  Needs PIL; run once (python tests/golden/make_jpeg_golden.py),
the tests only read the file."""
import io
import os
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_util as J  # noqa: E402


def pillow_bytes(frame_bgr, q):
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(frame_bgr[..., ::-1])).save(buf, format="JPEG", quality=q, subsampling=2, optimize=False)
    return buf.getvalue()


if __name__ == "__main__":
    out = {J.key(*c): np.frombuffer(pillow_bytes(J.frame(c[0], c[1], c[2]), c[3]), dtype=np.uint8) for c in J.cases()}
    out["pillow_version"] = np.array(PIL.__version__)
    path = os.path.join(HERE, "jpeg_pillow.npz")
    np.savez_compressed(path, **out)
    print(f"{len(out) - 1} files, {sum(v.size for k, v in out.items() if k != 'pillow_version')} bytes -> {path} ({os.path.getsize(path)} bytes)")
