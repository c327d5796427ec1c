"""Writes tests/golden/jpeg_decode_pillow.npz: Pillow's (libjpeg-turbo's) JPEG files of the seeded frames of tests/jpeg_util.py in
the cases of tests/jpeg_decode_util.golden_cases() -- 4:2:0 / 4:2:2 / 4:4:4, qualities 95, 100, 50, 10 and 1, optimised Huffman
tables, restart markers, a file with its DHT segments removed -- and the pixels np.asarray(Image.open(file)) gives for each.  Needs
PIL; run once (python tests/golden/make_jpeg_decode_golden.py), the tests only read the file."""
import io
import os
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_decode_util as U  # noqa: E402
import jpeg_util as J  # noqa: E402


def pillow_file(frame_bgr, q, sampling, **opts):
    strip = opts.pop("strip_dht", False)
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(frame_bgr[..., ::-1])).save(buf, format="JPEG", quality=q, subsampling=U.PIL_SUBSAMPLING[sampling], **opts)
    return U.strip_dht(buf.getvalue()) if strip else buf.getvalue()


def pillow_pixels(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


if __name__ == "__main__":
    out = {}
    for key, content, h, w, ss, q, opts in U.golden_cases():
        data = pillow_file(J.frame(content, h, w), q, ss, **dict(opts))
        out["file_" + key] = np.frombuffer(data, np.uint8)
        out["rgb_" + key] = pillow_pixels(data)
    out["pillow_version"] = np.array(PIL.__version__)
    path = os.path.join(HERE, "jpeg_decode_pillow.npz")
    np.savez_compressed(path, **out)
    print(f"{len(U.golden_cases())} files -> {path} ({os.path.getsize(path)} bytes)")
