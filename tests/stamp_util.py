"""Shared by the stamp tests (test_stamp.py, test_stamp_abi.py, test_gpu_stamp.py): a deterministic rasteriser in the place of
cv2.putText, the statement of what text_stamps must reproduce, and a reader of the packed stamp table."""
import struct
import zlib

import numpy as np

FACE = "FONT_HERSHEY_SIMPLEX"


def item(text, org, colour, scale=0.6, thickness=1):
    """One item in annotate.text_items' form."""
    return (text, tuple(org), FACE, scale, tuple(colour), thickness)


def rasterise(canvas, it):
    """Draws a pattern derived from the item, in 200, clipped to the canvas as a drawing call clips: "rect W H" a filled rectangle
    whose top-left corner is org, "frame W H" its outline, "diag N" the pixels org + (i, i), "anti N" the pixels org + (i, -i), "none"
    nothing; any other string (the text of a record) a pattern of a size and kind taken from its CRC, its bottom-left corner at org
    as putText places a string."""
    text, (x, y) = it[0], it[1]
    h, w = canvas.shape
    word = text.split()
    kind = word[0] if word and word[0] in ("rect", "frame", "diag", "anti", "none") else None
    if kind is None:
        crc = zlib.crc32(text.encode())
        bw, bh = 5 + crc % 40, 3 + (crc >> 8) % 12
        kind, word, y = ("rect", "frame", "diag")[(crc >> 16) % 3], [None, bw, bh], y - bh
    if kind == "none":
        return
    if kind in ("diag", "anti"):
        n = int(word[1])
        for i in range(n):
            px, py = x + i, y + (i if kind == "diag" else -i)
            if 0 <= px < w and 0 <= py < h:
                canvas[py, px] = 200
        return
    bw, bh = int(word[1]), int(word[2])
    x0, x1, y0, y1 = max(x, 0), min(x + bw, w), max(y, 0), min(y + bh, h)
    if x0 >= x1 or y0 >= y1:
        return
    if kind == "rect":
        canvas[y0:y1, x0:x1] = 200
        return
    for yy in (y, y + bh - 1):
        if 0 <= yy < h:
            canvas[yy, x0:x1] = 200
    for xx in (x, x + bw - 1):
        if 0 <= xx < w:
            canvas[y0:y1, xx] = 200


def painted(picture, items, rasteriser=rasterise):
    """What stamp(picture, text_stamps(items, h, w, rasteriser)) must equal: every item drawn on a canvas of its own, and the
    picture's pixels under the non-zero ones set to the item's colour, in order.  -> (a copy, the number of items that drew)."""
    out = picture.copy()
    drew = 0
    for it in items:
        canvas = np.zeros(picture.shape[:2], np.uint8)
        rasteriser(canvas, it)
        out[canvas != 0] = it[4]
        drew += int(canvas.any())
    return out, drew


def read_table(host):
    """The packed stamp table (a CPU u8 tensor or bytes) -> (header dict, [(H0, W0, begin, end)], [dict(offset, x, y, w, h, pitch,
    colour)]): a 64-byte header, 16 bytes per picture, 32 bytes per stamp."""
    raw = bytes(host.numpy().tobytes() if hasattr(host, "numpy") else host)
    magic, n_pictures, n_stamps, _, n_words = struct.unpack_from("<iiiiq", raw, 0)
    pics = [struct.unpack_from("<iiii", raw, 64 + 16 * k) for k in range(n_pictures)]
    at = 64 + 16 * n_pictures
    recs = []
    for i in range(n_stamps):
        off, x, y, w, h, pitch, col = struct.unpack_from("<qiiiiiI", raw, at + 32 * i)
        recs.append(dict(offset=off, x=x, y=y, w=w, h=h, pitch=pitch, colour=(col & 255, (col >> 8) & 255, (col >> 16) & 255)))
    assert len(raw) == at + 32 * n_stamps
    return dict(magic=magic, n_pictures=n_pictures, n_stamps=n_stamps, n_words=n_words), pics, recs


def unpacked(rec, words):
    """The bool [h, w] bits of one record of read_table, read from the bit buffer `words` (uint32) by the documented rule."""
    rows = np.asarray(words[rec["offset"]:rec["offset"] + rec["h"] * rec["pitch"]], dtype="<u4").reshape(rec["h"], rec["pitch"])
    return np.unpackbits(rows.view(np.uint8), axis=1, bitorder="little")[:, :rec["w"]].astype(bool)


def random_stamp(rng, x, y, w, h, colour=None, ones=None):
    bits = rng.integers(0, 2, (h, w)).astype(bool) if ones is None else np.full((h, w), bool(ones))
    return (int(x), int(y), bits, tuple(int(v) for v in (rng.integers(0, 256, 3) if colour is None else colour)))
