"""Seeded inputs of the JPEG tests: tests/golden/make_jpeg_golden.py wrote Pillow's bytes for exactly these frames, test_jpeg.py and
test_gpu_jpeg.py regenerate them from the seeds."""
import numpy as np

SIZES = [(1, 1), (8, 8), (16, 16), (17, 33), (50, 70), (135, 241)]
CONTENTS = ["noise", "checker", "flat", "ramp", "tiles", "zrl"]
QUALITIES_EVERYWHERE = (95,)
QUALITIES_17x33 = (100, 50, 10, 1)


def frame(content, h, w, seed=0):
    """A uint8 [h,w,3] BGR frame."""
    rng = np.random.Generator(np.random.PCG64([seed, h, w, CONTENTS.index(content)]))
    yy, xx = np.mgrid[:h, :w]
    if content == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if content == "checker":                # 8 x 8 tiles of black and white: neighbouring blocks at the two ends of the DC range
        f = ((((yy >> 3) + (xx >> 3)) & 1) * 255).astype(np.uint8)
        return np.repeat(f[..., None], 3, axis=2)
    if content == "flat":
        return np.broadcast_to(rng.integers(0, 256, 3, dtype=np.uint8), (h, w, 3)).copy()
    if content == "ramp":                   # a smooth ramp per channel with a few saturated single-pixel spikes, and in the top
        # left 8 x 16 a comb of black and white columns (a horizontal frequency of full amplitude: size-10 AC at quality 100)
        f = np.stack([(2 * xx + yy) % 256, (xx + 3 * yy) % 256, (255 - xx - yy) % 256], axis=2).astype(np.uint8)
        for _ in range(1 + h * w // 50):
            f[rng.integers(h), rng.integers(w)] = rng.choice([0, 255], 3)
        f[:8, :16] = ((xx[:8, :16] & 1) * 255)[..., None]
        return f
    if content == "tiles":                  # every 8 x 8 tile of every channel 0 or 255
        t = rng.integers(0, 2, ((h + 7) // 8, (w + 7) // 8, 3), dtype=np.uint8) * 255
        return np.repeat(np.repeat(t, 8, axis=0), 8, axis=1)[:h, :w].copy()
    if content == "zrl":                    # grey 8 x 8 tiles: a DC level plus a lone (7,7)-basis term -> 62 zeros in front of it
        c = np.cos((2 * np.arange(8) + 1) * 7 * np.pi / 16)
        basis = np.outer(c, c)
        lv = rng.integers(60, 196, ((h + 7) // 8, (w + 7) // 8))
        amp = rng.integers(20, 60, lv.shape)
        f = np.repeat(np.repeat(lv, 8, axis=0), 8, axis=1) + np.repeat(np.repeat(amp, 8, axis=0), 8, axis=1) * np.tile(basis, lv.shape)
        return np.repeat(np.clip(np.rint(f[:h, :w]), 0, 255).astype(np.uint8)[..., None], 3, axis=2)
    raise ValueError(content)


def cases():
    """[(content, h, w, quality)] of the golden file, in its order."""
    out = [(c, h, w, q) for (h, w) in SIZES for c in CONTENTS for q in QUALITIES_EVERYWHERE]
    out += [(c, 17, 33, q) for c in CONTENTS for q in QUALITIES_17x33]
    return out


def key(content, h, w, q):
    return f"{content}_{h}x{w}_q{q}"
