"""vti_encode_jpeg cost: us per Engine.encode_jpeg call (nine launches and one host read of offsets[n]) for n = 1, 8, 64 frames of
1280 x 960, timed with device events after warm-up, next to two yardsticks measured in the same run: a device-to-device copy of the
same frames (the floor: the call must at least read them), and what the encode is for, the device-to-host copy of the raw frames
(what process_frames(annotate=...) reads back) against that of the JPEG bytes (what encode="jpeg" reads back), wall clock.
    python3 tools/jpeg_bench.py [--n 1 8 64] [--quality 95] [--content smooth noise] [--rounds 5]
`smooth` is low-pass noise with a little sensor noise on top (the bytes per pixel of a camera frame, roughly); `noise` is the worst
case for the entropy stages.  (encode, copy) are interleaved in groups of 10 calls, `--rounds` groups each, and the whole
measurement runs twice."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

import vti_amd


def group_ms(fn, calls=10):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / calls


def wall_ms(fn, calls=5):
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts))


def make_frames(content, n, h, w):
    rng = np.random.Generator(np.random.PCG64(3))
    if content == "noise":
        return rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    low = rng.integers(0, 256, (n, h // 16 + 2, w // 16 + 2, 3)).astype(np.float32)
    t = torch.nn.functional.interpolate(torch.from_numpy(low).permute(0, 3, 1, 2), size=(h, w), mode="bilinear", align_corners=False)
    f = t.permute(0, 2, 3, 1).numpy() + rng.normal(0, 2, (n, h, w, 3)).astype(np.float32)
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--quality", type=int, default=95)
    ap.add_argument("--content", nargs="+", default=["smooth", "noise"])
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    h, w = 960, 1280
    eng = vti_amd.Engine("n", 2, H=64, W=64, max_batch=1)        # the encoder needs a context, not a model
    for content in a.content:
        host = make_frames(content, max(a.n), h, w)
        for n in a.n:
            frames = torch.from_numpy(host[:n]).cuda()
            floor = torch.empty_like(frames)
            enc = lambda: eng.encode_jpeg(frames, quality=a.quality)
            cpy = lambda: floor.copy_(frames)
            for _ in range(3):
                out, off = enc()
                cpy()
            total = int(off[n])
            raw = frames.numel()
            print(f"{content} n {n:3d} q {a.quality}: {total} JPEG bytes = {total / (n * h * w):.3f} B/px ({raw / total:.1f}x below the raw "
                  f"{raw} bytes), scratch {eng.encode_jpeg_scratch_bytes(n, h, w) / 1e6:.1f} MB")
            for run in range(2):
                te, tc = [], []
                for _ in range(a.rounds):
                    te.append(group_ms(enc))
                    tc.append(group_ms(cpy))
                me, mc = float(np.median(te)) * 1e3, float(np.median(tc)) * 1e3
                d2h_raw = wall_ms(lambda: frames.cpu())
                d2h_jpg = wall_ms(lambda: (off.cpu(), out[:total].cpu()))
                print(f"  run {run}: encode {me:9.1f} us/call (min {min(te) * 1e3:.1f}), {me / n:8.1f} us/frame, d2d copy {mc:8.1f} us, "
                      f"ratio {me / mc:6.2f}; device-to-host raw {d2h_raw * 1e3:9.1f} us, JPEG {d2h_jpg * 1e3:8.1f} us; "
                      f"encode + JPEG read {me + d2h_jpg * 1e3:9.1f} us")


if __name__ == "__main__":
    main()
