"""vti_encode_jpeg cost: us per Engine.encode_jpeg call (nine launches and one host read of offsets[n]) for n = 1, 8, 64 frames of
1280 x 960, timed with device events after warm-up, next to two yardsticks measured in the same run: a device-to-device copy of the
same frames (the floor: the call must at least read them), and what the encode is for, the device-to-host copy of the raw frames
(what process_frames(annotate=...) reads back) against that of the JPEG bytes (what encode="jpeg" reads back), wall clock.
    python3 tools/jpeg_bench.py [--n 1 8 64] [--quality 95] [--content smooth noise] [--rounds 5] [--size 960 1280] [--mixed]
--size: the frame size of the uniform batch.  --mixed: vti_encode_jpeg_frames instead (ten launches), on a batch of n frames that
cycles the four sizes of the tests (481 x 333, 720 x 960, 960 x 1280, 1080 x 1920; n = 64: 16 frames each) in one flat buffer with
its frame table.  What it replaces is one uniform call per size (--size h w --n 16).
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


MIXED_SIZES = [(481, 333), (720, 960), (960, 1280), (1080, 1920)]       # tests/test_gpu_annotate_frames.py


def mixed(a, eng):
    for content in a.content:
        for n in a.n:
            shapes = [MIXED_SIZES[k % 4] for k in range(n)]
            table, offs, total_in = eng.pack_frames(shapes, "cuda")
            flat = np.zeros(total_in, np.uint8)
            per_size = {hw: make_frames(content, -(-n // 4), *hw) for hw in set(shapes)}
            for k, ((h, w), at) in enumerate(zip(shapes, offs)):
                flat[at:at + 3 * h * w] = per_size[(h, w)][k // 4].reshape(-1)
            frames = torch.from_numpy(flat).cuda()
            floor = torch.empty_like(frames)
            enc = lambda: eng.encode_jpeg(frames, quality=a.quality, table=table)
            cpy = lambda: floor.copy_(frames)
            for _ in range(3):
                out, off = enc()
                cpy()
            total, px = int(off[n]), sum(h * w for h, w in shapes)
            scratch = vti_amd.lib().vti_encode_jpeg_frames_scratch_bytes(eng._ctx, table.host.data_ptr())
            print(f"mixed {content} n {n:3d} q {a.quality}: {total} JPEG bytes = {total / px:.3f} B/px ({3 * px / total:.1f}x below the raw "
                  f"{3 * px} bytes), scratch {scratch / 1e6:.1f} MB")
            for run in range(2):
                te, tc = [], []
                for _ in range(a.rounds):
                    te.append(group_ms(enc))
                    tc.append(group_ms(cpy))
                me, mc = float(np.median(te)) * 1e3, float(np.median(tc)) * 1e3
                print(f"  run {run}: encode_frames {me:9.1f} us/call (min {min(te) * 1e3:.1f}), {me / n:8.1f} us/frame, d2d copy {mc:8.1f} us, "
                      f"ratio {me / mc:6.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--quality", type=int, default=95)
    ap.add_argument("--content", nargs="+", default=["smooth", "noise"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--size", type=int, nargs=2, default=[960, 1280], metavar=("H0", "W0"))
    ap.add_argument("--mixed", action="store_true")
    a = ap.parse_args()
    h, w = a.size
    eng = vti_amd.Engine("n", 2, H=64, W=64, max_batch=1)        # the encoder needs a context, not a model
    if a.mixed:
        return mixed(a, eng)
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
