"""vti_decode_jpeg cost: us per Engine.decode_jpeg call (one pinned staging copy, one H2D of table + files, five launches) for n = 1,
8, 64 files of 1280 x 960, timed with device events after warm-up, with the rounds the entropy stage used (info), next to what the
call replaces: the same files decoded by Pillow (libjpeg-turbo) in a 16-thread pool, where PIL is installed; and the wall clock of
the H2D copy of the files against that of the raw frames.
    python3 tools/jpeg_decode_bench.py [--n 1 8 64] [--quality 95] [--content smooth noise] [--sampling 420 422] [--segment 0] [--rounds 5]
`smooth` is low-pass noise with a little sensor noise on top (the bytes per pixel of a camera frame, roughly); `noise` is the worst
case for the entropy stage (no EOB symbols to resynchronise on).  The files are written with Pillow when it is there, with the
package's own encoder (4:2:0 only) otherwise.  The whole measurement runs twice.
Kernel split: rocprofv3 --kernel-trace --stats -- python3 tools/jpeg_decode_bench.py --n 8 --rounds 2"""
import argparse
import io
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

import vti_amd
from jpeg_bench import group_ms, make_frames, wall_ms

try:
    from PIL import Image
except ImportError:
    Image = None

SUBSAMPLING = {"444": 0, "422": 1, "420": 2}


def make_files(frames_bgr, quality, sampling, eng):
    if Image is not None:
        out = []
        for f in frames_bgr:
            buf = io.BytesIO()
            Image.fromarray(np.ascontiguousarray(f[..., ::-1])).save(buf, format="JPEG", quality=quality, subsampling=SUBSAMPLING[sampling])
            out.append(buf.getvalue())
        return out
    if sampling != "420":
        return None
    data, off = eng.encode_jpeg(torch.from_numpy(frames_bgr).cuda(), quality=quality)
    off = off.cpu().numpy()
    host = data[:off[-1]].cpu().numpy().tobytes()
    return [host[off[k]:off[k + 1]] for k in range(len(frames_bgr))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--quality", type=int, default=95)
    ap.add_argument("--content", nargs="+", default=["smooth", "noise"])
    ap.add_argument("--sampling", nargs="+", default=["420", "422"])
    ap.add_argument("--segment", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    h, w = 960, 1280
    eng = vti_amd.Engine("n", 2, H=64, W=64, max_batch=1)        # the decoder needs a context, not a model
    pool = ThreadPoolExecutor(16)
    for content in a.content:
        host = make_frames(content, max(a.n), h, w)
        for sampling in a.sampling:
            files_all = make_files(host, a.quality, sampling, eng)
            if files_all is None:
                print(f"{content} {sampling}: no PIL here, and the package's encoder writes 4:2:0 only -- skipped")
                continue
            for n in a.n:
                files = files_all[:n]
                nbytes, raw = sum(len(f) for f in files), n * h * w * 3
                dec = lambda: eng.decode_jpeg(files, rgb=False, segment_bytes=a.segment)
                for _ in range(2):
                    frames, info = dec()
                info = info.cpu().numpy()
                assert not info[:, 0].any(), info
                print(f"{content} {sampling} n {n:3d} q {a.quality}: {nbytes} file bytes = {nbytes / (n * h * w):.3f} B/px ({raw / nbytes:.1f}x below "
                      f"the raw {raw}); segments/file {int(info[:, 1].mean())}, rounds min {info[:, 2].min()} median "
                      f"{int(np.median(info[:, 2]))} max {info[:, 2].max()}")
                pinned_files = torch.frombuffer(bytearray(b"".join(files)), dtype=torch.uint8).pin_memory()
                pinned_raw = torch.empty(raw, dtype=torch.uint8).pin_memory()
                d_files, d_raw = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(raw, dtype=torch.uint8, device="cuda")
                for run in range(2):
                    td = [group_ms(dec, a.calls) for _ in range(a.rounds)]
                    line = (f"  run {run}: decode {np.median(td) * 1e3:9.1f} us/call (min {min(td) * 1e3:.1f}, max {max(td) * 1e3:.1f}) = "
                            f"{np.median(td) * 1e3 / n:8.1f} us/file")
                    if Image is not None:
                        one = lambda b: np.asarray(Image.open(io.BytesIO(b)))
                        ts = []
                        for _ in range(3):
                            t = time.perf_counter()
                            list(pool.map(one, files))
                            ts.append((time.perf_counter() - t) * 1e3)
                        line += f"; Pillow, 16 threads {np.median(ts) * 1e3:9.1f} us/batch"
                    h2d_f = wall_ms(lambda: d_files.copy_(pinned_files, non_blocking=True))
                    h2d_r = wall_ms(lambda: d_raw.copy_(pinned_raw, non_blocking=True))
                    print(line + f"; H2D files {h2d_f * 1e3:.1f} us, raw frames {h2d_r * 1e3:.1f} us (wall)")


if __name__ == "__main__":
    main()
