#!/usr/bin/env python3
"""Work balance of the post-processing stage, from one `bench.py --dump-outputs DIR` (host only: numpy, no GPU).

    python tools/post_balance.py DIR [--H 640 --W 640] [--capacity N] [--c C] [--groups 4]

Reads DIR/dets.npy [B, max_det, 6+nm] and DIR/counts.npy [B] and prints
  per frame   (a) the (instance, 64x64 tile) pairs of masks_group_kernel, by the rectangle rule of mask_tile_rect (post.hip),
              (b) the kept count,
  per XCD     (c) the pair sum of the (frame, tile) items it owns under the equal-item-count partition,
              (d) the pair sum under the partition by cumulative weight of masks_group_kernel: an item of frame b weighs n_b + C,
                  n_b the frame's instances that own a slot, C = MASK_ITEM_C of post.hip,
  max/mean of (c) and (d), both also under the cost model "an item costs ALPHA pairs plus its pairs" (--alpha), the crowded frame's
  kept count per class group (class % G) and the largest group over all frames.
Only kept rows are in a dump: candidate counts come from tools/nms_stats.py."""
import argparse
import os

import numpy as np

MT = 64


def tile_rect(d, H, W):
    """mask_tile_rect: the tiles [tx0, tx1] x [ty0, ty1] an instance's crop box (+ 8 px) can reach, or None."""
    tiles_x, tiles_y = (W + MT - 1) // MT, (H + MT - 1) // MT
    f = np.float32
    x1, y1, x2, y2 = f(d[0]) - f(8), f(d[1]) - f(8), f(d[2]) + f(8), f(d[3]) + f(8)
    tx0, tx1 = int(np.floor(x1 / f(MT))), int(np.floor(x2 / f(MT)))
    ty0, ty1 = int(np.floor(y1 / f(MT))), int(np.floor(y2 / f(MT)))
    tx0, ty0, tx1, ty1 = max(tx0, 0), max(ty0, 0), min(tx1, tiles_x - 1), min(ty1, tiles_y - 1)
    return (tx0, tx1, ty0, ty1) if tx1 >= tx0 and ty1 >= ty0 else None


def item_pairs(dets, n_own, H, W):
    """[B, tiles] instances listed by each (frame, tile) item; n_own[b] = instances of frame b that own a slot."""
    tiles_x, tiles_y = (W + MT - 1) // MT, (H + MT - 1) // MT
    out = np.zeros((dets.shape[0], tiles_y, tiles_x), np.int64)
    for b in range(dets.shape[0]):
        for i in range(int(n_own[b])):
            r = tile_rect(dets[b, i], H, W)
            if r:
                out[b, r[2]:r[3] + 1, r[0]:r[1] + 1] += 1
    return out.reshape(dets.shape[0], -1)


def bounds_equal(n_items, x):
    per = (n_items + 7) >> 3
    return np.minimum(n_items, np.arange(x + 1) * per)


def bound_closed_form(off, tiles, c, k, xcds=8):
    """mask_weight_bound of post.hip, statement for statement: the start of XCD k's range from the prefix sums `off` [B + 1] alone."""
    B = len(off) - 1
    n = B * tiles
    if k <= 0:
        return 0
    if k >= xcds:
        return n
    wt = tiles * (int(off[B]) + c * B)
    thr = (wt * k + xcds - 1) // xcds
    lo, hi = 0, B
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if tiles * (int(off[mid]) + c * mid) < thr:
            lo = mid
        else:
            hi = mid
    w_b = int(off[lo + 1]) - int(off[lo]) + c
    rest = thr - tiles * (int(off[lo]) + c * lo)
    cnt = tiles if w_b <= 0 else min(tiles, (rest + w_b - 1) // w_b)
    return lo * tiles + cnt


def bounds_weighted(weight, x):
    """Items whose exclusive cumulative weight falls in [k W/x, (k+1) W/x) go to XCD k: start(k) = #items with x * cum < k * W."""
    cum = np.concatenate([[0], np.cumsum(weight)])[:-1]
    total = int(weight.sum())
    bnd = [int(np.count_nonzero(x * cum < k * total)) for k in range(x)]
    return np.array(bnd + [len(weight)])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("dir")
    ap.add_argument("--H", type=int, default=640)
    ap.add_argument("--W", type=int, default=640)
    ap.add_argument("--capacity", type=int, default=None, help="mask slots (default: every kept instance owns one)")
    ap.add_argument("--c", type=int, default=32, help="per-item constant added to the weight n_b (MASK_ITEM_C of post.hip)")
    ap.add_argument("--alpha", type=float, default=12.0, help="cost model of the last line: an item of a frame with instances costs ALPHA + its pairs")
    ap.add_argument("--groups", type=int, default=4, help="class groups of the NMS (class %% G)")
    ap.add_argument("--xcds", type=int, default=8)
    a = ap.parse_args()
    dets = np.load(os.path.join(a.dir, "dets.npy"))
    counts = np.load(os.path.join(a.dir, "counts.npy")).astype(np.int64)
    B, max_det = dets.shape[:2]
    off = np.concatenate([[0], np.cumsum(np.clip(counts, 0, max_det))])
    if a.capacity is not None:
        off = np.minimum(off, a.capacity)
    n_own = off[1:] - off[:-1]
    pairs = item_pairs(dets, n_own, a.H, a.W)
    tiles = pairs.shape[1]
    print(f"B {B}  tiles/frame {tiles}  instances {int(n_own.sum())}  pairs {int(pairs.sum())}  weight n_b + {a.c}")
    print("frame  (a) pairs  (b) kept")
    for b in range(B):
        print(f"{b:5d} {int(pairs[b].sum()):10d} {int(counts[b]):9d}")
    flat = pairs.reshape(-1)
    weight = np.repeat(n_own + a.c, tiles)
    print("XCD   (c) pairs, equal item counts   (d) pairs, by weight    items (c)  items (d)")
    sums = []
    bc, bd = bounds_equal(len(flat), a.xcds), bounds_weighted(weight, a.xcds)
    assert bd.tolist() == [bound_closed_form(off, tiles, a.c, k, a.xcds) for k in range(a.xcds + 1)]
    for x in range(a.xcds):
        c, d = int(flat[bc[x]:bc[x + 1]].sum()), int(flat[bd[x]:bd[x + 1]].sum())
        sums.append((c, d))
        print(f"{x:3d} {c:18d} {d:28d} {int(bc[x + 1] - bc[x]):16d} {int(bd[x + 1] - bd[x]):10d}")
    s = np.array(sums, np.float64)
    mean = max(s[:, 0].mean(), 1e-9)
    print(f"max/mean (c) {s[:, 0].max() / mean:.3f}   max/mean (d) {s[:, 1].max() / mean:.3f}")
    cost = np.where(np.repeat(n_own, tiles) > 0, a.alpha + flat, 0.0)
    cc = np.array([[cost[bc[x]:bc[x + 1]].sum(), cost[bd[x]:bd[x + 1]].sum()] for x in range(a.xcds)])
    print(f"cost = {a.alpha:g} + pairs per item: max/mean (c) {cc[:, 0].max() / cc[:, 0].mean():.3f}   (d) {cc[:, 1].max() / cc[:, 1].mean():.3f}")
    crowded = int(np.argmax(counts))
    cls = dets[..., 5].astype(np.int64)
    grp = np.array([[int(np.count_nonzero(cls[b, :counts[b]] % a.groups == g)) for g in range(a.groups)] for b in range(B)])
    print(f"crowded frame {crowded}: kept {int(counts[crowded])}, kept per class group (class % {a.groups}) {grp[crowded].tolist()}")
    print(f"kept per frame: median {int(np.median(counts))}  max {int(counts.max())};  largest kept class group over all frames "
          f"{int(grp.max())} (frame {int(np.argmax(grp.max(1)))})")


if __name__ == "__main__":
    main()
