"""vti_mask_polygons (Results.masks.xy on the device) against the host restatement polygons.masks2segments + scale_coords, bit for
bit: closed-form shapes, seeded random blobs, both strategies, letterbox bits and padded native rows, n_live, the overflow path,
frame-size worst cases with closed-form answers, and YOLO.predict's Masks.xy / .xyn."""
import numpy as np
import pytest
import torch

from gpu_util import frames_u8, need_gpu
from vti_amd.polygons import masks2segments, scale_coords

pytestmark = pytest.mark.gpu


def _engine():
    import vti_amd
    return vti_amd.Engine("n", 2, H=64, W=64, max_batch=1)


def _pack(masks, row_bytes, garbage_seed=None):
    """u8 0/1 [n,H,W] -> LSB-first bits u8 [n,H,row_bytes] on the device; garbage_seed: random bits in every column >= W."""
    n, H, W = masks.shape
    bits = np.zeros((n, H, row_bytes), np.uint8)
    packed = np.packbits(masks.astype(np.uint8), axis=-1, bitorder="little")
    bits[..., :packed.shape[-1]] = packed
    if garbage_seed is not None:
        rng = np.random.default_rng(garbage_seed)
        junk = rng.integers(0, 256, bits.shape, dtype=np.uint8)
        col = np.arange(row_bytes * 8).reshape(row_bytes, 8)
        pad = np.packbits((col >= W).astype(np.uint8).reshape(-1), bitorder="little")      # 1 where a bit is a pad bit
        bits |= junk & pad
    return torch.from_numpy(bits).cuda()


def _host(masks, strategy, H0, W0):
    H, W = masks.shape[1:]
    return [scale_coords((H, W), s, (H0, W0)) for s in masks2segments(masks, strategy)]


def _device(eng, bits, W, H0, W0, strategy, offsets=None):
    pts, off = eng.mask_polygons(bits, W, H0, W0, strategy, offsets=offsets)
    p, o = pts.cpu().numpy(), off.cpu().numpy()
    assert o[0] == 0 and np.all(np.diff(o) >= 0) and o[-1] == len(p)
    return [p[o[i]:o[i + 1]] for i in range(len(o) - 1)]


def _assert_same(got, ref, what=""):
    assert len(got) == len(ref)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g.dtype == np.float32 and g.shape == r.shape and np.array_equal(g, r), (what, i, g[:6], r[:6], g.shape, r.shape)


def _closed_form_masks():
    """The shapes of test_polygons.py on one 20 x 30 canvas each."""
    out = []

    def canvas():
        return np.zeros((20, 30), np.uint8)
    m = canvas(); m[3:8, 4:11] = 1; out.append(m)                                   # rectangle
    m = canvas(); m[2, 3] = 1; out.append(m)                                        # single pixel
    m = canvas(); m[1, 1:5] = 1; out.append(m)                                      # 1-pixel bar
    m = canvas()
    for i in range(4):
        m[1 + i, 1 + i] = 1                                                         # 8-connected diagonal
    out.append(m)
    m = canvas(); m[2:12, 2:12] = 1; m[5:8, 5:8] = 0; m[14:17, 20:28] = 1; out.append(m)   # hole + second blob
    m = canvas(); m[2:10, 2:5] = 1; m[7:10, 2:12] = 1; m[13, 13] = 1; out.append(m)    # L + stray pixel
    out.append(canvas())                                                            # empty
    m = canvas(); m[:] = 1; out.append(m)                                           # every border touched
    return np.stack(out)


def _random_blobs(n, H, W, seed):
    """Seeded masks with holes, islands inside holes, many components, border contact, 1-px lines, diagonal chains, dots."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((n, H, W), np.uint8)
    for k in range(n):
        m = np.zeros((H, W), bool)
        for _ in range(rng.integers(1, 6)):                                         # ellipses, some past the border
            cy, cx = rng.uniform(-4, H + 4), rng.uniform(-4, W + 4)
            ry, rx = rng.uniform(1, H / 2), rng.uniform(1, W / 2)
            e = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2
            if rng.random() < 0.4:                                                  # a ring: a hole, sometimes with an island in it
                m |= (e <= 1) & (e > rng.uniform(0.15, 0.6))
                if rng.random() < 0.5:
                    m |= e < 0.03
            else:
                m |= e <= 1
        kind = k % 5
        if kind == 1:                                                               # speckle: many tiny components
            m ^= rng.random((H, W)) < 0.08
        elif kind == 2:                                                             # 1-px lines and diagonal chains
            m[rng.integers(0, H), :] = True
            m[:, rng.integers(0, W)] = True
            d0 = rng.integers(0, W)
            for i in range(min(H, W)):
                if 0 <= d0 - i < W:
                    m[i, d0 - i] = True
        elif kind == 3:                                                             # isolated dots and a checker patch
            m[rng.integers(0, H, 12), rng.integers(0, W, 12)] = True
            y0, x0 = rng.integers(0, H - 8), rng.integers(0, W - 8)
            m[y0:y0 + 8, x0:x0 + 8] = ((yy[:8, :8] + xx[:8, :8]) % 2 == 0)
        elif kind == 4:
            m &= rng.random((H, W)) < 0.7                                           # eroded blobs: ragged borders, pinholes
        out[k] = m
    out[0] = 0                                                                      # an empty one too
    return out


@pytest.mark.parametrize("strategy", ["largest", "concat"])
def test_closed_form_shapes(strategy):
    need_gpu()
    eng = _engine()
    m = _closed_form_masks()
    n, H, W = m.shape
    for rb, H0, W0 in [(4, H, W), (8, H, W), (4, 27, 41), (5, 33, 30)]:            # identity and letterbox-style maps; odd row pitch
        got = _device(eng, _pack(m, rb), W, H0, W0, strategy)
        _assert_same(got, _host(m, strategy, H0, W0), (strategy, rb, H0, W0))
    if strategy == "largest":                                                       # the closed forms themselves
        got = _device(eng, _pack(m, 4), W, H, W, strategy)
        assert got[0].tolist() == [[4, 3], [4, 7], [10, 7], [10, 3]]
        assert got[5].tolist() == [[2, 2], [2, 9], [11, 9], [11, 7], [5, 7], [4, 6], [4, 2]]
        assert got[6].shape == (0, 2)


@pytest.mark.parametrize("strategy", ["largest", "concat"])
def test_random_blobs_letterbox_bits(strategy):
    """Letterbox-style slots (row_bytes = W/8), mapped to a larger frame as scale_coords does for the reference's 1280 x 960."""
    need_gpu()
    eng = _engine()
    m = _random_blobs(240, 46, 64, seed=7)
    got = _device(eng, _pack(m, 8), 64, 60, 80, strategy)
    _assert_same(got, _host(m, strategy, 60, 80), strategy)
    m2 = _random_blobs(60, 37, 72, seed=8)                                          # odd pitch (9 bytes): byte loads
    _assert_same(_device(eng, _pack(m2, 9), 72, 37, 72, strategy), _host(m2, strategy, 37, 72), strategy)


@pytest.mark.parametrize("strategy", ["largest", "concat"])
def test_native_rows_ignore_garbage_pad_bits(strategy):
    """vti_masks_native rows: W0 = 1000 columns in 8*ceil(1000/64) = 128 bytes; the 24 pad bits hold garbage."""
    need_gpu()
    eng = _engine()
    m = _random_blobs(24, 40, 1000, seed=11)
    m[3, :, 990:] = 1                                                               # foreground up to the last real column
    bits = _pack(m, 128, garbage_seed=5)
    got = _device(eng, bits, 1000, 40, 1000, strategy)
    _assert_same(got, _host(m, strategy, 40, 1000), strategy)


def test_n_live_cut_skips_poisoned_slots():
    need_gpu()
    eng = _engine()
    m = _random_blobs(20, 32, 64, seed=3)
    bits = _pack(m, 8)
    bits[12:] = 0xFF                                                                # dead slots: full of ones, never read
    offsets = torch.tensor([0, 5, 12], dtype=torch.int32, device="cuda")           # offsets[B] = 12 live slots
    for strategy in ("largest", "concat"):
        got = _device(eng, bits, 64, 32, 64, strategy, offsets=offsets)
        _assert_same(got[:12], _host(m[:12], strategy, 32, 64), strategy)
        assert all(g.shape == (0, 2) for g in got[12:])


def test_overflow_recall_and_repeatability():
    """A kept points buffer that is too small: offsets still come back, nothing is written, and the engine's second launch
    fills a larger buffer.  Two runs give identical bytes."""
    need_gpu()
    import vti_amd
    eng = _engine()
    m = _random_blobs(30, 48, 64, seed=21)
    bits = _pack(m, 8)
    ref = _host(m, "concat", 48, 64)
    total = sum(len(r) for r in ref)
    eng._poly_points = torch.full((max(total // 3, 1), 2), -7.0, device="cuda")     # too small on purpose
    small = eng._poly_points
    got = _device(eng, bits, 64, 48, 64, "concat")
    _assert_same(got, ref)
    assert torch.all(small == -7.0)                                                # the overflowing launch wrote no point
    assert eng._poly_points.shape[0] >= total
    # the C call itself: offsets always, points only when they fit
    n = bits.shape[0]
    off = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    pts = torch.full((4, 2), -3.0, device="cuda")
    ws = eng._poly_ws
    import ctypes as C
    rc = vti_amd.lib().vti_mask_polygons(eng._ctx, C.c_void_p(bits.data_ptr()), n, None, 48, 64, 8, 48, 64, 1,
                                         C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(off.data_ptr()),
                                         C.c_void_p(pts.data_ptr()), 4, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    assert int(off[-1]) == total and torch.all(pts == -3.0) and int(ws[:4].view(torch.int32)[0]) == 0
    a = eng.mask_polygons(bits, 64, 48, 64, "concat")
    a = (a[0].clone(), a[1].clone())
    b = eng.mask_polygons(bits, 64, 48, 64, "concat")
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


def test_frame_size_worst_cases_in_closed_form():
    """960 x 1280 native rows: a stride-2 dot grid (every pixel its own component: "largest" is the first dot, "concat" every dot in
    raster order) and an all-ones frame (the four corners)."""
    need_gpu()
    eng = _engine()
    H, W = 960, 1280
    dots = np.zeros((H, W), np.uint8)
    dots[::2, ::2] = 1
    ones = np.ones((H, W), np.uint8)
    bits = _pack(np.stack([dots, ones, dots]), 160)
    lg = _device(eng, bits, W, H, W, "largest")
    assert lg[0].tolist() == [[0, 0]] and lg[2].tolist() == [[0, 0]]
    assert lg[1].tolist() == [[0, 0], [0, H - 1], [W - 1, H - 1], [W - 1, 0]]
    cc = _device(eng, bits, W, H, W, "concat")
    ys, xs = np.mgrid[0:H:2, 0:W:2]
    grid = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)
    assert np.array_equal(cc[0], grid) and np.array_equal(cc[2], grid)
    assert cc[1].tolist() == lg[1].tolist()


def test_checkerboard_and_taller_than_lds_against_the_host():
    """The most runs a frame can hold (a 960 x 1280 checkerboard: 640 runs per row, one 8-connected component) and masks whose
    word image does not fit in LDS (1100 x 1280), against the host."""
    need_gpu()
    eng = _engine()
    H, W = 960, 1280
    yy, xx = np.mgrid[0:H, 0:W]
    cb = ((yy + xx) % 2 == 0).astype(np.uint8)[None]
    for strategy in ("largest", "concat"):
        _assert_same(_device(eng, _pack(cb, 160), W, H, W, strategy), _host(cb, strategy, H, W), strategy)
    tall = np.zeros((2, 1100, 1280), np.uint8)
    tall[0, 10:1090, 20:1270] = 1
    tall[0, 400:700, 300:900] = 0
    tall[0, 500:600, 500:700] = 1                                                   # an island in the hole
    tall[1, 1099, :] = 1
    tall[1, :, 0] = 1
    tall[1, 50:60, 1200:1280] = 1
    for strategy in ("largest", "concat"):
        _assert_same(_device(eng, _pack(tall, 160), 1280, 1100, 1280, strategy), _host(tall, strategy, 1100, 1280), strategy)


@pytest.mark.parametrize("retina,drop", [(False, False), (True, False), (False, True)])
def test_predict_masks_xy_matches_the_host_restatement(retina, drop):
    """YOLO.predict at the reference call (conf .20, iou .25, max_det 200, imgsz 960) on 1280 x 960 frames: Masks.xy is
    polygons.py on masks.data_u8, instance by instance; xyn is xy / (W0, H0) in float32."""
    need_gpu()
    import vti_amd
    from test_gpu_predict import _calibrated_model
    frames = frames_u8(2, 960, 1280, seed=31)
    model = _calibrated_model(vti_amd, 2, "h2", frames[0], 960, 0.20)
    model.drop_empty_masks = drop
    res = model.predict(frames, conf=0.20, iou=0.25, max_det=200, imgsz=960, retina_masks=retina)
    seen = 0
    for r in res:
        if r.masks is None:
            continue
        m = r.masks.data_u8.cpu().numpy()
        H, W = m.shape[1:]
        assert (H, W) == ((960, 1280) if retina else (736, 960))
        ref = [scale_coords((H, W), s, (960, 1280)) for s in masks2segments(m)]
        _assert_same(r.masks.xy, ref, (retina, drop))
        wh = np.float32([1280, 960])
        for xy, xyn in zip(r.masks.xy, r.masks.xyn):
            assert xyn.dtype == np.float32 and np.array_equal(xyn, xy / wh)
        seen += len(m)
    assert seen > 0
