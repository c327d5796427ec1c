"""-m gpu: masks_group_kernel cuts its (frame, tile) list among the XCDs by cumulative weight, not by item count, so a boundary can
fall inside a frame and an XCD's range can be empty.  The masks must stay what they were: both packings against process_mask, as
test_gpu_postproc.test_masks_crowded_tiles_rounds_and_ragged_width compares them; and since an item computes the same bits whichever
workgroup runs it, a batch must equal its frames run one at a time, byte for byte."""
import numpy as np
import pytest
import torch

from gpu_util import mask_iou, need_gpu
from oracle.postproc import process_mask

pytestmark = pytest.mark.gpu

NM = 32
_ENGINES = {}


def _engine(nc, H, W, B=4, dtype="fp16"):
    key = (nc, H, W, B, dtype)
    if key not in _ENGINES:
        import vti_amd
        eng = vti_amd.Engine("n", nc, H=H, W=W, max_batch=B, dtype=dtype)
        eng.load_weights(vti_amd.random_weights(eng, seed=1), 0)
        _ENGINES[key] = eng
    return _ENGINES[key]


COUNTS = (120, 0, 3, 0, 0, 1, 0, 64, 2)
MAX_DET = 128


def _mask_case(H, W, dtype):
    rng = np.random.default_rng(61)
    B = len(COUNTS)
    dets = np.zeros((B, MAX_DET, 6 + NM), np.float32)
    for b in range(B):
        for i in range(COUNTS[b]):
            w, h = rng.uniform(0.2, 0.8) * W, rng.uniform(0.2, 0.8) * H
            x1, y1 = rng.uniform(0, W - w), rng.uniform(0, H - h)
            dets[b, i, :4] = [x1, y1, x1 + w, y1 + h]
            dets[b, i, 4], dets[b, i, 5] = 0.9 - 0.001 * i, i % 2
            dets[b, i, 6:] = rng.standard_normal(NM)
    tdt = torch.float16 if dtype == "fp16" else torch.float32
    proto = torch.from_numpy(rng.standard_normal((B, H // 4, W // 4, NM)).astype(np.float32)).to(tdt).cuda()
    return dets, proto


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
@pytest.mark.parametrize("H,W", [(224, 288), (640, 640)])
def test_masks_partition_by_weight(dtype, H, W):
    """B = 9 with counts (120, 0, 3, 0, 0, 1, 0, 64, 2): XCD boundaries fall inside frames 0 and 7 and whole XCDs get ranges without
    an instance.  Both packings against process_mask; then the batch must equal B = 1 calls frame by frame, byte for byte, a call whose
    counts are all zero writes nothing, and a capacity below the total drops the slots beyond it and nothing else."""
    need_gpu()
    import vti_amd
    B = len(COUNTS)
    eng = _engine(2, H, W, B=B, dtype=dtype)
    dets, proto = _mask_case(H, W, dtype)
    dd, cc = torch.from_numpy(dets).cuda(), torch.tensor(COUNTS, dtype=torch.int32).cuda()
    total = sum(COUNTS)
    masks, off = eng.masks(dd, cc, proto, "logit", "u8")
    bits, off2 = eng.masks(dd, cc, proto, "logit", "bits")
    torch.cuda.synchronize()
    assert off.cpu().tolist() == np.concatenate(([0], np.cumsum(COUNTS))).tolist() and torch.equal(off, off2)
    assert masks.shape[0] == total and bits.shape[0] == total
    # Each packing against process_mask.  (The two packings are not compared with each other here: the byte path blends columns
    # first, the bit path rows first, and a logit within an ulp of 0 can fall on either side -- 2 of the 78 M pixels of the fp32
    # 640 x 640 case differ, with the equal-count partition as well.)
    refs = {}
    for b in range(B):
        if COUNTS[b]:
            d = dets[b, :COUNTS[b]]
            refs[b] = process_mask(proto[b].float().cpu().permute(2, 0, 1), d[:, 6:], d[:, :4], (H, W), "logit").numpy()
    for packing, whole in (("u8", masks), ("bits", vti_amd.unpack_bits(bits, W))):
        worst = 1.0
        for b, ref in refs.items():
            got = whole[int(off[b]):int(off[b + 1])].cpu().numpy()
            for i in range(COUNTS[b]):
                if ref[i].sum() == 0:
                    assert got[i].sum() == 0, (packing, b, i)
                else:
                    worst = min(worst, mask_iou(got[i], ref[i]))
        print(packing, "worst IoU", worst)
        assert worst >= 0.999, (packing, worst)
    # B = 1: every frame alone gives the bytes it has in the batch
    for b in range(B):
        for packing, whole in (("u8", masks), ("bits", bits)):
            m1, o1 = eng.masks(dd[b:b + 1], cc[b:b + 1], proto[b:b + 1], "logit", packing)
            assert o1.cpu().tolist() == [0, COUNTS[b]] and torch.equal(m1, whole[int(off[b]):int(off[b + 1])]), (b, packing)
    # all counts zero: offsets are zeros and no byte of a given buffer is written
    for packing in ("u8", "bits"):
        buf = torch.full((4, H, W if packing == "u8" else W // 8), 0xAB, dtype=torch.uint8, device="cuda")
        _, o0 = eng.masks(dd, torch.zeros_like(cc), proto, "logit", packing, capacity=4, masks=buf)
        torch.cuda.synchronize()
        assert o0.cpu().tolist() == [0] * (B + 1) and bool((buf == 0xAB).all())
    # capacity below the total (inside frame 0, and inside frame 7): the slots that fit are what they were, the one behind is not touched
    for cap in (100, 150):
        for packing, whole in (("u8", masks), ("bits", bits)):
            buf = torch.full((cap + 1,) + tuple(whole.shape[1:]), 0xAB, dtype=torch.uint8, device="cuda")
            _, oc = eng.masks(dd, cc, proto, "logit", packing, capacity=cap, masks=buf[:cap])
            torch.cuda.synchronize()
            assert torch.equal(oc, off) and torch.equal(buf[:cap], whole[:cap]) and bool((buf[cap] == 0xAB).all()), (cap, packing)
