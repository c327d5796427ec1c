"""Per-tile 1x1 convs with the weight fragments fed to the MFMAs from registers (conv_kernel<..., WREG>; VTI_CONV1_WREG).

Exact-integer method of test_gpu_conv.py: small integer operands make every product and partial sum exactly representable, so the
kernel must equal the CPU convolution BIT FOR BIT.  Every case runs with the switch off (weights staged through LDS) and on (each
wave loads the fragments of its own n-tiles and uses them as loaded); both must equal the reference and each other, and the LDS
image must be smaller with the switch on -- which shows that the register path ran.  The templates are shared by the three storage
types, so a wrong fragment index breaks all of them."""
import numpy as np
import pytest
import torch

from gpu_util import need_gpu, ref_conv

pytestmark = pytest.mark.gpu

SLICES = {"in_coff": 16, "in_ld": 96, "out_coff": 32, "out_ld": 320}
CASES = [
    # c1, c2, H, W, forced (wn, nrep), extras
    (48, 256, 7, 9, (4, 4), {}),        # 63 pixels: one ragged 80-pixel tile; h2: three chunks (two-in-flight tail); fp16: remainder chunk
    (48, 256, 7, 9, (4, 2), {}),
    (16, 256, 8, 20, (4, 4), {}),       # one chunk: fewer than the two register sets
    (16, 256, 8, 20, (4, 2), {}),
    (80, 200, 8, 20, (4, 4), {}),       # five chunks, 12.5 n-tiles: a zero-padded fragment and the Cout tail guard
    (80, 200, 8, 20, (4, 2), {}),
    (64, 256, 8, 20, (4, 2), SLICES),   # grid.y = 2, channel slices on both sides
]


def _to_dev(a, dtype):
    import vti_amd
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype == "h2":
        return vti_amd.h2_encode(t).cuda()
    return t.to(torch.float16 if dtype == "fp16" else torch.float32).cuda()


def _to_host(t, dtype):
    import vti_amd
    return vti_amd.h2_decode(t.cpu()) if dtype == "h2" else t.float().cpu()


@pytest.mark.parametrize("dtype", ["fp16", "fp32", "h2"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}to{c[1]}_{c[2]}x{c[3]}_wn{c[4][0]}n{c[4][1]}{'_slices' if c[5] else ''}")
def test_conv1x1_per_tile_wreg(case, dtype, monkeypatch):
    need_gpu()
    import vti_amd
    c1, c2, H, W, (wn, nrep), ex = case
    monkeypatch.setenv("VTI_NO_PK1", "1")       # the per-tile kernel, not conv1_pk
    rng = np.random.default_rng(c1 * 100003 + c2 * 101 + H * 7 + nrep)
    B = 2
    in_ld, in_coff = ex.get("in_ld", c1), ex.get("in_coff", 0)
    oc = ex.get("out_coff", 0)
    x_full = rng.integers(-2, 3, (B, H, W, in_ld)).astype(np.float32)
    x = x_full[..., in_coff:in_coff + c1]
    w = rng.integers(-1, 2, (c2, c1, 1, 1)).astype(np.float32)
    b = rng.integers(-3, 4, (c2,)).astype(np.float32)
    xd = _to_dev(x_full, dtype)
    ref = ref_conv(x, w, b, 1, 1, 1, dtype, act=False)
    got, cfg = {}, {}
    for arm in ("0", "1"):
        monkeypatch.setenv("VTI_CONV1_WREG", arm)
        out, _, cfg[arm] = vti_amd.debug_conv2d(xd, w, b, 1, 1, 1, dtype, in_coff=in_coff, c1=c1, out_coff=oc,
                                                out_ld=ex.get("out_ld"), waves_n=wn, nrep=nrep)
        torch.cuda.synchronize()
        got[arm] = _to_host(out, dtype)
        assert not cfg[arm]["pk"] and cfg[arm]["waves_n"] == wn and cfg[arm]["nrep"] == nrep, cfg[arm]
        assert torch.equal(got[arm][..., oc:oc + c2], ref), f"VTI_CONV1_WREG={arm} cfg={cfg[arm]} max|d|={(got[arm][..., oc:oc + c2] - ref).abs().max()}"
        if oc:      # neighbours of the written channel slice stay untouched
            assert (got[arm][..., :oc] == 0).all() and (got[arm][..., oc + c2:] == 0).all()
    assert torch.equal(got["0"], got["1"])
    assert cfg["1"]["tile"] == cfg["0"]["tile"]
    assert cfg["1"]["lds"] == cfg["0"]["lds"] - wn * nrep * 1024, (cfg["0"], cfg["1"])      # no weight image: the register path ran


def split_exact_case(c1, c2, H, W, ex, seed):
    """h2 only: the case's operands with nonzero lo halves in both operands, asserted split-exact on the host (test_gpu_conv.py)."""
    import h2_ref
    return h2_ref.split_case(seed, (2, H, W, ex.get("in_ld", c1)), ex.get("in_coff", 0), c1, (c2, c1, 1, 1), 1, 1, 1)


def _split_arms(monkeypatch, c1, c2, H, W, wn, nrep, ex, seed, tile, pk):
    """Both VTI_CONV1_WREG arms on the split-exact operands: the stored dwords equal the scheme's, bit for bit."""
    import h2_ref
    import vti_amd
    x_full, _, w, b, _, want = split_exact_case(c1, c2, H, W, ex, seed)
    ref = torch.from_numpy(h2_ref.bits(*h2_ref.enc_act(want)))
    oc = ex.get("out_coff", 0)
    xd = _to_dev(x_full, "h2")
    cfg = {}
    for arm in ("0", "1"):
        monkeypatch.setenv("VTI_CONV1_WREG", arm)
        out, _, cfg[arm] = vti_amd.debug_conv2d(xd, w, b, 1, 1, 1, "h2", in_coff=ex.get("in_coff", 0), c1=c1, out_coff=oc,
                                                out_ld=ex.get("out_ld"), tile=tile, waves_n=wn, nrep=nrep)
        torch.cuda.synchronize()
        got = out.cpu().view(torch.int32)
        assert bool(cfg[arm]["pk"]) == pk and cfg[arm]["waves_n"] == wn and cfg[arm]["nrep"] == nrep, cfg[arm]
        assert torch.equal(got[..., oc:oc + c2], ref), f"VTI_CONV1_WREG={arm} cfg={cfg[arm]} differing outputs: {(got[..., oc:oc + c2] != ref).float().mean():.3f}"
        if oc:
            assert (got[..., :oc] == 0).all() and (got[..., oc + c2:] == 0).all()
    return cfg


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}to{c[1]}_{c[2]}x{c[3]}_wn{c[4][0]}n{c[4][1]}{'_slices' if c[5] else ''}")
def test_conv1x1_per_tile_wreg_split_exact_h2(case, monkeypatch):
    """The cases above with nonzero lo halves (h2): the lo operands of the LDS-staged and of the register-fed weight fragments."""
    need_gpu()
    c1, c2, H, W, (wn, nrep), ex = case
    monkeypatch.setenv("VTI_NO_PK1", "1")
    cfg = _split_arms(monkeypatch, c1, c2, H, W, wn, nrep, ex, c1 * 100003 + c2 * 101 + H * 7 + nrep + 1, (0, 0), False)
    assert cfg["1"]["lds"] == cfg["0"]["lds"] - wn * nrep * 1024, cfg


# ---- conv1_pk with the n-group's weights in the compute waves' registers (pk_wstat == 2)
# (nrep, wn, K chunks) with a register-resident instantiation (conv_pk.hip: Conv1PkWH2 / Conv1PkWF16; none for fp32): the
# instantiations that compile without spills.  Every other case must run today's kernel, with an unchanged LDS image.
PK_WREG = {"h2": {(2, w, n) for w in (2, 4) for n in (4, 6, 8, 12, 16)},
           "fp16": {(2, w, n) for w in (2, 4) for n in (2, 3, 4, 6, 8)} | {(4, 1, 2)},
           "fp32": set()}
PK_CASES = [
    # c1, c2, H, W, forced (wn, nrep), VTI_PK_MAX_WGS, extras
    (96, 128, 9, 20, (4, 2), 3, {}),        # 360 pixels = 4.5 tiles: tile chains, ragged last tile, no XCD ranges
    (96, 128, 9, 20, (4, 2), 8, {}),
    (64, 64, 9, 20, (1, 4), 0, {}),
    (80, 64, 9, 20, (1, 4), 0, {}),         # five h2 chunks: no instantiation, and the dummy second chunk of the last step
    (112, 128, 9, 20, (4, 2), 0, {}),       # seven 16-channel chunks: no instantiation, must fall back (fp16: 3.5 chunks of 32, engages)
    (128, 128, 4, 20, (4, 2), 0, {}),       # h2: eight chunks, the most that keep the prepared operands
    (192, 128, 4, 20, (4, 2), 0, {}),       # h2: twelve chunks of raw fragments, prepared in the loop
    (256, 128, 4, 20, (4, 2), 0, {}),       # the largest register budget: h2 sixteen chunks (raw), fp16 eight
    (64, 128, 9, 20, (4, 2), 3, SLICES),
]


@pytest.mark.parametrize("dtype", ["fp16", "fp32", "h2"])
@pytest.mark.parametrize("case", PK_CASES, ids=lambda c: f"{c[0]}to{c[1]}_{c[2]}x{c[3]}_wn{c[4][0]}n{c[4][1]}_wgs{c[5]}{'_slices' if c[6] else ''}")
def test_conv1_pk_wreg(case, dtype, monkeypatch):
    need_gpu()
    import vti_amd
    c1, c2, H, W, (wn, nrep), wgs, ex = case
    monkeypatch.delenv("VTI_NO_PK1", raising=False)
    if wgs:
        monkeypatch.setenv("VTI_PK_MAX_WGS", str(wgs))
    rng = np.random.default_rng(c1 * 100003 + c2 * 101 + H * 7 + wgs)
    B = 2
    in_ld, in_coff = ex.get("in_ld", c1), ex.get("in_coff", 0)
    oc = ex.get("out_coff", 0)
    x_full = rng.integers(-2, 3, (B, H, W, in_ld)).astype(np.float32)
    x = x_full[..., in_coff:in_coff + c1]
    w = rng.integers(-1, 2, (c2, c1, 1, 1)).astype(np.float32)
    b = rng.integers(-3, 4, (c2,)).astype(np.float32)
    xd = _to_dev(x_full, dtype)
    ref = ref_conv(x, w, b, 1, 1, 1, dtype, act=False)
    engages = (nrep, wn, -(-c1 // (32 if dtype == "fp16" else 16))) in PK_WREG[dtype]
    got, cfg = {}, {}
    for arm in ("0", "1"):
        monkeypatch.setenv("VTI_CONV1_WREG", arm)
        out, _, cfg[arm] = vti_amd.debug_conv2d(xd, w, b, 1, 1, 1, dtype, in_coff=in_coff, c1=c1, out_coff=oc,
                                                out_ld=ex.get("out_ld"), tile=(1, 80), waves_n=wn, nrep=nrep)
        torch.cuda.synchronize()
        got[arm] = _to_host(out, dtype)
        assert cfg[arm]["pk"] and cfg[arm]["waves_n"] == wn and cfg[arm]["nrep"] == nrep, cfg[arm]
        assert torch.equal(got[arm][..., oc:oc + c2], ref), f"VTI_CONV1_WREG={arm} cfg={cfg[arm]} max|d|={(got[arm][..., oc:oc + c2] - ref).abs().max()}"
        if oc:
            assert (got[arm][..., :oc] == 0).all() and (got[arm][..., oc + c2:] == 0).all()
    assert torch.equal(got["0"], got["1"])
    if engages:
        assert cfg["1"]["lds"] < cfg["0"]["lds"], (cfg["0"], cfg["1"])      # no weight image in LDS: the register path ran
    else:
        assert cfg["1"]["lds"] == cfg["0"]["lds"], (cfg["0"], cfg["1"])     # no instantiation for this chunk count: today's kernel


@pytest.mark.parametrize("case", PK_CASES, ids=lambda c: f"{c[0]}to{c[1]}_{c[2]}x{c[3]}_wn{c[4][0]}n{c[4][1]}_wgs{c[5]}{'_slices' if c[6] else ''}")
def test_conv1_pk_wreg_split_exact_h2(case, monkeypatch):
    """The persistent 1x1's cases with nonzero lo halves (h2): prepared and raw register-resident fragments, and the LDS image."""
    need_gpu()
    c1, c2, H, W, (wn, nrep), wgs, ex = case
    monkeypatch.delenv("VTI_NO_PK1", raising=False)
    if wgs:
        monkeypatch.setenv("VTI_PK_MAX_WGS", str(wgs))
    cfg = _split_arms(monkeypatch, c1, c2, H, W, wn, nrep, ex, c1 * 100003 + c2 * 101 + H * 7 + wgs + 1, (1, 80), True)
    engages = (nrep, wn, -(-c1 // 16)) in PK_WREG["h2"]
    assert (cfg["1"]["lds"] < cfg["0"]["lds"]) if engages else (cfg["1"]["lds"] == cfg["0"]["lds"]), cfg
