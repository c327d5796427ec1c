#!/usr/bin/env python3
"""Headline benchmark: frames/s of the YOLOv8n-seg hot path (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W
    N > 1 works both ways: under `python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...`
    (RANK / LOCAL_RANK / WORLD_SIZE from the environment), and as the plain command above -- the parent then starts N fresh
    rank processes itself (before it touches a GPU; never exec), relays rank 0's JSON line and returns the worst exit code.
    `--backend gloo --dry` runs the launch + per-step exchange + JSON path on CPU tensors without any kernel (CPU tests).

The headline dtype is h2 (split-fp16 pairs on the fp16 matrix pipe, include/vti.h): the dtype whose detections and masks meet the
north-star tolerance against the fp32 CPU oracle (`parity.meets_north_star`).  The plain-fp16 engine (faster, but its results
drift past the tolerance) and the exact-f32 engine are reported beside it as `fp16_engine` / `fp32_engine` (--full).

One step = one pass of the whole predict pipeline (letterbox[identity] -> 76-conv network -> decode ->
NMS -> mask assembly (bit-packed) -> scale_boxes) over one batch of 64 synthetic 640x640x3 uint8
frames per GPU, inputs already resident in HBM.  Network and post-processing run in series on one stream, so the forward's
HIP-event time in the timed region is its own.  --pipeline overlaps post-processing of batch k-1 with the network of batch k
on a second stream (~6 % more frames/s; every batch's full output is still complete before the closing barrier); the forward
then shares the chip, which is why `roofline.isolated` (--full) also reports the same forward timed alone right after the timed region.  N > 1: one process per GPU; frames live on rank 0
and every step scatters the next batch / gathers the previous batch's detections + bit-packed masks
over RCCL (xGMI) on a side stream, overlapped with compute (weak scaling: 64 frames per GPU).

Before the W warm-up steps the chip is pre-heated with >= --preheat seconds of the same steps (clocks sag under sustained
MFMA load; a 20-step run is only ~50 ms long), so the timed steps land on settled clocks.

Prints ONE JSON line on rank 0 (contract in the task statement).  A plain run sets up, pre-heats, warms up, times the K steps and
prints the line with
  roofline     -- the conv network (76 MFMA conv launches, >85 % of the step) against the dense fp16
                  MFMA peak: achieved = 2*MAC of all convs per forward / forward time measured with HIP
                  events on the launch stream inside the timed region.
--full adds the measurements and checks that take runs of their own, after the timed region:
  roofline.isolated -- the same forward timed alone on the chip.
  parity       -- the benchmarked engine against the fp32 CPU oracle on --parity-frames of the bench frames,
                  through the same entry points the timed loop uses: mask IoU (min / p1 / mean), |d box| in px and
                  normalised, kept-set equality (north_star: IoU >= 0.999, |d box| < 1e-3, same kept set).
  host_fed     -- the same step with the frames starting in pinned host memory (N = 1 only).
  fp16_engine / fp32_engine -- the same pipeline, weights and frames on the other two storage types, each with the driver's
                  --steps / --warmup, its own roofline fraction and parity object (N = 1 only).
  cpu_baseline -- the CPU oracle (torch-CPU fp32 restatement, kind "port") timed on this host's cores,
                  rank 0, N = 1 only, on a bounded sample.
The --no-* options and --parity-frames switch single parts of --full off.

--dump-outputs DIR writes what rank 0's last timed step computed as .npy files (see dump_outputs); the frames and weights are seeded,
so two builds run with the same arguments can be compared output for output.
"""
import argparse
import json
import math
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

MFMA_PEAK_TFLOPS = 2517.0      # dense fp16: 256 CU x 4 SIMD x 1024 FLOP/clk x 2.4 GHz (MI355X_MICROARCH.md: ~2.5 PF)
# h2 (split-fp16): an algorithmic MAC needs at least three fp16 MFMA MACs (wh*xh, wh*xl, wl*xh), so the dense ceiling of the dtype is a
# third of the fp16 pipe's (the figure round 2's review set for this scheme: 2,517 / 3 = 839 TF/s); this build issues four (two
# MFMAs per 16 channels, the second half-filled).  Both fractions are reported: against 839 (`frac`) and against 2,517 (`frac_of_fp16_pipe`).
H2_PEAK_TFLOPS = MFMA_PEAK_TFLOPS / 3.0
F32_MFMA_PEAK_TFLOPS = 157.3   # f32-input MFMA (v_mfma_f32_16x16x4_f32): 64 FLOP/clk/SIMD = 1/16 of the fp16 rate (same guide)
HBM_PEAK_GBS = 8000.0
CONF, IOU, MAX_DET = 0.25, 0.7, 300      # Ultralytics predict() defaults
UNSCORED = os.environ.get("VTI_BENCH_UNSCORED") == "1"     # A/B aid: vti_forward + vti_nms (class scores re-scanned) instead of the scored pair
SLOTS_PER_FRAME = 64                     # mask output capacity = B * SLOTS_PER_FRAME instances (shared by the batch)


def calibrated_weights(vti_amd, eng, frames, conf, target):
    """Random nets with Ultralytics' stock class prior emit no detections at all, which would leave
    NMS and mask assembly idle.  Shift the class bias (GPU path only) so ~`target` anchors per frame
    clear `conf`; everything else stays the seeded He init."""
    eng.load_weights(vti_amd.random_weights(eng, seed=1, cls_bias=0.0), torch.cuda.current_device())
    pred, _ = eng.forward(frames[:8].contiguous())
    p = pred[:, 4:4 + eng.nc].amax(1).flatten().clamp(1e-7, 1 - 1e-7)
    logit = torch.log(p / (1 - p))
    top = torch.topk(logit, target * 8 + 1).values
    kth = 0.5 * (top[-2].item() + top[-1].item())       # midway between two anchors: no score sits exactly on the threshold
    bias = float(math.log(conf / (1 - conf)) - kth)
    blob = vti_amd.random_weights(eng, seed=1, cls_bias=bias)
    eng.load_weights(blob, torch.cuda.current_device())
    return blob, bias


def cpu_baseline(blob, H, W, nc, budget_s=12.0):
    """The oracle's full pipeline (fp32) on the host cores.  `value` is the best of the bs = 1 / 8 / 64 rates (`by_batch`,
    BASELINE.md section 3; bs=8 gets about budget_s of CPU work), `stage_ms_per_frame` the split at bs=8."""
    from oracle.model import OracleModel
    from oracle.postproc import non_max_suppression, process_mask, scale_boxes
    # host threads: the cores this process may actually use (a 1-GPU box grants 16 of the host's
    # cores; asking torch for all 256 hardware threads oversubscribes them ~16x)
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    threads = max(1, min(avail, int(os.environ.get("VTI_CPU_THREADS", "16"))))
    torch.set_num_threads(threads)
    om = OracleModel(blob, H, W, "fp32")
    rng = np.random.Generator(np.random.PCG64(0))
    stage = {"net": 0.0, "nms": 0.0, "masks": 0.0}

    def one(frames):
        t0 = time.perf_counter()
        pred, proto = om.forward_u8(frames, swap_rb=True)
        t1 = time.perf_counter()
        dets = non_max_suppression(pred.numpy(), CONF, IOU, MAX_DET, nc=nc)
        t2 = time.perf_counter()
        for b, d in enumerate(dets):
            if len(d):
                process_mask(proto[b], d[:, 6:], d[:, :4], (H, W), "logit")
                scale_boxes((H, W), d[:, :4], (H, W))
        t3 = time.perf_counter()
        stage["net"] += t1 - t0; stage["nms"] += t2 - t1; stage["masks"] += t3 - t2

    def rate(bs, budget, max_it):
        frames = rng.integers(0, 256, (bs, H, W, 3), dtype=np.uint8)
        one(frames)                             # warm-up (oneDNN primitive creation for this batch size)
        for k in stage: stage[k] = 0.0
        t0 = time.perf_counter()
        it = 0
        while True:
            one(frames)
            it += 1
            dt = time.perf_counter() - t0
            if dt > budget or it >= max_it:
                break
        return bs * it / dt, it, dt

    v8, it8, dt8 = rate(8, budget_s, 32)
    split = {k: round(v / (8 * it8) * 1e3, 3) for k, v in stage.items()}
    v1, it1, dt1 = rate(1, 3.0, 16)
    v64, it64, dt64 = rate(64, 4.0, 2)
    best_bs, best_v = max((("1", v1), ("8", v8), ("64", v64)), key=lambda t: t[1])
    return dict(value=round(best_v, 3), unit="frames/s", cores=torch.get_num_threads(), kind="port",
                sample=f"best of three batch sizes (bs={best_bs}); bs=8: {it8} iterations of {H}x{W} frames, full predict pipeline "
                       f"(net fp32 + NMS + process_mask), torch-CPU oracle, {dt8:.1f} s; bs=1 and bs=64 below",
                by_batch={"1": round(v1, 3), "8": round(v8, 3), "64": round(v64, 3)},
                by_batch_sample=f"bs=1: {it1} it / {dt1:.1f} s; bs=64: {it64} it / {dt64:.1f} s",
                stage_ms_per_frame=split)


def parity_check(eng, blob, frames_dev, nc, H, W, n_frames):
    """The engine's detections + masks for the first n_frames bench frames against the fp32 CPU oracle (checker only;
    runs after the timed region)."""
    from oracle import parity as op
    fr = frames_dev[:n_frames].contiguous()
    got = op.engine_predict(eng, fr, CONF, IOU, MAX_DET)
    want = op.oracle_predict(blob, fr.cpu().numpy(), nc, CONF, IOU, MAX_DET, mode="fp32")
    res = op.compare(got, want, H, W)
    res["frames"] = n_frames
    res["oracle"] = "torch-CPU fp32 restatement of Ultralytics predict (oracle/, parity unpinned)"
    return res


def other_engine_line(vti_amd, dtype, blob, frames, B, H, W, nc, cap, dev, n_par, steps, warmup):
    """The same pipeline, weights and frames on another storage type: frames/s, its own roofline fraction and its parity against
    the fp32 CPU oracle.  Timed like the headline: >= 0.5 s of untimed steps, `warmup` steps, then `steps` steps between syncs."""
    eng = vti_amd.Engine("n", nc, H=H, W=W, max_batch=B, dtype=dtype)
    eng.load_weights(blob, torch.cuda.current_device())
    o = eng.alloc_outputs(B, MAX_DET, cap, "bits", dev)
    st = torch.cuda.current_stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * steps)]

    def step(i=None):
        if i is not None: ev[2 * i].record(st)
        eng.forward(frames, True, pred=o["pred"], proto=o["proto"], best=None if UNSCORED else o["best"])
        if i is not None: ev[2 * i + 1].record(st)
        eng.nms(o["pred"], CONF, IOU, MAX_DET, False, dets=o["dets"], counts=o["counts"], best=None if UNSCORED else o["best"])
        eng.masks(o["dets"], o["counts"], o["proto"], "logit", "bits", capacity=cap, masks=o["masks"], offsets=o["offsets"])
        eng.scale_boxes(o["dets"], o["counts"], H, W, xyxy=o["xyxy"])
    t_heat = time.perf_counter()
    while time.perf_counter() - t_heat < 0.5:
        for _ in range(4):
            step()
        torch.cuda.synchronize()
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        step(i)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    fwd_ms = float(np.mean([ev[2 * i].elapsed_time(ev[2 * i + 1]) for i in range(steps)]))
    ach = 2.0 * eng.macs_per_frame * B / (fwd_ms * 1e-3) / 1e12
    peak = PEAKS[dtype]
    res = dict(dtype=DTYPE_TAG[dtype], value=round(B * steps / dt, 1), unit="frames/s", steps=steps, warmup=warmup, ms_per_step=round(dt / steps * 1e3, 4),
               roofline=dict(bound="mfma", achieved=round(ach, 2), peak=peak, unit="TFLOP/s", frac=round(ach / peak, 5), avg_ms=round(fwd_ms, 4)),
               note=DTYPE_NOTE[dtype])
    if n_par > 0:
        res["parity"] = parity_check(eng, blob, frames, nc, H, W, n_par)
    return res


def host_fed_line(vti_amd, eng, frames, B, H, W, cap, dev, steps, warmup):
    """The same step with the frames starting in HOST memory (main.py:188 -> measurement.py:205-210): a
    vti_amd.FrameFeeder ring of pinned staging buffers, the H2D copy of batch k+1 on a copy stream under the compute of batch k.
    PCIe-inclusive, therefore never the headline `value` (which the contract defines with inputs resident in HBM)."""
    feeder = vti_amd.FrameFeeder(B, H, W, depth=3, device=dev)
    host = frames.cpu().numpy()
    for sl in range(feeder.depth):
        feeder.host_view(sl)[:] = host                       # the "camera" has filled every staging buffer
    outs = [eng.alloc_outputs(B, MAX_DET, cap, "bits", dev) for _ in range(2)]

    def run(n):
        nxt = feeder.submit(feeder.next_slot())
        for k in range(n):
            cur = nxt
            if k + 1 < n:
                nxt = feeder.submit(feeder.next_slot())      # next batch's copy goes out before this batch's kernels are enqueued
            o = outs[k & 1]
            x = feeder.frames(cur)
            eng.forward(x, True, pred=o["pred"], proto=o["proto"], best=o["best"])
            feeder.release(cur)
            eng.nms(o["pred"], CONF, IOU, MAX_DET, False, dets=o["dets"], counts=o["counts"], best=o["best"])
            eng.masks(o["dets"], o["counts"], o["proto"], "logit", "bits", capacity=cap, masks=o["masks"], offsets=o["offsets"])
            eng.scale_boxes(o["dets"], o["counts"], H, W, xyxy=o["xyxy"])
        torch.cuda.synchronize()
    run(max(2, warmup))
    t0 = time.perf_counter()
    run(steps)
    dt = time.perf_counter() - t0
    return dict(value=round(B * steps / dt, 1), unit="frames/s", steps=steps, ms_per_step=round(dt / steps * 1e3, 4),
                h2d_gb_per_s=round(B * H * W * 3 * steps / dt / 1e9, 2),
                note="frames start in pinned host memory: vti_amd.FrameFeeder (3-slot ring, async H2D on a copy stream, event-chained into the "
                     "predict kernels); PCIe-inclusive rate, not the headline")


def dump_outputs(vti_amd, d, o, B, H, W, cap, n_frames=8, n_inst=2, n_full=2, seed=0):
    """--dump-outputs: the arrays a caller of the timed pipeline receives from one step (output set `o`), as float32 / float64 .npy in
    `d` (~45 MB).  Rows past a frame's detection count and mask slots past the live ones are zeroed: the pipeline does not write them.
      dets [B,max_det,6+nm] f32, xyxy [B,max_det,4] f32, counts [B] / offsets [B+1] f64 -- whole;
      mask_area [live slots] f64 -- pixels set in every live mask (the bit-packed masks are ~50 kB each, too many to write whole);
      frame_sample [n_frames] f64 -- a fixed seeded sample of frame indices, and for those frames
      masks_sample [n_frames, n_inst, H, W] f32 -- the first n_inst instance masks unpacked to 0/1 (zeros where a frame has fewer),
      pred_sample [n_full, 4+nc+nm, A] f32 / proto_sample [n_full, H/4, W/4, nm] f32 -- the forward's outputs of the first n_full."""
    os.makedirs(d, exist_ok=True)
    counts = o["counts"].cpu().numpy().astype(np.int64)
    offsets = o["offsets"].cpu().numpy().astype(np.int64)
    max_det = o["dets"].shape[1]
    valid = (np.arange(max_det)[None, :] < counts[:, None])[..., None]
    n_live = int(min(max(offsets[-1], 0), cap))
    popc = torch.tensor([bin(i).count("1") for i in range(256)], dtype=torch.int64, device=o["masks"].device)
    area = torch.cat([popc[o["masks"][i:min(i + 256, n_live)].long()].sum((1, 2)) for i in range(0, n_live, 256)]) if n_live else torch.zeros(0)
    fr = np.sort(np.random.Generator(np.random.PCG64(seed)).choice(B, min(n_frames, B), replace=False))
    ms = np.zeros((len(fr), n_inst, H, W), np.float32)
    for j, b in enumerate(fr):
        for i in range(n_inst):
            slot = offsets[b] + i
            if i < counts[b] and slot < n_live:
                ms[j, i] = vti_amd.unpack_bits(o["masks"][slot], W).cpu().numpy()
    out = {"dets": np.where(valid, o["dets"].cpu().numpy(), 0).astype(np.float32),
           "xyxy": np.where(valid, o["xyxy"].cpu().numpy(), 0).astype(np.float32),
           "counts": counts.astype(np.float64), "offsets": offsets.astype(np.float64),
           "mask_area": area.cpu().numpy().astype(np.float64), "frame_sample": fr.astype(np.float64), "masks_sample": ms,
           "pred_sample": o["pred"][torch.as_tensor(fr[:n_full])].float().cpu().numpy(),
           "proto_sample": o["proto"][torch.as_tensor(fr[:n_full])].float().cpu().numpy()}
    for name, a in out.items():
        np.save(os.path.join(d, name + ".npy"), np.ascontiguousarray(a))
    return sorted(out)


DTYPE_TAG = {"h2": "f16x2", "fp16": "f16", "fp32": "f32"}
PEAKS = {"h2": round(H2_PEAK_TFLOPS, 1), "fp16": MFMA_PEAK_TFLOPS, "fp32": F32_MFMA_PEAK_TFLOPS}
DTYPE_NOTE = {
    "h2": "split-fp16 storage: every weight and activation an fp16 (hi, lo) pair (22-23 significant bits), all products on the fp16 matrix "
          "pipe (v_mfma_f32_16x16x32_f16, two per 16 input channels), f32 accumulation",
    "fp16": "plain fp16 storage of weights and activations, one v_mfma_f32_16x16x32_f16 per 32 input channels: fastest, but 11-bit storage "
            "drifts past the north-star tolerance on these networks (profiles/r03_precision_ablation.txt: >= 20 bits needed)",
    "fp32": "exact-f32 MFMA (v_mfma_f32_16x16x4_f32), fp32 activations",
}


def free_port():
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def launch_ranks(n):
    """`python bench.py --gpus N` without a launcher: start N fresh rank processes (this parent has touched no GPU and never
    execs), let rank 0's JSON line through on stdout, return the worst exit code.  A rank that dies takes the others down."""
    port = free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    worst, deadline = 0, None
    while any(p.poll() is None for p in procs):
        for p in procs:
            rc = p.poll()
            if rc not in (None, 0) and deadline is None:
                worst, deadline = rc, time.time() + 20.0       # the others are probably stuck in a collective: give them 20 s
        if deadline is not None and time.time() > deadline:
            for p in procs:
                if p.poll() is None:
                    p.terminate()
            deadline = time.time() + 1e9
        time.sleep(0.2)
    for p in procs:
        if p.returncode != 0 and worst == 0:
            worst = p.returncode
    return worst if worst >= 0 else 128 - worst


def dry_main(args, world, rank):
    """--dry: the launch, the per-step exchange (scatter of frames / gather of detections [+ live masks]) and the JSON line on CPU
    tensors over gloo -- no GPU, no kernel; the "compute" of a step writes rank-tagged outputs.  For the CPU test of the N > 1 path."""
    import torch.distributed as dist
    from vti_amd import dataparallel as dp
    dev = torch.device("cpu")
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(args.backend, rank=rank, world_size=world)
    B, H, W, nm, cap = args.batch, 32, 32, 32, args.batch * 4
    outs = [dict(dets=torch.zeros((B, MAX_DET, 6 + nm)), counts=torch.zeros((B,), dtype=torch.int32), xyxy=torch.zeros((B, MAX_DET, 4)),
                 offsets=torch.zeros((B + 1,), dtype=torch.int32), masks=torch.zeros((cap, H, W // 8), dtype=torch.uint8),
                 stats=torch.zeros((cap, 5), dtype=torch.int64), envelope=torch.zeros((B, W), dtype=torch.int32)) for _ in range(2)]
    root_pool = torch.arange(world * B * H * W * 3, dtype=torch.int64).remainder(251).to(torch.uint8).view(world * B, H, W, 3) if rank == 0 else None
    shards = [torch.zeros((B, H, W, 3), dtype=torch.uint8) for _ in range(2)]
    ok, gathered = True, None
    exchange = world > 1 and not args.no_exchange

    def step(k):
        nonlocal ok, gathered
        cur, nxt = k & 1, (k + 1) & 1
        if exchange:
            shards[nxt] = dp.scatter_frames(root_pool, B, (H, W, 3), dev)
            gathered = dp.gather_detections(outs[nxt], reuse=nxt)
            if args.gather_masks:
                dp.gather_live_masks(outs[nxt]["masks"], outs[nxt]["offsets"])
        o = outs[cur]
        o["counts"].fill_(1 + rank); o["dets"].fill_(float(rank)); o["offsets"].copy_(torch.arange(B + 1, dtype=torch.int32) * (1 + rank))
    t0 = time.perf_counter()
    for k in range(args.warmup + args.steps):
        step(k)
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if exchange:
        lo = rank * B
        ok &= bool(torch.equal(shards[(args.warmup + args.steps) & 1], torch.arange(world * B * H * W * 3, dtype=torch.int64).remainder(251).to(torch.uint8).view(world * B, H, W, 3)[lo:lo + B]))
        if rank == 0:
            ok &= gathered is not None and gathered["counts"].shape[0] == world * B and gathered["counts"].view(world, B)[:, 0].tolist() == [1 + r for r in range(world)]
        flag = torch.tensor([1.0 if ok else 0.0], dtype=torch.float64)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        ok = bool(flag.item() == 1.0)
    if rank == 0:
        print(json.dumps({"metric": "frames/sec whole-node, YOLOv8n-seg 640x640 bs=64; mask IoU vs CPU ref", "dry": True, "value": round(world * B * args.steps / elapsed, 1),
                          "unit": "frames/s (no kernels: launch + exchange only)", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                          "ranks": dist.get_world_size() if world > 1 else 1, "backend": args.backend, "exchange_ok": ok,
                          "exchange": "scatter of uint8 frames + gather of dets/counts/xyxy/offsets/stats/envelope" + ("; + live masks" if args.gather_masks else "") if exchange else "none",
                          "config": {"workload": "dry run: CPU tensors, no kernels", "global_batch": world * B, "parallelism": f"dp{world}"}}), flush=True)
    if world > 1:
        dist.destroy_process_group()
    return 0 if ok else 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64, help="frames per GPU per step")
    ap.add_argument("--dtype", default="h2", choices=["h2", "fp16", "fp32"],
                    help="storage type of the HEADLINE engine (default h2: the one that meets the north-star tolerance)")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"], help="torch.distributed backend for N > 1 (nccl = RCCL; gloo with --dry)")
    ap.add_argument("--dry", action="store_true", help="no GPU, no kernels: run the rank launch + per-step exchange + JSON path on CPU tensors (tests)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-exchange", action="store_true", help="N>1: skip the per-step scatter/gather")
    ap.add_argument("--rehearse-exchange", action="store_true",
                    help="N=1 only: open a ONE-rank process group on --backend and run the per-step scatter/gather through it (the RCCL code "
                         "path of the N>1 run -- dtypes, streams, receive buffers -- on a single-GPU box); the line is marked as a rehearsal")
    ap.add_argument("--gather-masks", action="store_true",
                    help="N>1: also ship every rank's LIVE bit-packed mask slots to the root each step (variable-length point-to-point "
                         "gather, one host read of the slot count per step); default: dets/counts/xyxy + on-device reductions only")
    ap.add_argument("--preheat", type=float, default=1.0, help="seconds of untimed steps before the warm-up steps (clock settling)")
    ap.add_argument("--parity-frames", type=int, default=8, help="bench frames checked against the fp32 CPU oracle after the timed region (0: skip)")
    ap.add_argument("--no-fp32-line", action="store_true", help="skip the secondary fp32-engine measurement + parity")
    ap.add_argument("--no-host-fed", action="store_true", help="skip the secondary measurement with frames starting in (pinned) host memory")
    ap.add_argument("--no-fp16-line", action="store_true", help="skip the secondary plain-fp16-engine measurement + parity")
    ap.add_argument("--pipeline", action="store_true",
                    help="overlap post-processing of batch k-1 with the network of batch k on a second stream: ~6 %% more frames/s "
                         "(24.7k vs 23.2k on one MI355X), but the forward then shares the chip and its in-region HIP-event time (the "
                         "roofline line) is inflated; default: the stages in series on one stream")
    ap.add_argument("--full", action="store_true",
                    help="after the timed region also run what takes runs of its own: the isolated forward (roofline.isolated), parity "
                         "against the CPU oracle, the host-fed, fp16 / fp32 engine lines and the CPU baseline; default: the headline only")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the last timed step computed (rank 0) as DIR/<name>.npy, float32 / float64 (see dump_outputs)")
    args = ap.parse_args()
    if args.dry and args.dump_outputs:
        ap.error("--dump-outputs needs the GPU path (not --dry)")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:      # plain `python bench.py --gpus N`: be the launcher (no GPU touched yet)
        sys.exit(launch_ranks(args.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if rank == 0:
            print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}", file=sys.stderr)
        sys.exit(2)
    if args.dry:
        sys.exit(dry_main(args, world, rank))

    import vti_amd
    from vti_amd import dataparallel as dp

    if not torch.cuda.is_available():
        print("bench.py needs a ROCm GPU (no CPU fallback for the product path)", file=sys.stderr)
        sys.exit(2)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    grouped = world > 1 or args.rehearse_exchange      # a process group exists (world == 1 only under --rehearse-exchange)
    if grouped:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group(args.backend, rank=rank, world_size=world, device_id=dev)   # "nccl" == RCCL on ROCm

    B, H, W, nc = args.batch, 640, 640, 80
    eng = vti_amd.Engine("n", nc, H=H, W=W, max_batch=B, dtype=args.dtype)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    frames = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device=dev, generator=gen)
    # the class prior is calibrated on the SAME seeded frames on every rank (deterministic kernels: identical bias, i.e. the weights
    # really are replicas); ranks > 0 then draw their own frames
    blob, bias = calibrated_weights(vti_amd, eng, frames, CONF, target=60)
    if rank > 0:
        gen.manual_seed(1234 + rank)
        frames = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device=dev, generator=gen)
    cap = B * SLOTS_PER_FRAME
    outs = [eng.alloc_outputs(B, MAX_DET, cap, "bits", dev) for _ in range(2)]
    for o in outs:                           # a gather that runs before this buffer's first post-processing must see "no detections"
        o["counts"].zero_(); o["offsets"].zero_()
    shards = [frames, frames.clone()]
    FABRIC_CLS = 1                          # the reference's FABRIC_CLASS_ID (config.py:70): whose union envelope the consumer reads

    exchange = grouped and not args.no_exchange
    exch_note = "none (single GPU)" if not grouped else "disabled (--no-exchange)"
    if exchange:                            # what the consumer needs from a frame travels, not the mask buffer
        for o in outs:
            o["stats"] = torch.empty((cap, 5), dtype=torch.int64, device=dev)
            o["envelope"] = torch.empty((B, W), dtype=torch.int32, device=dev)
    comm = torch.cuda.Stream(device=dev) if exchange else None
    root_pool = None
    if exchange and rank == 0:       # the node's frames live on the root GPU
        root_pool = torch.randint(0, 256, (world * B, H, W, 3), dtype=torch.uint8, device=dev, generator=gen)

    ev_f0 = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps)]
    ev_f1 = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps)]
    ev_p0 = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps)]
    ev_end = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps)]
    main_stream = torch.cuda.current_stream()
    # Two-stage software pipeline on one GPU: the network of batch k runs on the main stream while NMS + mask
    # assembly + scale_boxes of batch k-1 run on a second stream (outputs are double-buffered).  The forward
    # fills the chip; post-processing is latency/VALU-bound with few workgroups and hides underneath it.
    pipelined = args.pipeline
    post_stream = torch.cuda.Stream(device=dev) if pipelined else main_stream
    fwd_done = [torch.cuda.Event(), torch.cuda.Event()]
    post_done = [None, None]

    def step(k, timed_idx=None):
        cur, nxt = k & 1, (k + 1) & 1
        ready = None
        if exchange:
            with torch.cuda.stream(comm):
                if post_done[nxt] is not None:
                    comm.wait_event(post_done[nxt])  # step k-1's outputs (outs[nxt]) are complete
                else:
                    comm.wait_stream(main_stream)
                shards[nxt] = dp.scatter_frames(root_pool, B, (H, W, 3), dev)
                dp.gather_detections(outs[nxt], reuse=nxt)
                if args.gather_masks:
                    dp.gather_live_masks(outs[nxt]["masks"], outs[nxt]["offsets"])
                ready = torch.cuda.Event()
                ready.record(comm)
        x, o = shards[cur], outs[cur]
        if post_done[cur] is not None:
            main_stream.wait_event(post_done[cur])   # post of step k-2 no longer reads outs[cur]
        if timed_idx is not None:
            ev_f0[timed_idx].record(main_stream)
        eng.forward(x, True, pred=o["pred"], proto=o["proto"], best=None if UNSCORED else o["best"])
        if timed_idx is not None:
            ev_f1[timed_idx].record(main_stream)
        fwd_done[cur].record(main_stream)
        with torch.cuda.stream(post_stream):
            post_stream.wait_event(fwd_done[cur])
            if timed_idx is not None:
                ev_p0[timed_idx].record(post_stream)
            eng.nms(o["pred"], CONF, IOU, MAX_DET, False, dets=o["dets"], counts=o["counts"], best=None if UNSCORED else o["best"])
            eng.masks(o["dets"], o["counts"], o["proto"], "logit", "bits", capacity=cap, masks=o["masks"], offsets=o["offsets"])
            eng.scale_boxes(o["dets"], o["counts"], H, W, xyxy=o["xyxy"])
            if exchange:                    # consumer reductions straight from the bit-packed masks: the gather's payload
                eng.mask_stats_bits(o["masks"], H, W, stats=o["stats"], offsets=o["offsets"])
                eng.envelope_bits(o["masks"], o["offsets"], o["dets"], FABRIC_CLS, H, W, envelope=o["envelope"])
            if timed_idx is not None:
                ev_end[timed_idx].record(post_stream)
            post_done[cur] = torch.cuda.Event()
            post_done[cur].record(post_stream)
        if ready is not None:
            main_stream.wait_event(ready)            # next shard landed; results of k-1 gathered

    def barrier():
        torch.cuda.synchronize()
        if grouped:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    if exchange:
        # a failing exchange is fatal (exit code != 0): a scaling number without it is not a sharded run; --no-exchange says so explicitly
        try:
            step(0)
            torch.cuda.synchronize()
        except Exception as e:
            print(f"bench.py: rank {rank}: the RCCL scatter/gather step failed ({type(e).__name__}: {e}); "
                  f"fix it or pass --no-exchange", file=sys.stderr, flush=True)
            sys.exit(3)
        exch_note = ("per step: RCCL scatter of uint8 frames from rank 0 + gather of dets/counts/xyxy/offsets + on-device consumer "
                     "reductions (per-instance moments/extents, per-frame fabric envelope), side stream, overlapped"
                     + ("; + live bit-packed mask slots (variable length)" if args.gather_masks else ""))
    # pre-heat: sustained load until the clocks have settled (untimed), then the W warm-up steps of the contract
    t_heat = time.perf_counter()
    n_heat = 0
    while True:
        for _ in range(8):
            step(n_heat); n_heat += 1
        torch.cuda.synchronize()
        heated = time.perf_counter() - t_heat
        if grouped:                                  # every rank must run the same number of (collective) steps
            heated = dp.max_over_ranks(heated, dev)
        if heated >= args.preheat:
            break
    if n_heat & 1:                                   # keep the double-buffer phase: step k uses buffer k & 1
        step(n_heat); n_heat += 1
    for k in range(args.warmup):
        step(k)
    barrier()
    t0 = time.perf_counter()
    for k in range(args.steps):
        step(k, k)
    barrier()
    elapsed = time.perf_counter() - t0
    if grouped:
        elapsed = dp.max_over_ranks(elapsed, dev)
    if args.dump_outputs and rank == 0:              # the last timed step wrote outs[(steps - 1) & 1]; nothing has touched it since
        dump_outputs(vti_amd, args.dump_outputs, outs[(args.steps - 1) & 1], B, H, W, cap)

    if args.full:
        # the forward alone (nothing else on the chip), HIP events on the launch stream, right after the timed region
        iso0, iso1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n_iso = max(5, min(20, args.steps))
        eng.forward(shards[0], True, pred=outs[0]["pred"], proto=outs[0]["proto"], best=None if UNSCORED else outs[0]["best"])
        torch.cuda.synchronize()
        iso0.record(main_stream)
        for _ in range(n_iso):
            eng.forward(shards[0], True, pred=outs[0]["pred"], proto=outs[0]["proto"], best=None if UNSCORED else outs[0]["best"])
        iso1.record(main_stream)
        torch.cuda.synchronize()
        iso_ms = iso0.elapsed_time(iso1) / n_iso

    fwd_ms = float(np.mean([a.elapsed_time(b) for a, b in zip(ev_f0, ev_f1)]))
    post_ms = float(np.mean([a.elapsed_time(b) for a, b in zip(ev_p0, ev_end)]))
    dets_per_frame = float(outs[(args.steps - 1) & 1]["counts"].float().mean().item())
    total_frames = world * B * args.steps
    value = total_frames / elapsed
    flops_per_forward = 2.0 * eng.macs_per_frame * B
    achieved = flops_per_forward / (fwd_ms * 1e-3) / 1e12
    # MACs the kernels actually issue: the ConvTranspose folded into the 3x3 behind it runs as four 2x2 convs on the low-resolution map
    # (h_in * w_in * c1 * 4 * c2 * 4 MACs instead of the two layers' own); every other conv issues its algorithmic MACs
    tab = eng.conv_table()
    exec_macs = eng.macs_per_frame
    for i, tr in enumerate(tab):
        if tr["kind"] == 2 and tr["lds"] == 0 and i + 1 < len(tab):         # folded deconv (vti_conv_at reports it without an LDS size of its own)
            nxt = tab[i + 1]
            exec_macs += tr["h_in"] * tr["w_in"] * tr["c1"] * 4 * nxt["c2"] * 4 - tr["macs"] - nxt["macs"]
    flops_executed = 2.0 * exec_macs * B
    peak = PEAKS[args.dtype]

    # HBM bytes per forward from the committed rocprofv3 PMC passes (tools/make_profiles.sh): only
    # valid for the configuration they were collected on.
    traffic = None
    tpath = next((q for q in (os.path.join(ROOT, "profiles", f"r{r:02d}_hbm_traffic.json") for r in range(9, 0, -1)) if os.path.exists(q)), "")
    if tpath and B == 64 and json.load(open(tpath)).get("dtype", "fp16") == args.dtype:
        fam = json.load(open(tpath))["families"]
        traffic = sum(v["total_bytes"] for k, v in fam.items() if k.startswith("conv family") or k in ("decode_kernel", "sppf_pool", "upsample2x"))    # the forward's kernels

    if rank == 0:
        line = {
            "metric": "frames/sec whole-node, YOLOv8n-seg 640x640 bs=64; mask IoU vs CPU ref",
            "value": round(value, 1), "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": DTYPE_TAG[args.dtype], "dtype_note": DTYPE_NOTE[args.dtype], "data": "synthetic",
            "config": {"workload": f"YOLOv8n-seg nc=80 640x640 bs={B} per GPU, full predict: net + decode + NMS + "
                                   f"bit-packed masks + scale_boxes (BASELINE configs[2]; configs[1] is the bs=1 case)",
                       "global_batch": world * B, "weights": f"seeded random (He, seed 1), class bias calibrated to {bias:.3f}",
                       "conf": CONF, "iou": IOU, "max_det": MAX_DET, "detections_per_frame": round(dets_per_frame, 2),
                       "pipeline": ("post-processing of batch k overlaps the network of batch k+1 on a second stream"
                                    if pipelined else "network and post-processing in series"),
                       "mask_capacity": cap, "masks_dropped": max(0, int(outs[(args.steps - 1) & 1]["offsets"][-1].item()) - cap), "parallelism": f"dp{world}", "exchange": exch_note,
                       "ranks": world, "backend": args.backend if grouped else None,
                       **({"rehearsal": "one-rank process group: the N>1 exchange path on a single GPU, not a scaling number"} if args.rehearse_exchange else {})},
            "roofline": {"bound": "mfma", "achieved": round(achieved, 2), "peak": peak, "unit": "TFLOP/s",
                         "frac": round(achieved / peak, 5), "traffic": traffic,
                         "peak_note": ("f16x2 (split-fp16): 2517 / 3 -- an algorithmic MAC costs at least three fp16 MFMA MACs (wh*xh, wh*xl, wl*xh)"
                                       if args.dtype == "h2" else "dense MFMA peak of the dtype (MI355X_MICROARCH.md)"),
                         "frac_of_fp16_pipe": round(achieved / MFMA_PEAK_TFLOPS, 5) if args.dtype != "fp32" else None,
                         "mfma_issue_frac": round(achieved / MFMA_PEAK_TFLOPS * (4.0 if args.dtype == "h2" else 1.0), 5) if args.dtype != "fp32" else None,
                         "mfma_issue_note": "share of the fp16 matrix pipe's time the ISSUED MFMAs occupy (h2 issues 4 fp16 MFMA MACs per algorithmic MAC; `achieved` counts algorithmic flops only)",
                         "traffic_note": "HBM bytes per forward (FETCH_SIZE x2 + WRITE_SIZE, separate rocprofv3 --pmc passes, profiles/" + os.path.basename(tpath) + "); algorithmic unfused activation bytes = 91.6 MB/frame",
                         "kernel": f"vti conv family: conv3_pk / conv1_pk (persistent LDS-DMA 3x3 / 1x1) + conv_kernel (fused towers, stride 2) + stem_l1_kernel ({eng.num_launches} launches per forward incl. the SPPF pool; {len(eng.conv_table())} convs, {sum(1 for t in eng.conv_table() if t['fused'])} fused into their producer's kernel, decode fused into the box towers)",
                         "flop_per_launch": flops_per_forward, "avg_ms": round(fwd_ms, 4),
                         "flop_executed_per_launch": flops_executed,
                         "executed_note": "algebraic fold of proto.upsample into proto.cv2: the kernels issue this many flops for the same result; `achieved` and `frac` use the ALGORITHMIC count (SURVEY 8d), the matrix pipe's own utilisation follows from the executed one: "
                                          + f"{flops_executed / (fwd_ms * 1e-3) / 1e12 * (4.0 if args.dtype == 'h2' else 1.0) / (F32_MFMA_PEAK_TFLOPS if args.dtype == 'fp32' else MFMA_PEAK_TFLOPS):.4f} of its peak"},
            "stage_ms": {"forward": round(fwd_ms, 4), "nms+masks+scale_boxes": round(post_ms, 4)},
        }
        line["config"]["preheat"] = f"{n_heat} untimed steps over >= {args.preheat:.1f} s before the {args.warmup} warm-up steps"
        if args.full:
            line["roofline"]["isolated"] = {"avg_ms": round(iso_ms, 4), "achieved": round(flops_per_forward / (iso_ms * 1e-3) / 1e12, 2),
                                            "frac": round(flops_per_forward / (iso_ms * 1e-3) / 1e12 / peak, 5),
                                            "note": f"the same forward alone on the chip, {n_iso} back-to-back launches after the timed region"}
            if args.parity_frames > 0:
                line["parity"] = parity_check(eng, blob, frames, nc, H, W, min(args.parity_frames, B))
                line["parity"]["engine"] = line["dtype"]
                line["parity"]["tolerance"] = "north_star gate: mask IoU >= 0.999 for every instance and |d box| < 1e-3 (normalised by 640) with the same kept set and order: see meets_north_star"
            if world == 1 and not args.no_host_fed:
                line["host_fed"] = host_fed_line(vti_amd, eng, frames, B, H, W, cap, dev, args.steps, args.warmup)
            for other, skip in (("fp16", args.no_fp16_line), ("fp32", args.no_fp32_line)):
                if world == 1 and other != args.dtype and not skip:
                    line[other + "_engine"] = other_engine_line(vti_amd, other, blob, frames, B, H, W, nc, cap, dev, min(args.parity_frames, B), args.steps, args.warmup)
            if world == 1 and not args.no_cpu_baseline:
                line["cpu_baseline"] = cpu_baseline(blob, H, W, nc)
        if args.dump_outputs:
            line["dump_outputs"] = args.dump_outputs
        print(json.dumps(line), flush=True)
    if grouped:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
