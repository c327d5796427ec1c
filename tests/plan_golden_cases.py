"""The cases of the planner's golden dumps (tests/golden/plan_dumps.json), shared by the recorder (tests/golden/make_plan_dumps.py)
and the replay (tests/test_plan_golden.py), and how tests/plan_dump_main.cpp is built and run.  Host only: nothing here needs a GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vision-textile-inspection_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_dumps.json")
DTYPES = {"fp16": 0, "fp32": 1, "h2": 2}

# every switch the planner reads, alone, at each non-default value (the parse oddities included)
ON_SWITCHES = ("VTI_NO_PK", "VTI_NO_PK2", "VTI_NO_PK1", "VTI_PK_WIDE16", "VTI_NO_PK_WSTAT", "VTI_H2_NO_N5", "VTI_PK1_ALL",
               "VTI_PK1_NO_WGPC2", "VTI_PK1_FORCE_WGPC2", "VTI_P3_LANES", "VTI_NO_FUSE", "VTI_NO_FOLD", "VTI_NO_BNECK",
               "VTI_NO_BNECK_TAIL", "VTI_NO_STEM_FUSE", "VTI_NO_STEM_FUSE3", "VTI_NO_PRED_SCATTER", "VTI_NO_DFL_FUSE", "VTI_NO_PK_FOLD",
               "VTI_NO_T512", "VTI_NO_UPFUSE", "VTI_NO_FOLD512")
VALUED = (("VTI_CONV1_WREG", ("0",)), ("VTI_FOLD512", ("0", "1")), ("VTI_PK_FUSED", ("1", "2", "3")),
          ("VTI_PK_DEPTH", ("3", "4", "9", "1")), ("VTI_PK_FOLD_DEPTH", ("2", "4")), ("VTI_PK_LIMIT_BYTES", ("1000000",)),
          ("VTI_PK1_WSTAT_KB", ("0", "32")), ("VTI_PK1_INFLIGHT_KB", ("10",)), ("VTI_NO_PK", ("10", "true")))
PLANNER_SWITCHES = ON_SWITCHES + tuple(n for n, _ in VALUED[:-1])
PLAIN_SWITCHES = ("VTI_NO_FUSE", "VTI_NO_FOLD", "VTI_NO_BNECK", "VTI_NO_STEM_FUSE", "VTI_NO_UPFUSE", "VTI_NO_PK", "VTI_NO_PK1", "VTI_NO_PK2")
PLAIN_PLAN = {k: "1" for k in PLAIN_SWITCHES}        # gpu_util.PLAIN_PLAN
# every switch of csrc/ (the launch-time ones too): none of them may leak in from the caller's environment
ALL_SWITCHES = PLANNER_SWITCHES + ("VTI_PK_MAX_WGS", "VTI_PK_STAGGER", "VTI_PK_LINEAR_MAP", "VTI_SINGLE_STREAM", "VTI_LIST_OPS",
                                   "VTI_STAMP_OP", "VTI_MASK_WGS_PER_CU", "VTI_STEM_NOT_PERSISTENT")

RAGGED = [(224, 352, "h2", 3), (224, 352, "h2", 64), (224, 352, "fp16", 3), (224, 352, "fp16", 64), (224, 352, "fp32", 3),
          (608, 736, "h2", 1), (608, 736, "fp16", 1)]        # test_plan_ragged.CASES
SWITCH_BASES = [("n", 80, 640, 640, 64, "h2"), ("n", 80, 640, 640, 64, "fp16"), ("n", 80, 224, 352, 3, "fp32")]
# these also store a 4-hex-digit fingerprint of every line of their dump, so that a mismatch can name its first differing line
# (the dumps themselves, ~55 KB each, are not stored: the SHA-256 pins the bytes)
FULL = {"n80_640x640_b64_h2", "n80_640x640_b64_fp16", "n80_640x640_b64_fp32", "n2_960x960_b8_h2", "n80_224x352_b3_fp32",
        "n80_608x736_b1_h2", "s80_640x640_b8_h2", "n80_640x640_b64_h2+PLAIN"}


def line_prints(dump):
    import hashlib
    return "".join(hashlib.sha256(l.encode()).hexdigest()[:4] for l in dump.splitlines())


def plan_argv(scale, nc, H, W, max_batch, dtype, nm=32):
    return ["plan", scale, str(nc), str(nm), str(H), str(W), str(max_batch), str(DTYPES.get(dtype, dtype))]


def base_id(scale, nc, H, W, max_batch, dtype):
    return f"{scale}{nc}_{H}x{W}_b{max_batch}_{dtype}"


def _forced():
    """(dtype, B, H, W, c1, c2, k, s, kind, th, tw, wn, nrep, env) of every debug_conv2d call of test_gpu_conv.py and
    test_gpu_conv1x1_wreg.py."""
    import test_gpu_conv as tc
    import test_gpu_conv1x1_wreg as tw
    out = []
    for dt in ("fp16", "fp32", "h2"):
        for k, s, kind, c1, c2, H, W, (wn, nrep), ex in tc.CASES:
            out.append((dt, 2, H, W, c1, c2, k, s, kind, 0, 0, wn, nrep, {"VTI_PK_MAX_WGS": str(ex["pk_wgs"])} if "pk_wgs" in ex else {}))
        out.append((dt, 2, 24, 20, 64, 64, 3, 1, 0, 0, 0, 0, 0, {}))                 # test_conv_silu_random
        out.append((dt, 2, 46, 62, 3, 16, 3, 2, 0, 0, 0, 0, 0, {}))                  # test_stem_conv_u8
        for arm in ("0", "1"):
            for c1, c2, H, W, (wn, nrep), ex in tw.CASES:
                out.append((dt, 2, H, W, c1, c2, 1, 1, 1, 0, 0, wn, nrep, {"VTI_NO_PK1": "1", "VTI_CONV1_WREG": arm}))
            for c1, c2, H, W, (wn, nrep), wgs, ex in tw.PK_CASES:
                env = {"VTI_CONV1_WREG": arm}
                if wgs:
                    env["VTI_PK_MAX_WGS"] = str(wgs)
                out.append((dt, 2, H, W, c1, c2, 1, 1, 1, 1, 80, wn, nrep, env))
    for c1, c2, H, W, wn, nrep in [(16, 16, 40, 40, 0, 0), (32, 32, 40, 60, 0, 0), (64, 64, 44, 40, 0, 0), (64, 80, 40, 40, 0, 0),
                                   (80, 80, 24, 40, 0, 0), (128, 80, 40, 40, 2, 3), (128, 128, 20, 20, 0, 0), (64, 64, 80, 80, 1, 4)]:
        for wgs in (0, 8):                                                           # test_conv3x3_silu_persistent
            out.append(("fp16", 3, H, W, c1, c2, 3, 1, 0, 0, 0, wn, nrep, {"VTI_PK_MAX_WGS": str(wgs)} if wgs else {}))
    return out


def cases():
    """[(id, argv, env)]: one fresh process of plan_dump_main each."""
    out = []
    bases = [("n", 80, 640, 640, 64, "h2"), ("n", 80, 640, 640, 64, "fp16"), ("n", 80, 640, 640, 64, "fp32"),
             ("n", 2, 960, 960, 8, "h2"), ("n", 2, 960, 960, 8, "fp16")]
    bases += [("n", 80, H, W, B, dt) for H, W, dt, B in RAGGED]
    bases += [("n", 80, 1280, 1280, 4, "h2")]
    bases += [(sc, 80, 640, 640, 8, dt) for sc in ("s", "m") for dt in ("h2", "fp16")]
    for b in bases:
        out.append((base_id(*b), plan_argv(*b), {}))
    out.append(("refuse_scale", plan_argv("q", 80, 640, 640, 1, "h2"), {}))
    out.append(("refuse_H100", plan_argv("n", 80, 100, 640, 1, "h2"), {}))
    out.append(("refuse_batch0", plan_argv("n", 80, 640, 640, 0, "h2"), {}))
    out.append(("refuse_dtype9", plan_argv("n", 80, 640, 640, 1, 9), {}))
    out.append(("refuse_nm30", plan_argv("n", 80, 640, 640, 1, "h2", nm=30), {}))
    for b in SWITCH_BASES:
        envs = [{n: "1"} for n in ON_SWITCHES] + [{n: v} for n, vals in VALUED for v in vals]
        envs += [dict(PLAIN_PLAN), dict(PLAIN_PLAN, VTI_PK1_ALL="1")]
        for env in envs:
            tag = "PLAIN" + ("+VTI_PK1_ALL=1" if "VTI_PK1_ALL" in env else "") if len(env) > 1 else "%s=%s" % next(iter(env.items()))
            out.append((base_id(*b) + "+" + tag, plan_argv(*b), env))
    # VTI_PK1_NO_WGPC2 changes none of the three bases above: it does where conv1_pk runs two fp32 workgroups per CU
    out.append((base_id(*bases[2]) + "+VTI_PK1_NO_WGPC2=1", plan_argv(*bases[2]), {"VTI_PK1_NO_WGPC2": "1"}))
    seen = set()
    for dt, B, H, W, c1, c2, k, s, kind, th, tw, wn, nrep, env in _forced():
        argv = ["cfg"] + [str(v) for v in (DTYPES[dt], B, H, W, c1, c2, k, s, kind, th, tw, wn, nrep)]
        cid = "cfg_" + "_".join(argv[1:]) + "".join(f"+{n}={v}" for n, v in sorted(env.items()))
        if cid not in seen:
            seen.add(cid)
            out.append((cid, argv, env))
    return out


# ---- the launch parameters of one forward (tests/golden/launch_params.json) --------------------------------------------------------
LAUNCH_GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_params.json")
LAUNCH_BASES = [("n", 80, 640, 640, 64, "h2"), ("n", 80, 640, 640, 64, "fp16"), ("n", 80, 640, 640, 64, "fp32"), ("n", 2, 960, 960, 8, "h2"),
                ("n", 80, 224, 352, 3, "fp32"), ("n", 80, 608, 736, 1, "h2"), ("s", 80, 640, 640, 8, "h2")]      # FULL's, and its PLAIN below
# switches of the launch path, and planner switches that steer forward_impl into a branch the defaults never take
LAUNCH_RUN_ENVS = [{"VTI_PK_MAX_WGS": "8"}, {"VTI_PK_STAGGER": "0"}, {"VTI_PK_STAGGER": "3"}, {"VTI_PK_LINEAR_MAP": "1"},
                   {"VTI_STEM_NOT_PERSISTENT": "1"}]
LAUNCH_PLAN_ENVS = [dict(PLAIN_PLAN)] + [{n: "1"} for n in ("VTI_NO_PRED_SCATTER", "VTI_NO_DFL_FUSE", "VTI_NO_UPFUSE", "VTI_NO_FOLD",
                                                           "VTI_NO_PK_FOLD", "VTI_NO_BNECK_TAIL", "VTI_NO_STEM_FUSE3", "VTI_NO_STEM_FUSE",
                                                           "VTI_PK_FUSED")]
# 512 frames of 640x640 on h2: tensors past 2^31 bytes.  The planner keeps such convs off the persistent kernels by itself; with its
# limit raised the launch path meets them: a fused Bottleneck is refused, and without the Bottleneck fusion persistent kernels fall
# back (pk=0) until the folded upsample is refused
BIG = ("n", 80, 640, 640, 512, "h2")
BIG_ENVS = [{}, {"VTI_PK_LIMIT_BYTES": str(1 << 40)}, {"VTI_PK_LIMIT_BYTES": str(1 << 40), "VTI_NO_BNECK": "1"}]
LAUNCH_FULL = {"n80_640x640_b64_h2@B64_swap1_best1", "n80_640x640_b64_fp16@B64_swap1_best1", "n80_640x640_b64_fp32@B1_swap1_best1",
               "n80_640x640_b64_h2@B64_swap1_best1+PLAIN", "n80_640x640_b512_h2@B512_swap1_best1+VTI_NO_BNECK=1+VTI_PK_LIMIT_BYTES=1099511627776"}


def _env_tag(env):
    return "+PLAIN" if env == PLAIN_PLAN else "".join(f"+{n}={v}" for n, v in sorted(env.items()))


def launch_cases():
    """[(id, argv, env)]: `launches` prints every launch of one forward (base, B, swap_rb, with / without best), `cfglaunch` the
    block vti_debug_conv2d would launch for a forced geometry."""
    out = []

    def add(base, B, swap_rb, best, env):
        cid = f"{base_id(*base)}@B{B}_swap{swap_rb}_best{best}{_env_tag(env)}"
        out.append((cid, ["launches"] + plan_argv(*base)[1:] + [str(B), str(swap_rb), str(best)], env))

    h2, fp16 = LAUNCH_BASES[0], LAUNCH_BASES[1]
    for base in LAUNCH_BASES:
        for B in sorted({base[4], 1}):
            add(base, B, 1, 1, {})
    for B in (64, 1):
        add(h2, B, 1, 1, dict(PLAIN_PLAN))
    for swap_rb, best in ((0, 1), (1, 0), (0, 0)):
        add(h2, 64, swap_rb, best, {})
    for env in LAUNCH_RUN_ENVS:
        add(h2, 64, 1, 1, env)
    for base in (h2, fp16):
        for env in LAUNCH_PLAN_ENVS:
            if not (base == h2 and env == PLAIN_PLAN):
                add(base, 64, 1, 1, env)
    for env in BIG_ENVS:
        add(BIG, 512, 1, 1, env)
    for cid, argv, env in cases():
        if argv[0] == "cfg":
            out.append((cid, ["cfglaunch"] + argv[1:], env))
    return out


def build_program(out_dir):
    """Compiles tests/plan_dump_main.cpp the way csrc/Makefile compiles plan.o and links it against the built libvti.so."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = os.path.join(str(out_dir), "plan_dump_main")
    lib_dir = os.path.dirname(CSRC)
    subprocess.run([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-x", "hip",
                    os.path.join(ROOT, "tests", "plan_dump_main.cpp"), "-L", lib_dir, "-lvti", "-Wl,-rpath," + lib_dir, "-o", exe],
                   check=True)
    return exe


def run(exe, argv, env):
    """The program's output under exactly the switches of `env`."""
    e = {k: v for k, v in os.environ.items() if k not in ALL_SWITCHES}
    e.update(env)
    r = subprocess.run([exe] + list(argv), env=e, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (argv, env, r.returncode, r.stderr[-2000:])
    return r.stdout
