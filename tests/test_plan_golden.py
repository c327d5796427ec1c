"""The host planner, pinned byte for byte (host only: Plan::build touches no GPU).

tests/golden/plan_dumps.json holds what tests/plan_dump_main.cpp printed for every case of tests/plan_golden_cases.py when the
planner still read its switches with getenv where it used them -- a fresh process per case, because a third of the switches were
function-local statics then.  The replay asks for the same bytes from the planner as a function of (vti_desc, PlanOptions):
every base canvas, every refusal, every planner switch alone at each non-default value (parse oddities included) and the forced
geometries that tests/test_gpu_conv.py and tests/test_gpu_conv1x1_wreg.py pass to debug_conv2d."""
import glob
import hashlib
import json
import os
import re

import pytest

import plan_golden_cases as G


@pytest.fixture(scope="module")
def exe(lib_built, tmp_path_factory):
    return G.build_program(tmp_path_factory.mktemp("plan_dump"))


@pytest.fixture(scope="module")
def golden():
    with open(G.GOLDEN) as f:
        return json.load(f)


def _sha(dump):
    return hashlib.sha256(dump.encode()).hexdigest()


def _first_difference(want, got):
    want, got = want.splitlines(), got.splitlines()
    for i in range(max(len(want), len(got))):
        w, g = (want[i] if i < len(want) else "<end>"), (got[i] if i < len(got) else "<end>")
        if w != g:
            return f"line {i + 1}:\n  first:  {w}\n  second: {g}"
    return "no difference"


def _first_changed_line(prints, dump):
    """The first line of `dump` whose fingerprint is not the recorded one."""
    now, lines = G.line_prints(dump), dump.splitlines()
    for i in range(max(len(prints), len(now)) // 4):
        if prints[4 * i:4 * i + 4] != now[4 * i:4 * i + 4]:
            return f"first differing line {i + 1} of {len(prints) // 4} recorded; now: {lines[i] if i < len(lines) else '<end>'}"
    return "a line differs that its 16-bit fingerprint does not tell apart"


def test_every_recorded_plan_is_replayed_byte_for_byte(exe, golden):
    cases = G.cases()
    assert {c[0] for c in cases} == set(golden) and G.FULL <= set(golden)
    bad = []
    for cid, argv, env in cases:
        want = golden[cid]
        dump = G.run(exe, argv, env)
        if _sha(dump) != want["sha256"]:
            got = {k: int(m.group(1)) for k in ("num_launches", "ws_bytes", "wpk_bytes") for m in [re.search(r"\b%s=(\d+)" % k, dump)] if m}
            bad.append(f"{cid}: SHA-256 differs; golden {({k: want[k] for k in got})}, now {got}" +
                       ("; " + _first_changed_line(want["lines"], dump) if "lines" in want else ""))
    assert not bad, f"{len(bad)} of {len(cases)} plans differ:\n" + "\n".join(bad[:20])


def test_every_recorded_forward_is_replayed_launch_for_launch(exe):
    """The launch parameters (csrc/launch.cpp), pinned the same way: tests/golden/launch_params.json holds what the forward launched
    -- launcher, selector arguments and every field of each block, the tensors at fake addresses -- when forward_impl still filled
    the blocks inline (recorded from that commit: tests/golden/make_launch_params.py).  The cases: every base at max_batch and at
    one frame, swap_rb and the anchor pairs on and off, the switches of the launch path, each planner switch that steers the loop
    into another branch, tensors past 2^31 bytes (persistent kernels falling back, two refusals), and the block of every forced
    geometry of vti_debug_conv2d.  Between them they reach every launcher."""
    with open(G.LAUNCH_GOLDEN) as f:
        golden = json.load(f)
    cases = G.launch_cases()
    assert {c[0] for c in cases} == set(golden) and G.LAUNCH_FULL <= set(golden)
    bad, launchers, refusals = [], set(), set()
    for cid, argv, env in cases:
        want = golden[cid]
        dump = G.run(exe, argv, env)
        launchers |= set(re.findall(r": (launch_\w+) ", dump))
        refusals |= set(re.findall(r": refused \(status -?\d+\): (.*)", dump))
        if _sha(dump) != want["sha256"]:
            got = {"launches": dump.count(": launch_"), "refused": int(": refused (" in dump)}
            bad.append(f"{cid}: SHA-256 differs; golden {({k: want[k] for k in got})}, now {got}" +
                       ("; " + _first_changed_line(want["lines"], dump) if "lines" in want else ""))
    assert not bad, f"{len(bad)} of {len(cases)} forwards differ:\n" + "\n".join(bad[:20])
    assert launchers == {"launch_stem_l1", "launch_conv", "launch_convfold", "launch_conv_pk_fold", "launch_sppf_pool", "launch_upsample2x",
                         "launch_decode", "launch_box_decode", "launch_anchor_best"}, launchers
    assert refusals == {"fused bottleneck needs the persistent kernel (tensor too large?)",
                        "folded upsample needs the persistent 1x1 kernel (tensor too large?)"}, refusals


BASE_H2 = ("n", 80, 640, 640, 64, "h2")
BASE_F32 = ("n", 80, 640, 640, 64, "fp32")
DIRECT = [   # base, the switch in the environment, the same option filled into PlanOptions directly
    (BASE_H2, {}, ["pk_depth=2"]),
    (BASE_H2, {"VTI_NO_FUSE": "1"}, ["no_fuse=1"]),
    (BASE_H2, {"VTI_P3_LANES": "1"}, ["p3_lanes=1"]),
    (BASE_H2, {"VTI_PK_DEPTH": "9"}, ["pk_depth=4"]),
    (BASE_H2, {"VTI_PK_FUSED": "2"}, ["pk_fused=2"]),
    (BASE_H2, {"VTI_PK_LIMIT_BYTES": "1000000"}, ["pk_limit_bytes=1000000"]),
    (BASE_H2, {"VTI_CONV1_WREG": "0"}, ["conv1_wreg=0"]),
    (BASE_H2, {"VTI_FOLD512": "0"}, ["fold512=0"]),
    (BASE_F32, {"VTI_PK1_NO_WGPC2": "1"}, ["pk1_no_wgpc2=1"]),
]


@pytest.mark.parametrize("base,env,members", DIRECT, ids=lambda v: "+".join(v) if isinstance(v, list) else None)
def test_options_from_the_environment_and_filled_in_directly_give_the_same_plan(exe, golden, base, env, members):
    """The planner is a function of its arguments: the environment is only one way to fill them."""
    from_env = G.run(exe, G.plan_argv(*base), env)
    poison = {n: "1" for n in G.ON_SWITCHES}        # --set does not read the environment, whatever it holds
    direct = G.run(exe, G.plan_argv(*base) + [a for m in members for a in ("--set", m)], poison)
    assert direct == from_env, _first_difference(from_env, direct)
    cid = G.base_id(*base) + "".join(f"+{k}={v}" for k, v in env.items())
    assert _sha(direct) == golden[cid]["sha256"]


@pytest.mark.parametrize("base,switch", [(BASE_H2, "VTI_P3_LANES"), (BASE_F32, "VTI_PK1_NO_WGPC2")])
def test_two_plans_of_one_process_follow_a_formerly_static_switch(exe, golden, base, switch):
    """These switches were read once per process; now two plans built in one process under two settings differ exactly as the
    two fresh-process goldens do."""
    off, on = golden[G.base_id(*base)], golden[G.base_id(*base) + f"+{switch}=1"]
    assert off["sha256"] != on["sha256"]
    for a, b in (("-", "1"), ("1", "-")):
        out = G.run(exe, ["twice", switch, a, b] + G.plan_argv(*base)[1:], {})
        first, second = out.split("==== second plan\n")
        assert _sha(first) == (on if a == "1" else off)["sha256"] and _sha(second) == (on if b == "1" else off)["sha256"]


def test_the_launch_switches_keep_their_parse_rules(exe):
    """What the launch path did with the text of its switches, written out by hand from those rules: VTI_PK_MAX_WGS and
    VTI_MASK_WGS_PER_CU are atoi floored at 1 (0 here: no cap), VTI_PK_STAGGER is clamped to 0..255 (-1 here: the dtype's default),
    VTI_LIST_OPS is on when set at all, the others when their first character is '1'."""
    def opts(env):
        return dict(kv.split("=", 1) for kv in G.run(exe, ["runopts"], env).split())
    off = "pk_max_wgs=0 pk_stagger=-1 pk_linear_map=0 single_stream=0 list_ops=0 stem_not_persistent=0 mask_wgs_per_cu=0 stamp_op=\n"
    assert G.run(exe, ["runopts"], {}) == off
    for text, want in (("8", "8"), ("0", "1"), ("-3", "1"), ("12abc", "12"), ("abc", "1")):
        assert opts({"VTI_PK_MAX_WGS": text})["pk_max_wgs"] == want and opts({"VTI_MASK_WGS_PER_CU": text})["mask_wgs_per_cu"] == want
    for text, want in (("10", "10"), ("0", "0"), ("300", "255"), ("-5", "0")):
        assert opts({"VTI_PK_STAGGER": text})["pk_stagger"] == want
    assert opts({"VTI_LIST_OPS": ""})["list_ops"] == "1" and opts({"VTI_LIST_OPS": "0"})["list_ops"] == "1"
    for name, key in (("VTI_PK_LINEAR_MAP", "pk_linear_map"), ("VTI_SINGLE_STREAM", "single_stream"), ("VTI_STEM_NOT_PERSISTENT", "stem_not_persistent")):
        assert [opts({name: t})[key] for t in ("1", "10", "true", "0")] == ["1", "1", "0", "0"]
    assert opts({"VTI_STAMP_OP": "model.3"})["stamp_op"] == "model.3"


def test_the_environment_is_read_in_one_file_and_every_switch_is_documented():
    """getenv lives in one translation unit under csrc/ (none of it in a .hip file), and DESIGN.md's table lists every switch
    that file names."""
    sources = [p for p in sorted(glob.glob(os.path.join(G.CSRC, "*"))) if p.endswith((".cpp", ".hip", ".h"))]
    assert len(sources) > 20
    users = [os.path.basename(p) for p in sources if "getenv(" in open(p).read()]
    assert users == ["options.cpp"], users
    names = set(re.findall(r'"(VTI_[A-Z0-9_]+)"', open(os.path.join(G.CSRC, "options.cpp")).read()))
    assert names == set(G.ALL_SWITCHES), names ^ set(G.ALL_SWITCHES)
    design = open(os.path.join(G.ROOT, "DESIGN.md")).read()
    table = design[design.index("Environment switches\n"):]
    missing = sorted(n for n in names if f"| `{n}` |" not in table)
    assert not missing, missing
