"""Records tests/golden/launch_params.json: every launch of one forward (launcher, selector arguments, every field of the block) for
the cases of tests/plan_golden_cases.py: launch_cases(), one fresh process each.  One line per case: the SHA-256 of its dump, the
number of launches, whether it ends in a refusal, and for a few cases a fingerprint per line.

The `launches` cases were recorded from the commit BEFORE csrc/launch.cpp existed, whose forward_impl filled the blocks inline: its
launch_* calls were made to print their arguments by tests/golden/launch_params_recorder.patch (see its head), which builds a
recorder program that takes the same arguments as `plan_dump_main launches`:

    python tests/golden/make_launch_params.py --recorder /path/to/launch_record_main

The `cfglaunch` cases (the block vti_debug_conv2d launches) cannot be recorded that way, because vti_debug_conv2d allocates device
memory before it fills the block; they are recorded from csrc/launch.cpp itself (tests/test_gpu_conv.py and
tests/test_gpu_conv1x1_wreg.py check those launches on the device).  Without --recorder everything is recorded from the built
libvti.so; with --keep-launches the recorded `launches` cases are kept and only the `cfglaunch` ones are written anew."""
import hashlib
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plan_golden_cases as G      # noqa: E402


def summary(cid, dump):
    lines = dump.splitlines()
    out = {"sha256": hashlib.sha256(dump.encode()).hexdigest(), "launches": sum(": launch_" in l for l in lines),
           "refused": int(any(": refused (" in l for l in lines))}
    if cid in G.LAUNCH_FULL:
        out["lines"] = G.line_prints(dump)
    return out


def main():
    recorder = sys.argv[sys.argv.index("--recorder") + 1] if "--recorder" in sys.argv else None
    golden = {}
    if "--keep-launches" in sys.argv:
        with open(G.LAUNCH_GOLDEN) as f:
            golden = {k: v for k, v in json.load(f).items() if not k.startswith("cfg_")}
    with tempfile.TemporaryDirectory() as tmp:
        exe = None
        for cid, argv, env in G.launch_cases():
            if cid in golden:
                continue
            if argv[0] == "launches" and recorder:
                golden[cid] = summary(cid, G.run(recorder, argv, env))
            else:
                exe = exe or G.build_program(tmp)
                golden[cid] = summary(cid, G.run(exe, argv, env))
    assert G.LAUNCH_FULL <= set(golden), G.LAUNCH_FULL - set(golden)
    with open(G.LAUNCH_GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(golden[k], sort_keys=True)}" for k in sorted(golden)) + "\n}\n")
    print(len(golden), "cases,", os.path.getsize(G.LAUNCH_GOLDEN), "bytes")


if __name__ == "__main__":
    main()
