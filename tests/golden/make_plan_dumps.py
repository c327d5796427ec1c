"""Records tests/golden/plan_dumps.json: what the host planner decides for every case of tests/plan_golden_cases.py, printed by
tests/plan_dump_main.cpp in a fresh process per case.  One line per case: the SHA-256 of its dump, num_launches, ws_bytes and
wpk_bytes, and for eight base cases a fingerprint per line of the dump.  Run it against a built libvti.so of the commit whose
plans are to be pinned:

    python tests/golden/make_plan_dumps.py
"""
import hashlib
import json
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plan_golden_cases as G      # noqa: E402


def summary(dump):
    out = {"sha256": hashlib.sha256(dump.encode()).hexdigest()}
    for key in ("num_launches", "ws_bytes", "wpk_bytes"):
        m = re.search(r"\b%s=(\d+)" % key, dump)
        if m:
            out[key] = int(m.group(1))
    return out


def main():
    with tempfile.TemporaryDirectory() as tmp:
        exe = G.build_program(tmp)
        golden = {}
        for cid, argv, env in G.cases():
            dump = G.run(exe, argv, env)
            golden[cid] = summary(dump)
            if cid in G.FULL:
                golden[cid]["lines"] = G.line_prints(dump)
    assert G.FULL <= set(golden), G.FULL - set(golden)
    with open(G.GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(golden[k], sort_keys=True)}" for k in sorted(golden)) + "\n}\n")
    print(len(golden), "cases,", os.path.getsize(G.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
