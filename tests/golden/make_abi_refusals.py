"""Records tests/golden/abi_refusals.json: what one commit's library answers to every case of tests/abi_refusal_cases.py.

    python tests/golden/make_abi_refusals.py TREE COMMIT

TREE is a checkout of COMMIT (the parent of the change whose refusals must not move) in which libvti.so has been built; its package
is the one imported, so the record is that commit's, whatever the working tree holds.  Every case must be refused with VTI_ERR_ARG or
VTI_ERR_UNSUPPORTED (the size queries, vti_*_scratch_bytes and vti_mask_native_*_bytes: with 0), else nothing is written."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def main(tree, commit):
    sys.path[:0] = [os.path.abspath(tree), os.path.dirname(HERE)]
    import vti_amd
    assert os.path.realpath(vti_amd.LIB_PATH).startswith(os.path.realpath(tree) + os.sep), vti_amd.LIB_PATH
    from abi_refusal_cases import cases
    rows, seen = [], set()
    for entry, case, call in cases(vti_amd):
        status, message = call()
        assert (entry, case) not in seen, (entry, case)
        seen.add((entry, case))
        query = entry.endswith("_scratch_bytes") or entry in ("vti_mask_native_frames_bytes", "vti_mask_native_windows_bytes")
        assert status in ((0,) if query else (-1, -6)), (entry, case, status, message)
        rows.append([entry, case, status, message])
    with open(os.path.join(HERE, "abi_refusals.json"), "w") as f:
        f.write('{"commit": %s, "rows": [\n%s\n]}\n' % (json.dumps(commit), ",\n".join(json.dumps(row) for row in rows)))      # a row per line
    print(f"{len(rows)} refusals of {len({r[0] for r in rows})} entry points recorded at {commit}")


if __name__ == "__main__":
    main(*sys.argv[1:3])
