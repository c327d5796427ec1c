#!/usr/bin/env python3
"""Per-kernel register counts and instruction mix from hipcc's device assembly.

    hipcc <csrc/Makefile's CXXFLAGS> --cuda-device-only -S csrc/conv_pk.hip -o conv_pk.s
    tools/kernel_resources.py conv_pk.s                 one line per kernel
    tools/kernel_resources.py parent.s new.s            only the kernels that differ (and names present on one side only)

Per kernel: the mangled name; vgpr_count, agpr_count, sgpr_count, vgpr_spill_count, sgpr_spill_count and
private_segment_fixed_size from the amdhsa.kernels metadata; the number of instructions in the kernel's body whose
mnemonic starts with v_mfma, ds_read, ds_write, buffer_load, buffer_store, s_barrier.  Reads compiler output only.
"""
import re
import sys

META = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")
PREFIXES = ("v_mfma", "ds_read", "ds_write", "buffer_load", "buffer_store", "s_barrier")
SHORT = ("vgpr", "agpr", "sgpr", "vspill", "sspill", "scratch", "mfma", "ds_rd", "ds_wr", "buf_ld", "buf_st", "barrier")


def parse(path):
    """{kernel name: tuple of the 12 figures, in META + PREFIXES order}"""
    records, counts = [], {}
    body = None                 # name of the function whose body is being read
    in_meta = False
    with open(path) as f:
        for line in f:
            s = line.strip()
            if s.startswith(".amdgpu_metadata"):
                in_meta, body = True, None
                continue
            if in_meta:
                if s.startswith(".end_amdgpu_metadata"):
                    in_meta = False
                # a kernel's own keys sit four columns in ("  - .key:" opens its record, "    .key:" continues it); its arguments' deeper
                m = re.match(r"^  ([- ]) \.(\w+):\s*(.*)$", line)
                if m:
                    if m.group(1) == "-":
                        records.append({})
                    records[-1][m.group(2)] = m.group(3).strip().strip("'\"")
                continue
            m = re.match(r"^([A-Za-z_$][\w$.]*):", line)
            if m and not m.group(1).startswith(".L"):
                body = m.group(1)
                counts[body] = [0] * len(PREFIXES)
                continue
            if s.startswith(".Lfunc_end") or s.startswith(".section") or s.startswith(".amdhsa_kernel"):
                body = None
                continue
            if body is None or not s or s[0] in ".;":
                continue
            mnem = s.split(None, 1)[0]
            for i, pre in enumerate(PREFIXES):
                if mnem.startswith(pre):
                    counts[body][i] += 1
    out = {}
    for rec in records:
        name = rec.get("name")
        if name is None or "vgpr_count" not in rec or name not in counts:
            continue
        out[name] = tuple(int(rec.get(k, 0)) for k in META) + tuple(counts[name])
    return out


def row(name, v):
    return name + "  " + " ".join("%s=%d" % (k, x) for k, x in zip(SHORT, v))


def main(argv):
    if len(argv) == 2:
        for name, v in sorted(parse(argv[1]).items()):
            print(row(name, v))
        return 0
    if len(argv) != 3:
        print(__doc__)
        return 2
    a, b = parse(argv[1]), parse(argv[2])
    for name in sorted(set(a) - set(b)):
        print("only in %s: %s" % (argv[1], name))
    for name in sorted(set(b) - set(a)):
        print("only in %s: %s" % (argv[2], name))
    ndiff = 0
    for name in sorted(set(a) & set(b)):
        if a[name] != b[name]:
            ndiff += 1
            print(name + "  " + " ".join("%s=%d->%d" % (k, x, y) for k, x, y in zip(SHORT, a[name], b[name]) if x != y))
    print("# %d kernels in %s, %d in %s, %d in both differ" % (len(a), argv[1], len(b), argv[2], ndiff))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
