#!/usr/bin/env python3
"""Instruction mix per kernel of a `hipcc -S --cuda-device-only` listing: counts by class (MFMA, packed VALU, transcendental,
other VALU, LDS, VMEM, SALU) for kernels whose mangled name contains one of the given substrings.

    hipcc -O3 -std=c++20 --offload-arch=gfx950 -Iinclude -S --cuda-device-only -o /tmp/edge.s torch-m3gnet_amd/csrc/m3g_edge_mfma.hip
    python tools/asm_mix.py /tmp/edge.s rev_fusedILi3ELb1 edge_block_mfmaILi3ELb1

--signature prints, for every kernel of the listing (sorted by name), its register and memory footprint and the count of EVERY
mnemonic, then one line of totals: the text to `diff` between two builds of a unit whose source was only reshaped (a moved or
renamed register changes no line of it; profiles/device_idioms.txt).

    python tools/asm_mix.py --signature /tmp/node_mfma.s > node_mfma.sig
"""
import collections
import re
import sys


def classify(op):
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("v_pk_"):
        return "v_pk"
    if op.startswith(("v_exp", "v_rcp", "v_log", "v_sqrt", "v_rsq", "v_sin", "v_cos")):
        return "trans"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("s_"):
        return "salu"
    return "other"


FOOTPRINT = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size", "private_segment_fixed_size")


def signature(path):
    """kernel -> (mnemonic counts of its body, its .amdhsa_* footprint values); kernels = the names of the .amdhsa_kernel blocks"""
    lines = open(path).read().splitlines()
    foot, cur = {}, None
    for line in lines:
        t = line.split()
        if len(t) == 2 and t[0] == ".amdhsa_kernel":
            cur = foot[t[1]] = {}
        elif t and t[0] == ".end_amdhsa_kernel":
            cur = None
        elif cur is not None and len(t) == 2 and t[0].startswith(".amdhsa_") and t[0][8:] in FOOTPRINT:
            cur[t[0][8:]] = t[1]
    ops, name = {}, None
    for line in lines:
        m = re.match(r"^([A-Za-z_][\w.$]*):", line)
        if m and m.group(1) in foot:
            name = m.group(1)
            ops[name] = collections.Counter()
        elif line.startswith(".Lfunc_end"):
            name = None
        elif name:
            m = re.match(r"^\s+([a-z][a-z_0-9]+)(\s|$)", line)
            if m:
                ops[name][m.group(1)] += 1
    total = 0
    for k in sorted(foot):
        total += sum(ops[k].values())
        print(k)
        print("  ", " ".join(f"{f}={foot[k].get(f, '-')}" for f in FOOTPRINT))
        print("  ", " ".join(f"{op}={n}" for op, n in sorted(ops[k].items())))
    print(f"kernels {len(foot)} instructions {total}")


def main():
    if sys.argv[1] == "--signature":
        return signature(sys.argv[2])
    path, pats = sys.argv[1], sys.argv[2:]
    name, ops = None, None
    out = []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            if name:
                out.append((name, ops))
            name, ops = m.group(1), collections.Counter()
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            out.append((name, ops))
            name = None
            continue
        m = re.match(r"^\s+([a-z][a-z_0-9]+)\s", line)
        if m:
            ops[m.group(1)] += 1
    for name, ops in out:
        if pats and not any(p in name for p in pats):
            continue
        cls = collections.Counter()
        for k, v in ops.items():
            cls[classify(k)] += v
        print(name[:90], "total", sum(ops.values()))
        print("  ", dict(cls))
        print("  ", [(k, v) for k, v in ops.most_common(28)])


if __name__ == "__main__":
    main()
