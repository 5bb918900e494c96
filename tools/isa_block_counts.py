#!/usr/bin/env python3
"""Static instruction counts per basic block of one kernel of a device assembly file.

    hipcc <the Makefile's flags> -S --cuda-device-only orb_kernels.hip -o orb.s
    tools/isa_block_counts.py orb.s k_describe_tilesILb1E        # any substring of the mangled name

Prints, for every basic block (label) of the kernel, the number of vector (v_*), LDS (ds_*) and global-memory (global_*)
instructions, then the totals and the register / LDS figures of the kernel's metadata.  It only counts: which blocks run how
often is read off the source.
"""
import re
import sys


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    path, want = sys.argv[1], sys.argv[2]
    lines = open(path).read().splitlines()
    start = [i for i, l in enumerate(lines) if re.match(r"^[A-Za-z_$][\w$.]*:", l) and want in l and not l.startswith(".L")]
    if not start:
        sys.exit("no kernel label contains %r" % want)
    i = start[0]
    name = lines[i].split(":")[0]
    blocks, cur = [], [name, 0, 0, 0]
    for l in lines[i + 1:]:
        t = l.strip()
        if t.startswith(".Lfunc_end"):
            break
        m = re.match(r"^(\.LBB[\w$.]*):", t)
        if m:
            blocks.append(cur)
            cur = [m.group(1), 0, 0, 0]
            continue
        op = t.split()[0] if t and not t.startswith((";", ".", "//")) else ""
        if op.startswith("v_"):
            cur[1] += 1
        elif op.startswith("ds_"):
            cur[2] += 1
        elif op.startswith("global_"):
            cur[3] += 1
    blocks.append(cur)
    print("# %s" % name)
    print("%-14s %6s %6s %6s" % ("block", "v_", "ds_", "global_"))
    for b in blocks:
        if b[1] or b[2] or b[3]:
            print("%-14s %6d %6d %6d" % tuple(b))
    print("%-14s %6d %6d %6d" % ("total", sum(b[1] for b in blocks), sum(b[2] for b in blocks), sum(b[3] for b in blocks)))
    meta = re.search(r"\.amdhsa_kernel %s\b(.*?)\.end_amdhsa_kernel" % re.escape(name), "\n".join(lines), re.S)
    if meta:
        for key in ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size"):
            m = re.search(r"\.amdhsa_%s\s+(\S+)" % key, meta.group(1))
            if m:
                print("%s %s" % (key, m.group(1)))


if __name__ == "__main__":
    main()
