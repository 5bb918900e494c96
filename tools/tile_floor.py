#!/usr/bin/env python3
"""tools/tile_floor.py -- three-pipe issue floor per phase of the blurring k_resize2 (k_resize2<true>), the way tools/fast_floor.py does it for k_fast.

Step 1 (here, no GPU): compile csrc/orb_kernels.hip to gfx950 assembly with the library's flags, cut out k_resize2<true>, split it at its two
barriers into [prologue + staging | resize + blur row pass | blur column pass] and histogram each part's instructions by issue class
(tools/fast_floor.py: fast 2.26 / slow 4.5 cycles per vector instruction per SIMD, 4.28 per scalar-ALU instruction per SIMD, >= 2 cycles of a
CU's LDS pipe per ds_* instruction).  The resize and the row pass share a part: both are priced with its mix.
Step 2 (tools/tile_floor.sh on the GPU box): SQ_INSTS_SALU / SQ_INSTS_VALU / SQ_INSTS_LDS and the duration of every launch of the kernel (its seven
launches told apart by grid size, summed here) for the full kernel and the ablation builds of tools/tile_ablate.sh (r1 = returns after the
staging, r2 = after the resize, r3 = after the row pass): differences of builds = dynamic counts per phase.
Step 3 (--pmc <json>): per phase, vector / LDS / scalar floor in ms per step of 256 frames and the measured time of the phase; the scalar
term stands beside the other two (scalar and vector instructions of different waves issue side by side: profiles/scalar_ubench.txt), a phase's
floor is the largest of the three.  k_describe_tiles<true> is reported whole (no ablation builds: tools/tile_ablate.sh says why).
"""
import argparse
import collections
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fast_floor import C_FAST, C_SLOW, C_SALU, CLOCK, SIMDS, CUS, assembly, classify, kernel_blocks  # noqa: E402

KERNEL = "_Z9k_resize2ILb1EE"
PARTS = ["1 prologue + staging", "2 resize + row pass", "3 column pass"]


def static_parts(src):
    """class histogram of the kernel's instructions before the first barrier, between the two, behind the second; the scalar loads and the
    scalar-load waits (s_waitcnt lgkmcnt(0) behind an s_load) in front of the first global load"""
    blocks = kernel_blocks(assembly(src), KERNEL)
    parts, k = [collections.Counter() for _ in PARTS], 0
    sloads = waits = 0
    pending = seen_global = False
    for b in blocks:
        for ins in b["ins"]:
            if ins.startswith("s_barrier"):
                k = min(k + 1, len(PARTS) - 1)
            m = ins.split()[0]
            parts[k]["sload" if m.startswith(("s_load", "s_buffer_load")) else classify(ins)] += 1
            if not seen_global:
                if m.startswith("s_load"):
                    sloads += 1; pending = True
                elif m.startswith("s_waitcnt") and "lgkmcnt(0)" in ins and pending:
                    waits += 1; pending = False
                elif m.startswith("global_load"):
                    seen_global = True
    return parts, sloads, waits


def summed(pmc, build):
    """the seven launches of a step summed (a grid size that two levels share counts twice: its n is twice the others')"""
    k = pmc[build]["k_resize2<true>"]
    n1 = min(l["n"] for l in k["launches"])
    us = {t["grid"]: t["median_us"] for t in k["trace_us"]}
    tot = collections.Counter()
    for l in k["launches"]:
        mult = round(l["n"] / n1)
        for c in ("salu", "valu", "lds"):
            tot[c] += mult * l[c]
        tot["ms"] += mult * us[l["grid"]] / 1e3
        tot["launches"] += mult
    return tot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pmc", default="", help="JSON of tools/tile_floor.sh")
    ap.add_argument("--out", default="")
    ap.add_argument("--src", default="", help="another version of csrc/orb_kernels.hip to take the static counts from (compiled against the tree's headers)")
    args = ap.parse_args()
    out = []
    parts, sloads, waits = static_parts(args.src)
    out.append("k_resize2<true>, static counts per part (split at the two barriers):")
    out.append("  %-22s %6s %6s %6s %6s %6s %6s %6s | %s" % ("part", "fast", "slow", "lds", "vmem", "salu", "sload", "snop", "cycles per vector instruction"))
    cost = []
    for name, h in zip(PARTS, parts):
        v = max(h["fast"] + h["slow"], 1)
        cost.append((h["fast"] * C_FAST + h["slow"] * C_SLOW) / v)
        out.append("  %-22s %6d %6d %6d %6d %6d %6d %6d | %.2f" % (name, h["fast"], h["slow"], h["lds"], h["vmem"], h["salu"], h["sload"], h["snop"], cost[-1]))
    tot = sum(parts, collections.Counter())
    out.append("  %-22s %6d %6d %6d %6d %6d %6d %6d" % ("total", tot["fast"], tot["slow"], tot["lds"], tot["vmem"], tot["salu"], tot["sload"], tot["snop"]))
    out.append("  in front of the first global load: %d scalar loads, %d waits for them (dependent scalar round trips)" % (sloads, waits))
    if args.pmc:
        p = json.load(open(args.pmc))
        b = {v: summed(p, v) for v in ("r1", "r2", "r3", "full") if v in p}
        order = [("prologue + staging", None, "r1", cost[0]), ("resize", "r1", "r2", cost[1]), ("blur row pass", "r2", "r3", cost[1]), ("blur column pass", "r3", "full", cost[2])]
        out.append("")
        out.append("dynamic counts per step (256 frames, %d launches; differences of the ablation builds = phases) and the issue floors in ms:" % b["full"]["launches"])
        out.append("  %-20s %11s %11s %11s %9s | %8s %8s %8s %8s" % ("phase", "SALU", "VALU", "LDS", "build ms", "scalar", "vector", "LDS", "largest"))
        sums = collections.Counter()
        for name, lo, hi, cv in order:
            d = {c: b[hi][c] - (b[lo][c] if lo else 0.0) for c in ("salu", "valu", "lds", "ms")}
            fs, fv, fl = d["salu"] * C_SALU / SIMDS / CLOCK * 1e3, d["valu"] * cv / SIMDS / CLOCK * 1e3, d["lds"] * 2.0 / CUS / CLOCK * 1e3
            sums.update({"s": fs, "v": fv, "l": fl, "m": max(fs, fv, fl)})
            out.append("  %-20s %11.4g %11.4g %11.4g %9.4f | %8.4f %8.4f %8.4f %8.4f" % (name, d["salu"], d["valu"], d["lds"], d["ms"], fs, fv, fl, max(fs, fv, fl)))
        f = b["full"]
        out.append("  %-20s %11.4g %11.4g %11.4g %9.4f | %8.4f %8.4f %8.4f %8.4f" % ("total", f["salu"], f["valu"], f["lds"], f["ms"], sums["s"], sums["v"], sums["l"], sums["m"]))
        waves = sum(l["grid"] // 64 * round(l["n"] / min(x["n"] for x in p["full"]["k_resize2<true>"]["launches"])) for l in p["full"]["k_resize2<true>"]["launches"])
        out.append("  per wavefront (%d per step): %.0f scalar-ALU, %.0f vector instructions; in the prologue + staging build %.0f and %.0f"
                   % (waves, f["salu"] / waves, f["valu"] / waves, b["r1"]["salu"] / waves, b["r1"]["valu"] / waves))
        out.append("  (build ms: medians of the launches' durations in a kernel trace, summed over the step's launches; every launch carries its own ramp and tail)")
        d = p["full"]["k_describe_tiles<true>"]["launches"][0]
        st = p["full"]["k_describe_tiles<true>"]["stats"]
        out.append("")
        out.append("k_describe_tiles<true>, whole kernel per launch: SALU %.4g VALU %.4g LDS %.4g, %.4f ms; scalar term %.4f ms, LDS term %.4f ms"
                   % (d["salu"], d["valu"], d["lds"], st["avg_us"] / 1e3, d["salu"] * C_SALU / SIMDS / CLOCK * 1e3, d["lds"] * 2.0 / CUS / CLOCK * 1e3))
    text = "\n".join(out)
    print(text)
    if args.out:
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
