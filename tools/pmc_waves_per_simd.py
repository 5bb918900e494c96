"""tools/pmc_waves_per_simd.py <dir> [kernel-regex]: resident wavefronts per SIMD of each kernel from one counters-only
`rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU ... --output-format csv -d <dir>` pass.

SQ_WAVE_CYCLES counts quad-cycles summed over the wavefronts, SQ_BUSY_CYCLES is summed over the 32 shader engines, so
waves per SIMD = SQ_WAVE_CYCLES x 4 / (SQ_BUSY_CYCLES / 32 x 1024 SIMDs) (profiles/r04_pmc_per_kernel.json, NOTES.md).
One line per kernel and grid size: launches and the per-launch means."""
import collections
import csv
import os
import re
import sys

root = sys.argv[1]
pat = re.compile(sys.argv[2] if len(sys.argv) > 2 else "k_")
acc = collections.defaultdict(lambda: collections.defaultdict(list))
for d, _, files in os.walk(root):
    for f in files:
        if f.endswith("counter_collection.csv"):
            for r in csv.DictReader(open(os.path.join(d, f))):
                name = re.sub(r"\(.*", "", r["Kernel_Name"]).replace("void ", "")
                if pat.search(name):
                    acc[(name, r["Grid_Size"])][r["Counter_Name"]].append(float(r["Counter_Value"]))
for (name, grid), c in sorted(acc.items()):
    m = {k: sum(v) / len(v) for k, v in c.items()}
    wps = m["SQ_WAVE_CYCLES"] * 4 / (m["SQ_BUSY_CYCLES"] / 32 * 1024) if m.get("SQ_BUSY_CYCLES") else float("nan")
    print("%-28s grid %-9s launches %3d  SQ_WAVE_CYCLES %.4g  SQ_BUSY_CYCLES %.4g  SQ_INSTS_VALU %.4g  waves per SIMD %.2f"
          % (name, grid, len(c["SQ_WAVE_CYCLES"]), m.get("SQ_WAVE_CYCLES", 0), m.get("SQ_BUSY_CYCLES", 0), m.get("SQ_INSTS_VALU", 0), wps))
