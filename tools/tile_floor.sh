#!/bin/bash
# tools/tile_floor.sh <outdir> [tag] [full-lib] -- ON the GPU box: SQ_INSTS_SALU / SQ_INSTS_VALU / SQ_INSTS_LDS per launch of k_resize2<true> (its
# launches told apart by grid size) and of k_describe_tiles<true>, and their durations, for the library (default: the in-tree build) and the
# ablation builds of tools/tile_ablate.sh (variants/libtile<tag>_{r1,r2,r3}.so) -> <outdir>/tile_floor_pmc<tag>.json (tools/tile_floor.py --pmc).
# The counter passes run alone (kernel filter on, no tracing beside them); the durations come from kernel-trace passes of their own.
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
O=${1:?usage: tools/tile_floor.sh <outdir> [tag] [full-lib]}; mkdir -p $O
TAG=${2:-}
FULL=${3:-$R/visual-slam_amd/libvslam_amd.so}
cd /tmp && export TMPDIR=/tmp
B="python3 $R/bench.py --steps 5 --warmup 2 --prewarm-ms 50 --no-cpu-baseline --no-optin --no-extras --no-check --frames-cache /tmp/bench_frames"
# one GPU step under its own time limit; any failing step ends the script (nothing more is started on a GPU that may have faulted)
step() {
  local rc=0
  timeout -k 10 240 "$@" > /dev/null || rc=$?
  if [ $rc != 0 ]; then echo "tile_floor.sh: step ended with status $rc, stopping: $*" >&2; exit $rc; fi
}
step $B 2> $O/bench_first.err   # (frames generated and cached outside the counter passes)
for v in full r1 r2 r3; do
  lib=$R/visual-slam_amd/variants/libtile${TAG}_$v.so; [ "$v" = full ] && lib=$FULL
  [ -f "$lib" ] || continue
  export VSLAM_AMD_LIB=$lib
  step rocprofv3 --pmc SQ_INSTS_SALU SQ_INSTS_VALU SQ_INSTS_LDS --kernel-include-regex 'k_resize2|k_describe_tiles' -d $O/pmc_$v -o p --output-format csv -- $B 2> $O/pmc_$v.err
  step rocprofv3 --kernel-trace --stats -d $O/st_$v -o s --output-format csv -- $B 2> $O/st_$v.err
done
unset VSLAM_AMD_LIB
python3 - $O "$TAG" <<'PY'
import csv, json, sys, collections, glob, os
O, TAG = sys.argv[1], sys.argv[2]
KERNELS = ("k_resize2<true>", "k_describe_tiles<true>")
out = {}
for v in ("full", "r1", "r2", "r3"):
    acc = collections.defaultdict(lambda: collections.defaultdict(list))   # kernel -> (grid size, counter) -> values
    for f in glob.glob(os.path.join(O, "pmc_" + v, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            for k in KERNELS:
                if k in r["Kernel_Name"]:
                    acc[k][(int(r["Grid_Size"]), r["Counter_Name"])].append(float(r["Counter_Value"]))
    dur = collections.defaultdict(lambda: collections.defaultdict(list))   # kernel -> grid size -> ns (trace), and the --stats average
    stats = {}
    for f in glob.glob(os.path.join(O, "st_" + v, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            for k in KERNELS:
                if k in r["Kernel_Name"]:
                    g = int(r["Grid_Size_X"]) * int(r["Grid_Size_Y"]) * int(r["Grid_Size_Z"]) if "Grid_Size_X" in r else int(r["Grid_Size"])
                    dur[k][g].append(float(r["End_Timestamp"]) - float(r["Start_Timestamp"]))
    for f in glob.glob(os.path.join(O, "st_" + v, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            for k in KERNELS:
                if k in r["Name"]:
                    stats[k] = {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3}
    if not acc and not stats:
        continue
    out[v] = {}
    for k in KERNELS:
        grids = sorted({g for g, _ in acc[k]}, reverse=True)
        med = lambda xs: sorted(xs)[len(xs) // 2] if xs else None
        out[v][k] = {"stats": stats.get(k),
                     "launches": [{"grid": g, "n": len(acc[k][(g, "SQ_INSTS_SALU")]), "salu": med(acc[k][(g, "SQ_INSTS_SALU")]),
                                   "valu": med(acc[k][(g, "SQ_INSTS_VALU")]), "lds": med(acc[k][(g, "SQ_INSTS_LDS")])} for g in grids],
                     "trace_us": [{"grid": g, "n": len(x), "median_us": med(x) / 1e3} for g, x in sorted(dur[k].items(), reverse=True)]}
json.dump(out, open(os.path.join(O, "tile_floor_pmc%s.json" % TAG), "w"), indent=1)
print(json.dumps(out, indent=1))
PY
for f in $O/st_full/*/*kernel_stats.csv $O/st_full/*kernel_stats.csv; do [ -f "$f" ] && cp "$f" $O/tile_kernel_stats${TAG}.csv; done
rm -rf $O/pmc_* $O/st_*
