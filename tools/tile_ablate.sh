#!/bin/bash
# tools/tile_ablate.sh [tag]: timing-only variants of the blurring k_resize2 that return after a phase (their pyramids are garbage, every
# index downstream stays valid; never shipped; bench.py --no-check):
#   r1 = after the prologue + staging, r2 = after the resize, r3 = after the blur row pass
# built from the working tree into visual-slam_amd/variants/libtile<tag>_{r1,r2,r3}.so.
# (k_describe_tiles has no such builds: returning in front of phase A leaves the keypoint records unwritten, and the stages behind it index by them.)
set -e
tag=${1:-}
root=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$root/visual-slam_amd/variants"
for v in r1 r2 r3; do
  tmp=$(mktemp -d /tmp/abl.XXXX)
  mkdir -p "$tmp/visual-slam_amd" "$tmp/include"
  cp -r "$root/visual-slam_amd/csrc" "$tmp/visual-slam_amd/"; cp "$root/include/vslam_amd.h" "$tmp/include/"
  rm -rf "$tmp/visual-slam_amd/csrc/_obj"
  python3 - "$tmp/visual-slam_amd/csrc/orb_kernels.hip" "$v" <<'PY'
import sys
f, v = sys.argv[1], sys.argv[2]
s = open(f).read()
anchor = {"r1": "        {  // resize straight from the window: both source rows of an output row along x, then along y\n",
          "r2": "        const uint32_t g0 = bo.taps & 255u, g1 = (bo.taps >> 8) & 255u, g2 = (bo.taps >> 16) & 255u, g3 = bo.taps >> 24;\n",
          "r3": "        {  // blur column pass\n"}[v]
assert s.count(anchor) == 1, v
s = s.replace(anchor, "        if (dw > 0) return;\n" + anchor, 1)   # (a kernel argument: the compiler keeps the code in front)
open(f, "w").write(s)
PY
  make -C "$tmp/visual-slam_amd/csrc" -j8 > "$tmp/make.log" 2>&1 || { grep -E "error" -A3 "$tmp/make.log" | head -20; echo "tile_ablate.sh: the build of $v failed" >&2; exit 1; }
  cp "$tmp/visual-slam_amd/libvslam_amd.so" "$root/visual-slam_amd/variants/libtile${tag}_$v.so"
  rm -rf "$tmp"; echo built "libtile${tag}_$v.so"
done
