"""The device covisibility matrix, the local-keyframe selection and tracking against the covisible local map, on the maps of
tools/track_map_rate.py (16 and 64 keyframes of 2000 rows, 10^5 and 10^6 points with two observations each).

Per (keyframes, map points), medians over the warm calls of the device time of
  covis          k_covis inside LocalMapper.local_keyframes (the stage event "covis")
  covis_select   k_covis_select (the stage event "covis_select")
  track_cov      LocalMapper.track_local_map(local="covisible"), all its stages, seeded with the points the frame sees
  track_all      LocalMapper.track_local_map(window=0) on the same map and frame, all its stages; its "track_prep" stage is
                 k_trk_init + k_trk_rep + k_trk_grid: what k_covis, which streams the same observation lists once, is compared with
python tools/covis_rate.py [--out profiles/covis_rate.txt]   (one MI355X)
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "visual-slam_amd"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402

import vslam_amd as V  # noqa: E402
from track_map_rate import ROWS, build  # noqa: E402


def _stages(ctx):
    agg = {}
    for name, ms in ctx.stage_times():
        agg[name] = agg.get(name, 0.0) + ms
    return agg


def _median(runs):
    return {k: float(np.median([r.get(k, 0.0) for r in runs])) for k in runs[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", default="16,64")
    ap.add_argument("--points", default="100000,1000000")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "covis_rate.txt"))
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    ctx = V.Context(device=0, max_w=640, max_h=480, max_batch=1)
    ctx.set_host_timing(True)
    lines = []
    for n_kf in [int(x) for x in args.keyframes.split(",")]:
        for n_pts in [int(x) for x in args.points.split(",")]:
            m, qk, qd, pose0 = build(ctx, n_kf, n_pts, rng)
            seeds = np.arange(ROWS, dtype=np.int32)
            sel, cov, win = [], [], []
            for i in range(args.calls + 1):   # (the first call of each sizes its buffers: dropped)
                lk = m.local_keyframes(seed_points=seeds)
                sel.append(_stages(ctx))
                ok_c, _, ic = m.track_local_map(qk, qd, pose0, local="covisible", seed_points=seeds)
                cov.append(_stages(ctx))
                ok_w, _, iw = m.track_local_map(qk, qd, pose0, window=0)
                win.append(_stages(ctx))
            sel, cov, win = _median(sel[1:]), _median(cov[1:]), _median(win[1:])
            W = m.covisibility()
            line = ("keyframes %3d  rows %d  map_points %8d  covis %.3f ms  covis_select %.3f ms  local keyframes %d (K1 %d)  |  "
                    "track_cov %.3f ms (local %d, ok %s, inliers %s: %s)  |  track_all window 0 %.3f ms (local %d, ok %s, inliers %s: %s)  |  "
                    "W trace %d"
                    % (n_kf, ROWS, n_pts, sel["covis"], sel["covis_select"], len(lk["local"]), len(lk["k1"]), sum(cov.values()), ic["n_local"], ok_c,
                       ic["pass_inliers"], "  ".join("%s %.3f" % kv for kv in cov.items()), sum(win.values()), iw["n_local"], ok_w,
                       iw["pass_inliers"], "  ".join("%s %.3f" % kv for kv in win.items()), int(W.trace())))
            print(line, flush=True)
            lines.append(line)
            m.close()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
