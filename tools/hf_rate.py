"""Two-view initialisation with model selection (mo_init_two_view_hf) next to the essential path alone (mo_init_two_view, whose
kernels this call launches unchanged): device time of the call and of its two stages, "two_view" (the essential chain) and
"two_view_h" (the homography chain: k_h_prep, k_h_hyp, k_h_score, k_h_finish), from the stage marks, warm, median of repeated calls.

Scene: the tilted exact plane of tests/hf_cases.py (0.5 px noise, 30 % outliers) at m = 500 / 2000 / 4096 correspondences - the case
the homography chain works hardest on (every inlier goes through eight CheckRT passes) - and a general scene (depth 4 .. 12) at the
same sizes, where it has few inliers.  n_hyp = 4096, n_hyp_h = 512 / 2048.
python tools/hf_rate.py   (one MI355X)
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "visual-slam_amd")]

import numpy as np  # noqa: E402

import vslam_amd as V  # noqa: E402
from oracle import geom_oracle as G  # noqa: E402


def medians(ctx, call, n):
    """per-stage device medians (ms), the median of their sum and the wall median (ms) of n warm calls"""
    call(); call()
    wall, dev, stages = [], [], []
    for _ in range(n):
        t0 = time.perf_counter()
        res = call()
        wall.append(time.perf_counter() - t0)
        st = ctx.stage_times()
        dev.append(sum(ms for _, ms in st))
        stages.append(dict(st))
    return {k: float(np.median([s[k] for s in stages])) for k in stages[0]}, float(np.median(dev)), 1e3 * float(np.median(wall)), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="500,2000,4096")
    ap.add_argument("--n-hyp", type=int, default=4096)
    ap.add_argument("--n-hyp-h", default="512,2048")
    ap.add_argument("--repeat", type=int, default=30)
    args = ap.parse_args()
    ctx = V.Context(device=0, max_w=640, max_h=480, max_batch=1)
    scenes = {"plane": dict(depth=(0, 0), plane=(0.3, 0.2, 1.0, 8.0, 0.0)), "general": dict(depth=(4, 12))}
    for sname, kw in scenes.items():
        for m in [int(x) for x in args.sizes.split(",")]:
            s = G.synthetic_two_view(seed=4096, n=m, noise_px=0.5, outlier_frac=0.3, **kw)
            st_e, dev_e, wall_e, _ = medians(ctx, lambda: ctx.init_two_view(s["p1"], s["p2"], s["K"], n_hyp=args.n_hyp), args.repeat)
            for nh in [int(x) for x in args.n_hyp_h.split(",")]:
                st, dev, wall, g = medians(ctx, lambda: ctx.init_two_view_hf(s["p1"], s["p2"], s["K"], n_hyp=args.n_hyp, n_hyp_h=nh), args.repeat)
                print("%-7s m %4d  n_hyp %d  n_hyp_h %4d  init_two_view_hf: device %.3f ms (two_view %.3f + two_view_h %.3f: H chain %.0f %% of the call)  "
                      "wall %.3f ms | init_two_view: device %.3f ms  wall %.3f ms | model %d RH %.3f H inliers %d refits %d"
                      % (sname, m, args.n_hyp, nh, dev, st["two_view"], st["two_view_h"], 100.0 * st["two_view_h"] / dev, wall, dev_e, wall_e,
                         g["model"], g["RH"], g["n_inliers_h"], g["refits_h"]), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
