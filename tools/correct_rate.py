"""Loop correction (mo_map_loop_correct) against the size of the map, next to the fusion it is built from: the stages of the call with a
corrected set of 10 keyframes of 2000 rows and a group of 10, on maps of 10^5 and 10^6 points, and fuse_map_points(window=10) on the same
map in the same process as the yardstick.

The map of tools/bow_rate.py at 50 keyframes (2000-row keyframes whose row r holds the projection of point r under the keyframe's pose;
point i is observed from keyframes (i // 2000) % 50 and the next, at row i % 2000: at 10^5 points every keyframe starts 2000 of them,
so the yardstick's ten target keyframes see 22000 points, as many as the group).  The asking keyframe is 10, the corrected set the
positions 5 .. 14, the group the positions 30 .. 39: its loop points are the points of the keyframes 29 .. 39 (22000 of 10^5).  loop_point names,
for every row r of the asking keyframe, the group's point 30 * 2000 + r: every row is owned by a point of the corrected side, so the call
has 2000 direct merge edges and its merge stages do their work on 2000 components of two.  The model is the rigid motion between the two
keyframes (scale 1): the map stays where it is.  The descriptors of these maps are random: the searches walk their windows and take their
distances, and accept nothing - as the yardstick's does, whose merge stages therefore return at their first line.  The call changes the
map, so every call runs on a freshly built one (the build is not timed); the yardstick changes nothing and runs ten times on one map.  No
output array but the counts.  Device medians of 10 calls per line, each behind one call that is not counted.
python tools/correct_rate.py   (one MI355X)
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "visual-slam_amd"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402

import vslam_amd as V  # noqa: E402
import bow_rate  # noqa: E402
from bow_rate import K, ROWS, medians  # noqa: E402
from loop_rate import ASK, line  # noqa: E402

CORRECTED = list(range(5, 15))
GROUP = list(range(30, 40))
CAND = 30


def correct_call(m, n_kf):
    poses = np.zeros((n_kf, 12))
    for i, kf in enumerate(m.keyframes):
        poses[i] = np.asarray(kf["pose"], np.float64)[:3, :4].reshape(12)
    Ka = np.ascontiguousarray(K, np.float64).reshape(9)
    cm, gm = np.zeros(n_kf, np.uint8), np.zeros(n_kf, np.uint8)
    cm[CORRECTED] = 1; gm[GROUP] = 1
    lp = (CAND * ROWS + np.arange(ROWS)).astype(np.int32)
    Tp, Tc = poses[ASK].reshape(3, 4), poses[CAND].reshape(3, 4)
    R = Tp[:, :3] @ Tc[:, :3].T
    t = Tp[:, 3] - R @ Tc[:, 3]
    prm = V.MapCorrectParams(ASK, CAND, 1.0, (C.c_double * 9)(*R.reshape(9)), (C.c_double * 3)(*t), cm.ctypes.data, gm.ctypes.data, lp.ctypes.data, 640, 480,
                             4.0, 1.2, 50, 5.991)
    out = V.MapCorrectOut()
    m._check(m.lib.mo_map_loop_correct(m._h, V._ptr(Ka), V._ptr(poses), C.byref(prm), C.byref(out)))
    return tuple(int(getattr(out, k)) for k in ("n_corrected", "n_moved", "n_loop_points", "n_direct_edges", "n_direct_gained", "n_pairs", "n_cand",
                                                "n_proposals", "n_edges", "n_absorbed", "n_points"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=50)
    ap.add_argument("--points", default="100000,1000000")
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    ctx = V.Context(device=0, max_w=640, max_h=480, max_batch=1)
    ctx.set_host_timing(True)
    for n_pts in [int(x) for x in args.points.split(",")]:
        bow_rate.N_PTS = n_pts   # (build reads the module's constant)
        m, _, _ = bow_rate.build(ctx, args.keyframes, np.random.default_rng(1))
        st, fdev, fwall, fres = medians(ctx, lambda: m.fuse_map_points(window=10, image_size=(640, 480)), args.calls)
        print("points %7d  keyframes %3d  fuse_map_points(window=10): device median %.3f ms  wall median %.3f ms  local %d pairs %d cand %d proposals %d  | %s"
              % (n_pts, args.keyframes, fdev, fwall, fres["n_local"], fres["n_pairs"], fres["n_cand"], fres["n_proposals"], line(st)), flush=True)
        m.close()
        wall, dev, stages, res = [], [], [], None
        for i in range(args.calls + 1):
            m, _, _ = bow_rate.build(ctx, args.keyframes, np.random.default_rng(1))
            t0 = time.perf_counter()
            res = correct_call(m, args.keyframes)
            dt = time.perf_counter() - t0
            if i:   # (the first call loads the kernels)
                s = ctx.stage_times()
                wall.append(dt); dev.append(sum(ms for _, ms in s)); stages.append(dict(s))
            m.close()
        st = {k: float(np.median([s[k] for s in stages])) for k in stages[0]}
        cdev = float(np.median(dev))
        print("points %7d  keyframes %3d  corrected %d  group %d  loop_correct: device median %.3f ms  wall median %.3f ms  corrected %d moved %d loop points %d "
              "direct edges %d gained %d  pairs %d cand %d proposals %d  edges %d absorbed %d points %d  | %s  | %.2f x fuse"
              % ((n_pts, args.keyframes, len(CORRECTED), len(GROUP), cdev, 1e3 * float(np.median(wall))) + res + (line(st), cdev / fdev)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
