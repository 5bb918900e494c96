"""Essential-graph optimisation (mo_map_pose_graph) against the number of keyframes, next to the loop correction it follows and the fusion
both are measured against: 64 / 256 / 1024 keyframes of the map tools/correct_rate.py builds (tools/bow_rate.py: 2000-row keyframes, 10^5
points, point i observed from the keyframes (i // 2000) % n_kf and the next), so the first 50 positions share 2000 points with their
neighbour and every later one hangs on its predecessor by the parent rule: a chain, the worst case for a block-Jacobi conjugate gradient.

The trajectory drifts in scale (0.1 % per keyframe); the last ten keyframes were corrected onto the undrifted side (their init carries
the drifted scale), three extra edges close the loop, position 0 is fixed.  Every call starts from the same init, so one map serves all
calls of a size (an accepted call moves the points and kP, which the graph does not read).  Per size: device time per call (the sum of
the stages pg_edges, pg_solve, pg_write; median of `calls` calls behind one that is not counted), the steps, the conjugate-gradient
iterations of all steps, final / initial cost; then fuse_map_points(window=10) and one mo_map_loop_correct on the same map.
python tools/posegraph_rate.py   (one MI355X)
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
from bow_rate import K, medians  # noqa: E402
from correct_rate import correct_call  # noqa: E402
from loop_rate import line  # noqa: E402

N_CORR = 10


def graph_inputs(m, n_kf, drift=0.001):
    """poses [n_kf][12] (the odometry: the map's poses with the translation scaled by the accumulated drift), init [n_kf][13], fixed, extras"""
    poses, init = np.zeros((n_kf, 12)), np.zeros((n_kf, 13))
    sc = 1.0
    for i, kf in enumerate(m.keyframes):
        T = np.asarray(kf["pose"], np.float64)[:3, :4].copy()
        true_t = T[:, 3].copy()
        sc *= 1.0 + drift
        T[:, 3] *= sc
        poses[i] = T.reshape(12)
        init[i, 0] = 1.0; init[i, 1:10] = T[:, :3].reshape(9); init[i, 10:] = T[:, 3]
        if i >= n_kf - N_CORR:   # corrected: back at the true pose, the similarity keeps the drifted scale
            init[i, 0] = sc; init[i, 10:] = sc * true_t
    fixed = np.zeros(n_kf, np.uint8)
    fixed[0] = 1
    last = n_kf - 1
    return poses, init, fixed, np.array([0, 1, 0], np.int32), np.array([last, last, last - 1], np.int32)


def pg_call(m, n_kf, inputs, max_steps, max_cg):
    poses, init, fixed, xa, xb = inputs
    prm = V.MapPgParams(fixed.ctypes.data, xa.ctypes.data, xb.ctypes.data, len(xa), 100, max_steps, max_cg, 1e-8, 1e-10,
                        (C.c_double * 9)(*np.ascontiguousarray(K, np.float64).reshape(9)))
    out = V.MapPgOut()
    m._check(m.lib.mo_map_pose_graph(m._h, V._ptr(poses), V._ptr(init), C.byref(prm), C.byref(out)))
    return {"steps": out.steps, "accepted": out.accepted, "cg_iters": out.cg_iters, "n_edges": out.n_edges, "n_free": out.n_free, "n_moved": out.n_moved,
            "cost": (out.cost[0], out.cost[1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", default="64,256,1024")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--max-steps", type=int, default=20)
    ap.add_argument("--max-cg", type=int, default=200)
    args = ap.parse_args()
    ctx = V.Context(device=0, max_w=640, max_h=480, max_batch=1)
    ctx.set_host_timing(True)
    m, _, _ = bow_rate.build(ctx, 50, np.random.default_rng(1))   # (loads the kernels of the correction: its one timed call below is warm)
    correct_call(m, 50)
    m.close()
    for n_kf in [int(x) for x in args.keyframes.split(",")]:
        t0 = time.perf_counter()
        m, _, _ = bow_rate.build(ctx, n_kf, np.random.default_rng(1))
        t_build = time.perf_counter() - t0
        inputs = graph_inputs(m, n_kf)
        st, dev, wall, res = medians(ctx, lambda: pg_call(m, n_kf, inputs, args.max_steps, args.max_cg), args.calls)
        vec = "LDS" if 5 * 7 * res["n_free"] * 8 <= 158 * 1024 else "global"
        print("keyframes %4d  points %d  pose_graph: device median %.3f ms  wall median %.3f ms  free %d edges %d  steps %d accepted %d  cg iterations %d  "
              "cost %.6g -> %.6g (x %.3g)  moved %d  vectors in %s  | %s  (map built in %.1f s)"
              % (n_kf, bow_rate.N_PTS, dev, wall, res["n_free"], res["n_edges"], res["steps"], res["accepted"], res["cg_iters"], res["cost"][0], res["cost"][1],
                 res["cost"][1] / res["cost"][0] if res["cost"][0] else 0.0, res["n_moved"], vec, line(st), t_build), flush=True)
        st, fdev, fwall, fres = medians(ctx, lambda: m.fuse_map_points(window=10, image_size=(640, 480)), args.calls)
        print("keyframes %4d  fuse_map_points(window=10): device median %.3f ms  wall median %.3f ms  local %d pairs %d cand %d  | %s"
              % (n_kf, fdev, fwall, fres["n_local"], fres["n_pairs"], fres["n_cand"], line(st)), flush=True)
        t0 = time.perf_counter()
        cres = correct_call(m, n_kf)
        cwall = time.perf_counter() - t0
        s = ctx.stage_times()
        print("keyframes %4d  loop_correct (one call): device %.3f ms  wall %.3f ms  moved %d absorbed %d  | %s  | pose_graph = %.1f x loop_correct, %.1f x fuse"
              % (n_kf, sum(ms for _, ms in s), 1e3 * cwall, cres[1], cres[9], line(dict(s)), dev / max(sum(ms for _, ms in s), 1e-9), dev / fdev), flush=True)
        m.close()
    ctx.close()


if __name__ == "__main__":
    main()
