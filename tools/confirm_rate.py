"""Loop confirmation (mo_map_loop_confirm) against the number of candidates and the size of the map, next to the alignment that feeds it:
the stages of the call at 1, 4 and 16 candidates of 2000-row keyframes with groups of 10 keyframes, on maps of 10^5 and 10^6 points, and
mo_map_loop_sim3 on the same inputs in the same process.

The map of tools/bow_rate.py at 64 keyframes (2000-row keyframes whose row r holds the projection of point r under the keyframe's pose;
every point is observed from two consecutive keyframes), with the match lists of tools/sim3_rate.py: every row of the asking keyframe and
of a candidate names point r, 40 % of the rows of every candidate name another point instead.  The alignment runs first; its models and
inlier flags are the confirmation's inputs, so about 1200 rows per candidate are seeds and 800 are sources of the guided search.  A
candidate's group is the candidate and the 9 positions behind it.  The descriptors of these maps are random: the searches walk their
windows and take their distances, and accept nothing (the pair lists are the seeds, the projection claims no row).  No output array but
the counts.  Device medians of 10 warm calls per line.
python tools/confirm_rate.py   (one MI355X)
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "visual-slam_amd"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402

import vslam_amd as V  # noqa: E402
import bow_rate  # noqa: E402
from bow_rate import K, ROWS, medians  # noqa: E402
from loop_rate import ASK, line  # noqa: E402

GROUP = 10


def calls(m, n_kf, n_cand, n_hyp, rng):
    """(the alignment's call, the confirmation's call) on the same lists; the confirmation reads what the alignment's last run wrote"""
    n_pts = m._n_points
    cand = np.array([(ASK + 7 + 3 * c) % n_kf for c in range(n_cand)], np.int32)
    cur = np.arange(ROWS, dtype=np.int32)
    mpt = np.tile(cur, (n_cand, 1))
    out_rows = rng.random((n_cand, ROWS)) < 0.4
    mpt[out_rows] = rng.integers(ROWS, n_pts, int(out_rows.sum()))
    mrow = np.tile(cur, (n_cand, 1))
    poses = np.zeros((n_kf, 12))
    for i, kf in enumerate(m.keyframes):
        poses[i] = np.asarray(kf["pose"], np.float64)[:3, :4].reshape(12)
    Ka = np.ascontiguousarray(K, np.float64).reshape(9)
    scale, R, t = np.zeros(n_cand), np.zeros((n_cand, 9)), np.zeros((n_cand, 3))
    n_corr, n_inl = np.zeros(n_cand, np.int32), np.zeros(n_cand, np.int32)
    inl = np.zeros((n_cand, ROWS), np.uint8)
    group = np.zeros((n_cand, n_kf), np.uint8)
    for c, k in enumerate(cand):
        group[c, [(int(k) + q) % n_kf for q in range(GROUP)]] = 1
    sprm = V.MapSim3Params(ASK, n_cand, cand.ctypes.data, cur.ctypes.data, mpt.ctypes.data, mrow.ctypes.data, n_hyp, 20, 4096, 9.210, 1.2)
    sout = V.MapSim3Out(scale.ctypes.data, R.ctypes.data, t.ctypes.data, n_corr.ctypes.data, n_inl.ctypes.data, inl.ctypes.data)
    n_pairs, n_guided, n_in2 = np.zeros(n_cand, np.int32), np.zeros(n_cand, np.int32), np.zeros(n_cand, np.int32)
    cprm = V.MapConfirmParams(ASK, n_cand, cand.ctypes.data, cur.ctypes.data, mpt.ctypes.data, mrow.ctypes.data, inl.ctypes.data, scale.ctypes.data,
                              R.ctypes.data, t.ctypes.data, group.ctypes.data, 640, 480, 50, 20, 40, 7.5, 10.0, 9.210, 1.2)
    cout = V.MapConfirmOut(None, None, None, n_pairs.ctypes.data, n_guided.ctypes.data, n_in2.ctypes.data)
    keep = (cand, cur, mpt, mrow, poses, Ka, scale, R, t, n_corr, n_inl, inl, group, n_pairs, n_guided, n_in2)

    def sim3():
        m._check(m.lib.mo_map_loop_sim3(m._h, V._ptr(Ka), V._ptr(poses), C.byref(sprm), C.byref(sout)))
        return int(sout.win), int(sout.ok), int(sout.win_inliers), len(keep)

    def confirm():
        m._check(m.lib.mo_map_loop_confirm(m._h, V._ptr(Ka), V._ptr(poses), C.byref(cprm), C.byref(cout)))
        return (int(cout.win), int(cout.ok), int(cout.win_inliers), int(n_pairs.min()), int(n_pairs.max()), int(n_guided.sum()), int(cout.n_loop_points),
                int(cout.n_proj_cand), int(cout.n_proj), int(cout.n_total))
    return sim3, confirm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=64)
    ap.add_argument("--points", default="100000,1000000")
    ap.add_argument("--candidates", default="1,4,16")
    ap.add_argument("--n-hyp", type=int, default=300)
    args = ap.parse_args()
    ctx = V.Context(device=0, max_w=640, max_h=480, max_batch=1)
    ctx.set_host_timing(True)
    for n_pts in [int(x) for x in args.points.split(",")]:
        rng = np.random.default_rng(1)
        bow_rate.N_PTS = n_pts   # (build reads the module's constant)
        m, _, _ = bow_rate.build(ctx, args.keyframes, rng)
        for nc in [int(x) for x in args.candidates.split(",")]:
            sim3, confirm = calls(m, args.keyframes, nc, args.n_hyp, rng)
            st, sdev, swall, sres = medians(ctx, sim3)
            print("points %7d  keyframes %3d  candidates %2d  n_hyp %d  loop_sim3:    device median %.3f ms  wall median %.3f ms  win %d ok %d inliers %d  | %s"
                  % ((n_pts, args.keyframes, nc, args.n_hyp, sdev, swall) + sres[:3] + (line(st),)), flush=True)
            st, dev, wall, res = medians(ctx, confirm)
            print("points %7d  keyframes %3d  candidates %2d  group %d  loop_confirm: device median %.3f ms  wall median %.3f ms  win %d ok %d inliers %d  "
                  "pairs %d .. %d  guided %d  loop points %d  projected %d  claimed %d  total %d  | %s  | %.2f x loop_sim3"
                  % ((n_pts, args.keyframes, nc, GROUP, dev, wall) + res + (line(st), dev / sdev)), flush=True)
        m.close()
    ctx.close()


if __name__ == "__main__":
    main()
