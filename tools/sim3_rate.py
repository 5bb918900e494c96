"""Loop alignment (mo_map_loop_sim3) against the number of candidates, next to the detection that feeds it: the stages of the call at 1, 4
and 16 candidates of 2000-row keyframes with n_hyp = 300, and mo_map_loop_candidates(max_cand=4) on the same map in the same process.

The map of tools/bow_rate.py at 64 keyframes (2000-row keyframes whose row r holds the projection of point r under the keyframe's
pose).  The match lists are constructed: every row of the asking keyframe and of a candidate names point r, so the true similarity is
the relative pose at scale 1 and a row is an inlier; 40 % of the rows of every candidate name another point instead (outliers).  All
2000 rows are pairs: the worst case of the scoring.  No output array but the counts.  Device medians of 10 warm calls per line.
python tools/sim3_rate.py   (one MI355X)
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "visual-slam_amd"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402

import vslam_amd as V  # noqa: E402
from bow_rate import K, N_PTS, ROWS, build, medians  # noqa: E402
from loop_rate import ASK, line, loop_call  # noqa: E402


def sim3_call(m, n_kf, n_cand, n_hyp, rng):
    cand = np.array([(ASK + 7 + 3 * c) % n_kf for c in range(n_cand)], np.int32)
    cur = np.arange(ROWS, dtype=np.int32)
    mpt = np.tile(cur, (n_cand, 1))
    out_rows = rng.random((n_cand, ROWS)) < 0.4
    mpt[out_rows] = rng.integers(ROWS, N_PTS, int(out_rows.sum()))
    mrow = np.tile(cur, (n_cand, 1))
    poses = np.zeros((n_kf, 12))
    for i, kf in enumerate(m.keyframes):
        poses[i] = np.asarray(kf["pose"], np.float64)[:3, :4].reshape(12)
    Ka = np.ascontiguousarray(K, np.float64).reshape(9)
    n_corr, n_inl = np.zeros(n_cand, np.int32), np.zeros(n_cand, np.int32)
    prm = V.MapSim3Params(ASK, n_cand, cand.ctypes.data, cur.ctypes.data, mpt.ctypes.data, mrow.ctypes.data, n_hyp, 20, 4096, 9.210, 1.2)
    out = V.MapSim3Out(None, None, None, n_corr.ctypes.data, n_inl.ctypes.data, None)
    keep = (cand, cur, mpt, mrow, poses, Ka, n_corr, n_inl)

    def call():
        m._check(m.lib.mo_map_loop_sim3(m._h, V._ptr(Ka), V._ptr(poses), C.byref(prm), C.byref(out)))
        return int(out.win), int(out.ok), int(out.win_inliers), int(n_corr.min()), int(n_inl.min()), int(n_inl.max()), len(keep)
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=64)
    ap.add_argument("--words", type=int, default=1024)
    ap.add_argument("--candidates", default="1,4,16")
    ap.add_argument("--n-hyp", type=int, default=300)
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    ctx = V.Context(device=0, max_w=640, max_h=480, max_batch=1)
    ctx.set_host_timing(True)
    voc = V.Vocabulary.train([rng.integers(0, 256, (ROWS, 32)).astype(np.uint8) for _ in range(50)], args.words, 10, context=ctx)
    m, _, _ = build(ctx, args.keyframes, rng)
    m.set_vocabulary(voc)
    st, dev, wall, res = medians(ctx, loop_call(m, 4))
    print("keyframes %4d  words %5d  loop_candidates(max_cand=4): device median %.3f ms  wall median %.3f ms  | %s" % (args.keyframes, args.words, dev, wall, line(st)),
          flush=True)
    loop_dev = dev
    for nc in [int(x) for x in args.candidates.split(",")]:
        st, dev, wall, res = medians(ctx, sim3_call(m, args.keyframes, nc, args.n_hyp, rng))
        print("keyframes %4d  candidates %2d  n_hyp %d  loop_sim3: device median %.3f ms  wall median %.3f ms  win %d ok %d inliers %d  pairs >= %d  "
              "inliers per candidate %d .. %d  | %s  | %.2f x loop_candidates(max_cand=4)"
              % ((args.keyframes, nc, args.n_hyp, dev, wall) + res[:6] + (line(st), dev / loop_dev)), flush=True)
    m.close(); voc.close(); ctx.close()


if __name__ == "__main__":
    main()
