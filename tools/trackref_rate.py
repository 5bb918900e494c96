"""LocalMapper.track_reference_keyframe against the vocabulary size and the map size, device time per stage; beside it, on the same
frame and map, one track_local_map call and one relocalize(preselect=1) call.

The map is tools/track_map_rate.py's: keyframes of 2000 rows with random descriptors, points injected with two observations each so
that the last keyframe's 2000 rows all have a point; the frame sees those points (the last keyframe's rows, a few bits flipped) from
a pose 1 degree and 3 cm from the keyframe's.  The vocabulary is trained on the keyframes' rows, 5 iterations.
Per (words, map points): the median over the warm calls of every stage (trackref_words: the staged frame quantised - the keyframes
are quantised by the first call; trackref_prep: k_trk_init, point_of of the reference keyframe over the whole map, the bucket sort;
trackref_search: the search and the row pass; trackref_orient; trackref_refine: compaction and refinement), their sum, the wall time,
and the counts.
python tools/trackref_rate.py > profiles/trackref_rate.txt   (one MI355X)
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "visual-slam_amd"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402

import vslam_amd as V  # noqa: E402
from track_map_rate import ROWS, build  # noqa: E402


def timed(ctx, call, calls):
    call()   # warm: buffers sized, the keyframes quantised
    wall, stages = [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        res = call()
        wall.append(time.perf_counter() - t0)
        agg = {}
        for name, ms in ctx.stage_times():
            agg[name] = agg.get(name, 0.0) + ms
        stages.append(agg)
    med = {k: float(np.median([s.get(k, 0.0) for s in stages])) for k in stages[0]}
    dev = [sum(s.values()) for s in stages]
    return res, med, float(np.median(dev)), min(dev), max(dev), 1e3 * float(np.median(wall))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=16)
    ap.add_argument("--points", default="100000,1000000")
    ap.add_argument("--words", default="256,1024,4096")
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    ctx = V.Context(device=0, max_w=640, max_h=480, max_batch=1)
    ctx.set_host_timing(True)
    for n_pts in [int(x) for x in args.points.split(",")]:
        rng = np.random.default_rng(1)
        m, qk, qd, pose0 = build(ctx, args.keyframes, n_pts, rng)
        rows = [kf["descriptors"] for kf in m.keyframes]
        for n_words in [int(x) for x in args.words.split(",")]:
            voc = V.Vocabulary.train(rows, n_words, 5, context=ctx)
            m.set_vocabulary(voc)
            lengths = np.bincount(m.keyframe_words(-1), minlength=n_words)
            (ok, pose, info), med, dev, lo, hi, wall = timed(
                ctx, lambda: m.track_reference_keyframe(qk, qd, pose=pose0), args.calls)   # (every angle is 0: one bin, the stage keeps all)
            print("keyframes %3d  rows %d  map_points %8d  words %4d (longest bucket of the keyframe %d, empty %d)  track_reference device median %.3f ms "
                  "(%.3f .. %.3f)  wall median %.3f ms  ok %s  cand %d claims %d matches %d inliers %d  | %s"
                  % (args.keyframes, ROWS, n_pts, n_words, lengths.max(), (lengths == 0).sum(), dev, lo, hi, wall, ok, info["n_cand"], info["n_claims"],
                     info["n_matches"], info["n_inliers"], "  ".join("%s %.3f" % kv for kv in med.items())), flush=True)
        (ok, pose, info), med, dev, lo, hi, wall = timed(ctx, lambda: m.track_local_map(qk, qd, pose0), args.calls)
        print("keyframes %3d  rows %d  map_points %8d  track_local_map (window 10)  device median %.3f ms (%.3f .. %.3f)  wall median %.3f ms  ok %s  "
              "matches %s inliers %s  | %s" % (args.keyframes, ROWS, n_pts, dev, lo, hi, wall, ok, info["pass_matches"], info["pass_inliers"],
                                              "  ".join("%s %.3f" % kv for kv in med.items())), flush=True)
        (ok, pose, info), med, dev, lo, hi, wall = timed(ctx, lambda: m.relocalize(qk, qd, preselect=1), args.calls)
        print("keyframes %3d  rows %d  map_points %8d  relocalize(preselect=1, words %d)  device median %.3f ms (%.3f .. %.3f)  wall median %.3f ms  ok %s  "
              "kf_pos %d inliers %d  | %s" % (args.keyframes, ROWS, n_pts, n_words, dev, lo, hi, wall, ok, info["kf_pos"], info["n_inliers"],
                                             "  ".join("%s %.3f" % kv for kv in med.items())), flush=True)
        m.close()
    ctx.close()


if __name__ == "__main__":
    main()
