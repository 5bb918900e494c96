"""LocalMapper.track_local_map_batch against a loop of track_local_map over the same frames, on the maps of tools/track_map_rate.py.

The maps: 16 / 64 keyframes of 2000 rows, 10^5 / 10^6 points, window 10 (track_map_rate.build).  The frames: that tool's frame of 2000
keypoints, every frame of a batch from a predicted pose of its own (turned by 1 degree +- up to 0.2 about the optical axis), as host
arrays.  Per (map, batch size), three alternating runs of
  batch  the device time of one warm track_local_map_batch call (sum of its stage events), median of --calls calls, with its stages;
  loop   the device time of one warm track_local_map call per frame, summed over the batch; median of --calls passes over the batch
         (3 passes from 64 frames on),
in the same process on the same map, then frames/s of both (device time) and the batch's wall time.  The tables at the end: device time
per frame batch / loop per configuration, and the loop's own run-to-run spread next to it.
python tools/track_batch_rate.py   (one MI355X)
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "visual-slam_amd"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402

import vslam_amd as V  # noqa: E402
from track_map_rate import ROWS, _rot, build  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", default="16,64")
    ap.add_argument("--points", default="100000,1000000")
    ap.add_argument("--batches", default="1,4,16,64,256")
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    ctx = V.Context(device=0, max_w=640, max_h=480, max_batch=1)
    ctx.set_host_timing(True)
    print("tools/track_batch_rate.py on one MI355X (device times: sums of stage events; medians of %d warm calls; %d alternating runs batch, loop, "
          "batch, loop, ...; ms)" % (args.calls, args.runs))
    table = []
    for n_kf in [int(x) for x in args.keyframes.split(",")]:
        for n_pts in [int(x) for x in args.points.split(",")]:
            m, qk, qd, pose0 = build(ctx, n_kf, n_pts, rng)
            for nb in [int(x) for x in args.batches.split(",")]:
                frames = [(qk, qd)] * nb
                poses = []
                for i in range(nb):
                    T = pose0.copy()
                    T[:3, :3] = _rot([0.0, 0.0, np.deg2rad(1.0 + 0.2 * np.sin(1.0 + i))])
                    poses.append(T)
                poses = np.array(poses)
                ok, _, infos = m.track_local_map_batch(frames, poses, window=args.window)   # warm: buffers sized
                for i in range(min(nb, 2)):
                    m.track_local_map(qk, qd, poses[i], window=args.window)
                b_runs, l_runs, b_wall, med = [], [], [], {}
                for _ in range(args.runs):
                    dev, wall, stages = [], [], []
                    for _ in range(args.calls):
                        t0 = time.perf_counter()
                        ok, _, infos = m.track_local_map_batch(frames, poses, window=args.window)
                        wall.append(time.perf_counter() - t0)
                        st = ctx.stage_times()
                        dev.append(sum(ms for _, ms in st))
                        agg = {}
                        for name, ms in st:
                            agg[name] = agg.get(name, 0.0) + ms
                        stages.append(agg)
                    b_runs.append(float(np.median(dev))); b_wall.append(1e3 * float(np.median(wall)))
                    med = {k: np.median([s.get(k, 0.0) for s in stages]) for k in stages[0]}
                    passes = []
                    for _ in range(args.calls if nb < 64 else 3):
                        tot = 0.0
                        for i in range(nb):
                            m.track_local_map(qk, qd, poses[i], window=args.window)
                            tot += sum(ms for _, ms in ctx.stage_times())
                        passes.append(tot)
                    l_runs.append(float(np.median(passes)))
                b, lo = float(np.mean(b_runs)), float(np.mean(l_runs))
                print("keyframes %3d  rows %d  map_points %8d  window %2d  frames %3d  local %7d  ok %3d  batch device %.3f ms = %.4f ms/frame = %8.0f frames/s  "
                      "wall %.3f ms  | loop device %.3f ms = %.4f ms/frame = %8.0f frames/s  | %s"
                      % (n_kf, ROWS, n_pts, args.window, nb, infos[0]["n_local"], int(ok.sum()), b, b / nb, 1e3 * nb / b, float(np.median(b_wall)), lo,
                         lo / nb, 1e3 * nb / lo, "  ".join("%s %.3f" % kv for kv in med.items())), flush=True)
                table.append((n_kf, n_pts, nb, b_runs, l_runs))
            m.close()
    print("\ndevice time per frame, batch / loop (runs alternating batch, loop, batch, loop, ...; ms per call of the whole batch)")
    print("keyframes   points  frames   batch runs" + " " * (8 * args.runs - 9) + "batch mean   loop runs" + " " * (8 * args.runs - 8)
          + "loop mean   batch / loop   speed-up   loop's own spread")
    for n_kf, n_pts, nb, b_runs, l_runs in table:
        b, lo = np.mean(b_runs), np.mean(l_runs)
        print("%9d %8d %7d   %s  %9.3f    %s  %9.3f   %10.4f   %7.2fx   %8.1f %%"
              % (n_kf, n_pts, nb, " ".join("%7.3f" % x for x in b_runs), b, " ".join("%7.3f" % x for x in l_runs), lo, b / lo, lo / b,
                 100.0 * (max(l_runs) - min(l_runs)) / lo))
    ctx.close()


if __name__ == "__main__":
    main()
