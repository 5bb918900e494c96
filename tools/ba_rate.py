"""LocalMapper.bundle_adjust against the number of keyframes and the map size.

Keyframes of 2000 rows along x (random descriptors: no growth step finds a model), then points injected with three observations each:
point i on row i % 2000 of keyframe positions k, k - 1, k - 2 (mod n_kf), k = n_kf - 1 - (i // 2000) % n_kf, so the newest keyframes
are observed whatever the map size.  A row's keypoint is the projection of the first point that names it; the later points naming the
same row are wrong matches the robust rounds have to live with (the larger maps are mostly such edges: a stress case, not a clean one).
Poses of the window start 1 degree / 3 cm off.  Per (keyframes, map points): the device time of one call (sum of its stage events) after a call
without steps has sized the buffers - a second full call would start from the points the first one moved, a different problem -, its
wall time, the problem size and the steps taken.
python tools/ba_rate.py   (one MI355X; under rocprofv3 --kernel-trace --stats for the per-kernel times)
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "visual-slam_amd")]

import numpy as np  # noqa: E402

import vslam_amd as V  # noqa: E402
from vslam_amd.mapper import LocalMapper  # noqa: E402

K = np.array([[500.0, 0, 320.0], [0, 500.0, 240.0], [0, 0, 1.0]])
ROWS = 2000


def build(ctx, n_kf, n_pts, rng):
    m = LocalMapper(K, save_every_keyframe=False, context=ctx, capacity=(max(n_kf, 2), ROWS, n_pts, 3 * n_pts))
    img = np.zeros((480, 640), np.uint8)
    X = np.column_stack([rng.uniform(-3, 3, n_pts), rng.uniform(-2, 2, n_pts), rng.uniform(4, 10, n_pts)]).astype(np.float32)
    i = np.arange(n_pts)
    k0 = n_kf - 1 - (i // ROWS) % n_kf
    kfs = np.stack([k0, (k0 - 1) % n_kf, (k0 - 2) % n_kf], 1)
    poses = []
    for k in range(n_kf):
        T = np.eye(4); T[0, 3] = -0.1 * k
        kp = np.zeros(ROWS, V.KP_DTYPE)
        for c in range(3):   # the first point naming (k, row) gives the row its keypoint
            sel = np.flatnonzero(kfs[:, c] == k)[::-1]
            x = (K @ (X[sel].astype(np.float64) @ T[:3, :3].T + T[:3, 3]).T).T
            kp["x"][sel % ROWS] = x[:, 0] / x[:, 2]; kp["y"][sel % ROWS] = x[:, 1] / x[:, 2]
        m.add_keyframe(img, kp, rng.integers(0, 256, (ROWS, 32)).astype(np.uint8), T)
        poses.append(T)
    off = (np.arange(n_pts + 1) * 3).astype(np.int32)
    z = np.zeros(n_pts, np.int32)
    arrays = (X, np.zeros((n_pts, 3), np.uint8), i.astype(np.int32), off, kfs.reshape(-1).astype(np.int32), np.repeat(i % ROWS, 3).astype(np.int32))
    m._check(m.lib.mo_map_add_points(m._h, n_pts, *[V._ptr(a) for a in arrays], V._ptr(z - 1), V._ptr(z)))
    m._sync_size()
    return m, X, poses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", default="16,64")
    ap.add_argument("--points", default="100000,1000000")
    ap.add_argument("--window", type=int, default=10)
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    ctx = V.Context(device=0, max_w=640, max_h=480, max_batch=1)
    ctx.set_host_timing(True)
    w = np.deg2rad(1.0)
    P = np.eye(4)
    P[:3, :3] = [[np.cos(w), -np.sin(w), 0], [np.sin(w), np.cos(w), 0], [0, 0, 1]]
    P[:3, 3] = [0.03, 0.0, 0.0]
    for n_kf in [int(x) for x in args.keyframes.split(",")]:
        for n_pts in [int(x) for x in args.points.split(",")]:
            m, X, poses = build(ctx, n_kf, n_pts, rng)
            wall, dev, stages = [], [], []
            for call in range(2):
                for k, kf in enumerate(m.keyframes):
                    kf["pose"][:] = P @ poses[k] if k >= n_kf - args.window else poses[k]
                t0 = time.perf_counter()
                # the first call takes no step: it sizes the buffers and leaves poses and points as they are; the second is timed
                ok, info = m.bundle_adjust(window=args.window, max_steps=(5, 10) if call else (0, 0))
                if call == 0:
                    continue
                wall.append(time.perf_counter() - t0)
                st = ctx.stage_times()
                dev.append(sum(ms for _, ms in st))
                agg = {}
                for name, ms in st:
                    agg[name] = agg.get(name, 0.0) + ms
                stages.append(agg)
            med = {k: np.median([s.get(k, 0.0) for s in stages]) for k in stages[0]}
            print("keyframes %3d  rows %d  map_points %8d  window %2d  free %d fixed %d  local %8d  edges %8d  inliers %8d  steps %s accepted %s  "
                  "ba device %.3f ms  wall %.3f ms  ok %s  | %s"
                  % (n_kf, ROWS, n_pts, args.window, info["n_free"], info["n_fixed"], info["n_local"], info["n_edges"], info["n_inliers"], info["steps"],
                     info["accepted"], np.median(dev), 1e3 * np.median(wall), ok, "  ".join("%s %.3f" % kv for kv in med.items())), flush=True)
            m.close()
    ctx.close()


if __name__ == "__main__":
    main()
