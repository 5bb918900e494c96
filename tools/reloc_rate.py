"""LocalMapper.relocalize against the number of keyframes and the map size.

Keyframes of ~2000 rows with random descriptors (no growth step finds a model), then points injected with two observations each on
rows of the keyframes; the query is one keyframe's rows (descriptors with a few flipped bits, positions projected from the points
at a nearby pose).  Per (keyframes, map points): the device time of one warm call (sum of its stage events, median of 10) and its
wall time, the winner's inliers.
python tools/reloc_rate.py   (one MI355X; under rocprofv3 --kernel-trace --stats for the per-kernel times)
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
    m = LocalMapper(K, save_every_keyframe=False, context=ctx)
    img = np.zeros((480, 640), np.uint8)
    X = np.column_stack([rng.uniform(-3, 3, n_pts), rng.uniform(-2, 2, n_pts), rng.uniform(4, 10, n_pts)])
    descs = []
    for k in range(n_kf):
        T = np.eye(4); T[0, 3] = -0.01 * k
        kps = np.zeros(ROWS, V.KP_DTYPE)
        x = (K @ (X[:ROWS] + T[:3, 3]).T).T if n_pts >= ROWS else None
        if x is not None:
            kps["x"] = x[:, 0] / x[:, 2]; kps["y"] = x[:, 1] / x[:, 2]
        d = rng.integers(0, 256, (ROWS, 32)).astype(np.uint8)
        m.add_keyframe(img, kps, d, T)
        descs.append(d)
    # point i observed by rows i % ROWS of keyframes (i // ROWS) % n_kf and the next one
    i = np.arange(n_pts)
    k0 = (i // ROWS) % n_kf
    obs_kf = np.stack([k0, (k0 + 1) % n_kf], 1).reshape(-1).astype(np.int32)
    obs_kp = np.repeat(i % ROWS, 2).astype(np.int32)
    off = (np.arange(n_pts + 1) * 2).astype(np.int32)
    z = np.zeros(n_pts, np.int32)
    arrays = (X.astype(np.float32), np.zeros((n_pts, 3), np.uint8), i.astype(np.int32), off, obs_kf, obs_kp)
    m._check(m.lib.mo_map_add_points(m._h, n_pts, *[V._ptr(a) for a in arrays], V._ptr(z - 1), V._ptr(z)))
    m._sync_size()
    # the query: keyframe 0's rows seen from a nearby pose
    xq = (K @ (X[:ROWS] + np.array([0.02, -0.01, 0.03])).T).T
    qk = np.zeros(ROWS, V.KP_DTYPE)
    qk["x"] = xq[:, 0] / xq[:, 2]; qk["y"] = xq[:, 1] / xq[:, 2]
    qd = descs[0].copy()
    qd[:, 0] ^= rng.integers(0, 8, ROWS).astype(np.uint8)
    return m, qk, qd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", default="16,64,256")
    ap.add_argument("--points", default="100000,1000000")
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    ctx = V.Context(device=0, max_w=640, max_h=480, max_batch=1)
    ctx.set_host_timing(True)
    for n_kf in [int(x) for x in args.keyframes.split(",")]:
        for n_pts in [int(x) for x in args.points.split(",")]:
            m, qk, qd = build(ctx, n_kf, n_pts, rng)
            m.relocalize(qk, qd)   # warm: buffers sized
            wall, dev, stages = [], [], []
            for _ in range(10):
                t0 = time.perf_counter()
                ok, pose, info = m.relocalize(qk, qd)
                wall.append(time.perf_counter() - t0)
                st = ctx.stage_times()
                dev.append(sum(ms for _, ms in st))
                stages.append(dict(st))
            med = {k: np.median([s[k] for s in stages]) for k in stages[0]}
            print("keyframes %4d  rows %d  map_points %8d  relocalize device median %.3f ms  wall median %.3f ms  ok %s inliers %d  | %s"
                  % (n_kf, ROWS, n_pts, np.median(dev), 1e3 * np.median(wall), ok, info["n_inliers"],
                     "  ".join("%s %.3f" % kv for kv in med.items())), flush=True)
            m.close()
    ctx.close()


if __name__ == "__main__":
    main()
