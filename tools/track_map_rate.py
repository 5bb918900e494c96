"""LocalMapper.track_local_map against the number of keyframes, the map size and the local-map window.

Keyframes of 2000 rows with random descriptors (no growth step finds a model), then points injected with two observations each:
point i on row i % 2000 of keyframe positions n_kf - 1 - j and n_kf - 2 - j (mod n_kf), j = (i // 2000) % n_kf, so the newest
keyframes are observed whatever the map size.  The frame sees points 0 .. 1999 (the rows of the last keyframe, a few bits flipped)
from a pose 1 degree and 3 cm away from the predicted one; every other point in view is a candidate whose search finds nothing.
Per (keyframes, map points, window): the device time of one warm call (sum of its stage events, median of 10), its wall time, the
matches and inliers of the last pass, the local-map size.
--frustum: every line twice, the plain call and then track_local_map(frustum=True) on the same map in the same run, the second with
the time it adds and the share of the preparation stage (track_prep: k_trk_rep and the keypoint grid) that is.
python tools/track_map_rate.py   (one MI355X; under rocprofv3 --kernel-trace --stats for the per-kernel times)
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


def _rot(w):
    th = np.linalg.norm(w)
    k = np.asarray(w) / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def build(ctx, n_kf, n_pts, rng):
    m = LocalMapper(K, save_every_keyframe=False, context=ctx, capacity=(max(n_kf, 2), ROWS, n_pts, 2 * n_pts))
    img = np.zeros((480, 640), np.uint8)
    X = np.column_stack([rng.uniform(-3, 3, n_pts), rng.uniform(-2, 2, n_pts), rng.uniform(4, 10, n_pts)])
    descs = []
    for k in range(n_kf):
        T = np.eye(4); T[0, 3] = -0.01 * k
        d = rng.integers(0, 256, (ROWS, 32)).astype(np.uint8)
        m.add_keyframe(img, np.zeros(ROWS, V.KP_DTYPE), d, T)
        descs.append(d)
    i = np.arange(n_pts)
    k0 = n_kf - 1 - (i // ROWS) % n_kf
    obs_kf = np.stack([k0, (k0 - 1) % n_kf], 1).reshape(-1).astype(np.int32)
    obs_kp = np.repeat(i % ROWS, 2).astype(np.int32)
    off = (np.arange(n_pts + 1) * 2).astype(np.int32)
    z = np.zeros(n_pts, np.int32)
    arrays = (X.astype(np.float32), np.zeros((n_pts, 3), np.uint8), i.astype(np.int32), off, obs_kf, obs_kp)
    m._check(m.lib.mo_map_add_points(m._h, n_pts, *[V._ptr(a) for a in arrays], V._ptr(z - 1), V._ptr(z)))
    m._sync_size()
    # the frame: points 0 .. ROWS - 1 seen from T, descriptors of the last keyframe's rows with a few flipped bits
    T = np.eye(4); T[:3, 3] = [0.02, -0.01, 0.03]
    x = (K @ (X[:ROWS] @ T[:3, :3].T + T[:3, 3]).T).T
    qk = np.zeros(ROWS, V.KP_DTYPE)
    qk["x"] = x[:, 0] / x[:, 2]; qk["y"] = x[:, 1] / x[:, 2]
    qd = descs[-1].copy()
    qd[:, 0] ^= rng.integers(0, 8, ROWS).astype(np.uint8)
    pose0 = np.eye(4)
    pose0[:3, :3] = _rot([0.0, 0.0, np.deg2rad(1.0)])
    pose0[:3, 3] = T[:3, 3] + [0.03, 0.0, 0.0]
    return m, qk, qd, pose0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", default="16,64")
    ap.add_argument("--points", default="100000,1000000")
    ap.add_argument("--windows", default="10,0")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--frustum", action="store_true", help="also time track_local_map(frustum=True) on the same map")
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    ctx = V.Context(device=0, max_w=640, max_h=480, max_batch=1)
    ctx.set_host_timing(True)
    for n_kf in [int(x) for x in args.keyframes.split(",")]:
        for n_pts in [int(x) for x in args.points.split(",")]:
            m, qk, qd, pose0 = build(ctx, n_kf, n_pts, rng)
            for window in [int(x) for x in args.windows.split(",")]:
                plain = None
                for frustum in ([False, True] if args.frustum else [False]):
                    kw = {"frustum": True} if frustum else {}
                    m.track_local_map(qk, qd, pose0, window=window, **kw)   # warm: buffers sized
                    wall, dev, stages = [], [], []
                    for _ in range(args.calls):
                        t0 = time.perf_counter()
                        ok, pose, info = m.track_local_map(qk, qd, pose0, window=window, **kw)
                        wall.append(time.perf_counter() - t0)
                        st = ctx.stage_times()
                        dev.append(sum(ms for _, ms in st))
                        agg = {}
                        for name, ms in st:
                            agg[name] = agg.get(name, 0.0) + ms
                        stages.append(agg)
                    med = {k: np.median([s.get(k, 0.0) for s in stages]) for k in stages[0]}
                    extra = ""
                    if frustum:
                        extra = "  | frustum adds %.3f ms = %.2f of track_prep (repeats of the plain call: %.3f .. %.3f ms)" % (
                            np.median(dev) - np.median(plain), (np.median(dev) - np.median(plain)) / med["track_prep"], min(plain), max(plain))
                    else:
                        plain = dev
                    print("keyframes %3d  rows %d  map_points %8d  window %2d  %s  local %8d  track device median %.3f ms (%.3f .. %.3f)  wall median %.3f ms"
                          "  ok %s  matches %s inliers %s  | %s%s"
                          % (n_kf, ROWS, n_pts, window, "frustum" if frustum else "plain  ", info["n_local"], np.median(dev), min(dev), max(dev),
                             1e3 * np.median(wall), ok, info["pass_matches"], info["pass_inliers"], "  ".join("%s %.3f" % kv for kv in med.items()), extra),
                          flush=True)
            m.close()
    ctx.close()


if __name__ == "__main__":
    main()
