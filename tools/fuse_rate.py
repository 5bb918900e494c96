"""LocalMapper.fuse_map_points against the number of keyframes and the map size, next to track_local_map on the same map.

Keyframes of 2000 rows: keypoints uniform in the image, random descriptors (no growth step finds a model).  Points with two
observations each, as tools/track_map_rate.py injects them: point i on row i % 2000 of keyframe positions n_kf - 1 - j and
n_kf - 2 - j (mod n_kf), j = (i // 2000) % n_kf.  The first 2000 points are true features: rows r of the last three keyframes sit at
the projection of point r and carry one descriptor (each descriptor on two rows far apart, so that no growth step matches), so point r (observed in the last two) finds row r of the third, which point
2000 + r owns: 2000 merges in the first call.  Every other pair projects among random keypoints and finds nothing within max_dist.
Per (keyframes, map points): the device time of the first call (sum of its stage events; it merges) and the median of the later calls
(nothing left to fuse: preparation and search alone), the device time of one warm track_local_map call on the same map, the ratio.
The fuse call projects every local point into each of `window` keyframes, about window times the projections of one tracking pass.
--frustum: after the plain calls, the same later call as fuse_map_points(frustum=True) on the same map (nothing left to fuse either
way: preparation, the view kernels and the search), with the time it adds and the share of fuse_prep that is.
python tools/fuse_rate.py   (one MI355X; under rocprofv3 --kernel-trace --stats for the per-kernel times)
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "visual-slam_amd")]

import numpy as np  # noqa: E402

import vslam_amd as V  # noqa: E402
from vslam_amd.mapper import LocalMapper  # noqa: E402

K = np.array([[500.0, 0, 320.0], [0, 500.0, 240.0], [0, 0, 1.0]])
ROWS = 2000
W, H = 640, 480


def build(ctx, n_kf, n_pts, rng):
    m = LocalMapper(K, save_every_keyframe=False, context=ctx, capacity=(max(n_kf, 2), ROWS, n_pts, 2 * n_pts))
    img = np.zeros((H, W), np.uint8)
    X = np.column_stack([rng.uniform(-3, 3, n_pts), rng.uniform(-2, 2, n_pts), rng.uniform(4, 10, n_pts)])
    X[:ROWS] = np.column_stack([rng.uniform(-1.5, 1.5, ROWS), rng.uniform(-1.2, 1.2, ROWS), rng.uniform(5, 10, ROWS)])   # in view of every keyframe
    own = rng.integers(0, 256, (ROWS, 32)).astype(np.uint8)
    own[ROWS // 2:] = own[:ROWS // 2]   # every descriptor twice in a keyframe: the growth step's ratio test keeps no match
    for k in range(n_kf):
        T = np.eye(4); T[0, 3] = -0.01 * k
        kp = np.zeros(ROWS, V.KP_DTYPE)
        kp["x"] = rng.uniform(0, W, ROWS); kp["y"] = rng.uniform(0, H, ROWS)
        d = rng.integers(0, 256, (ROWS, 32)).astype(np.uint8)
        if k >= n_kf - 3:
            x = (K @ (X[:ROWS] @ T[:3, :3].T + T[:3, 3]).T).T
            kp["x"] = x[:, 0] / x[:, 2]; kp["y"] = x[:, 1] / x[:, 2]
            d = own
        m.add_keyframe(img, kp, d, T)
        assert m.last["n_new"] == 0
    i = np.arange(n_pts)
    k0 = n_kf - 1 - (i // ROWS) % n_kf
    obs_kf = np.stack([k0, (k0 - 1) % n_kf], 1).reshape(-1).astype(np.int32)
    obs_kp = np.repeat(i % ROWS, 2).astype(np.int32)
    off = (np.arange(n_pts + 1) * 2).astype(np.int32)
    z = np.zeros(n_pts, np.int32)
    arrays = (X.astype(np.float32), np.zeros((n_pts, 3), np.uint8), i.astype(np.int32), off, obs_kf, obs_kp)
    m._check(m.lib.mo_map_add_points(m._h, n_pts, *[V._ptr(a) for a in arrays], V._ptr(z - 1), V._ptr(z)))
    m._sync_size()
    T = np.eye(4); T[:3, 3] = [0.02, -0.01, 0.03]
    x = (K @ (X[:ROWS] @ T[:3, :3].T + T[:3, 3]).T).T
    qk = np.zeros(ROWS, V.KP_DTYPE)
    qk["x"] = x[:, 0] / x[:, 2]; qk["y"] = x[:, 1] / x[:, 2]
    qd = own.copy()
    qd[:, 0] ^= rng.integers(0, 8, ROWS).astype(np.uint8)
    pose0 = np.eye(4); pose0[:3, 3] = T[:3, 3] + [0.01, 0.0, 0.0]
    return m, qk, qd, pose0


def _device_ms(ctx):
    st = ctx.stage_times()
    agg = {}
    for name, ms in st:
        agg[name] = agg.get(name, 0.0) + ms
    return sum(agg.values()), agg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", default="16,64")
    ap.add_argument("--points", default="100000,1000000")
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--frustum", action="store_true", help="also time fuse_map_points(frustum=True) on the same map")
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    ctx = V.Context(device=0, max_w=W, max_h=H, max_batch=1)
    ctx.set_host_timing(True)
    for n_kf in [int(x) for x in args.keyframes.split(",")]:
        for n_pts in [int(x) for x in args.points.split(",")]:
            m, qk, qd, pose0 = build(ctx, n_kf, n_pts, rng)
            # (the co-visibility bookkeeping of fuse_map_points is host work on downloaded arrays: the native call is timed alone)
            m.track_local_map(qk, qd, pose0, window=args.window)
            trk = []
            for _ in range(args.calls):
                ok, _, ti = m.track_local_map(qk, qd, pose0, window=args.window)
                trk.append(_device_ms(ctx)[0])
            first = m.fuse_map_points(window=args.window, image_size=(W, H))
            f_ms, f_st = _device_ms(ctx)
            later, stages = [], []
            for _ in range(args.calls):
                info = m.fuse_map_points(window=args.window, image_size=(W, H))
                ms, st = _device_ms(ctx)
                later.append(ms); stages.append(st)
            med = {k: np.median([s.get(k, 0.0) for s in stages]) for k in stages[0]}
            t = float(np.median(trk))
            print("keyframes %3d  rows %d  map_points %8d  window %2d  local %8d  pairs %9d  candidates %9d  | first fuse %.3f ms (%d absorbed, %d gained: %s)"
                  "  later fuse median %.3f ms (%d proposals: %s)  | track device median %.3f ms (ok %s, matches %s)  | fuse / track %.1f first, %.1f later"
                  % (n_kf, ROWS, n_pts, args.window, first["n_local"], first["n_pairs"], first["n_cand"], f_ms, first["n_absorbed"], first["n_gained"],
                     "  ".join("%s %.3f" % kv for kv in f_st.items()), np.median(later), info["n_proposals"],
                     "  ".join("%s %.3f" % kv for kv in med.items()), t, ok, ti["pass_matches"], f_ms / t, np.median(later) / t), flush=True)
            if args.frustum:
                m.fuse_map_points(window=args.window, image_size=(W, H), frustum=True)
                fl, fstages = [], []
                for _ in range(args.calls):
                    fi = m.fuse_map_points(window=args.window, image_size=(W, H), frustum=True)
                    ms, st = _device_ms(ctx)
                    fl.append(ms); fstages.append(st)
                fmed = {k: np.median([s.get(k, 0.0) for s in fstages]) for k in fstages[0]}
                add = np.median(fl) - np.median(later)
                print("keyframes %3d  rows %d  map_points %8d  window %2d  frustum later fuse median %.3f ms (%.3f .. %.3f; %d candidates, %d proposals: %s)"
                      "  | plain later fuse %.3f ms (%.3f .. %.3f)  | frustum adds %.3f ms = %.2f of fuse_prep"
                      % (n_kf, ROWS, n_pts, args.window, np.median(fl), min(fl), max(fl), fi["n_cand"], fi["n_proposals"],
                         "  ".join("%s %.3f" % kv for kv in fmed.items()), np.median(later), min(later), max(later), add, add / fmed["fuse_prep"]), flush=True)
            m.close()
    ctx.close()


if __name__ == "__main__":
    main()
