"""LocalMapper.create_new_map_points against the number of keyframes and the map size, next to one fuse_map_points call and one
track_local_map call on the same map.

The maps of tools/fuse_rate.py - keyframes of 2000 rows, keypoints uniform in the image, random descriptors, points with two
observations each on row i % 2000 - with two changes that give the call work: the keyframes stand 0.1 apart (fuse_rate's 0.01 is below
the parallax gate), and the points observe keyframe positions outside the window only (1 + j and j, j = (i // 2000) % (n_kf - window
- 2)), so every row of the target and of the `window` neighbours is free: 2000 x 2000 x window epipolar tests, the most a keyframe of
2000 rows can ask for.  The rows r of the last three keyframes sit at the projection of one feature r each and carry one descriptor
(each descriptor on two rows far apart, so that no growth step of add_keyframe matches): the first call makes up to 2000 points with
three observations, the later calls find those rows owned and search the rest.
Per (keyframes, map points): the device time of the first call and the median of the later calls (sums of the stage events, with the
stages), the search stage's share, one fuse_map_points call and the median of warm track_local_map calls on the map the first call left.
python tools/grow_rate.py   (one MI355X; under rocprofv3 --kernel-trace --stats for the per-kernel times)
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
STEP = 0.1


def build(ctx, n_kf, n_pts, window, rng):
    m = LocalMapper(K, save_every_keyframe=False, context=ctx, capacity=(max(n_kf, 2), ROWS, n_pts + ROWS, 2 * n_pts + 16 * ROWS))
    img = np.zeros((H, W), np.uint8)
    X = np.column_stack([rng.uniform(-3, 3, n_pts), rng.uniform(-2, 2, n_pts), rng.uniform(4, 10, n_pts)])
    F = np.column_stack([rng.uniform(-1.5, 1.5, ROWS) + STEP * (n_kf - 2), rng.uniform(-1.2, 1.2, ROWS), rng.uniform(5, 10, ROWS)])   # the features
    own = rng.integers(0, 256, (ROWS, 32)).astype(np.uint8)
    own[ROWS // 2:] = own[:ROWS // 2]   # every descriptor twice in a keyframe: the growth step's ratio test keeps no match
    for k in range(n_kf):
        T = np.eye(4); T[0, 3] = -STEP * k
        kp = np.zeros(ROWS, V.KP_DTYPE)
        kp["x"] = rng.uniform(0, W, ROWS); kp["y"] = rng.uniform(0, H, ROWS)
        d = rng.integers(0, 256, (ROWS, 32)).astype(np.uint8)
        if k >= n_kf - 3:
            x = (K @ (F @ T[:3, :3].T + T[:3, 3]).T).T
            kp["x"] = x[:, 0] / x[:, 2]; kp["y"] = x[:, 1] / x[:, 2]
            d = own
        m.add_keyframe(img, kp, d, T)
        assert m.last["n_new"] == 0
    i = np.arange(n_pts)
    span = max(n_kf - min(window, n_kf - 1) - 2, 1)
    k0 = 1 + (i // ROWS) % span
    obs_kf = np.stack([k0, k0 - 1], 1).reshape(-1).astype(np.int32)
    obs_kp = np.repeat(i % ROWS, 2).astype(np.int32)
    off = (np.arange(n_pts + 1) * 2).astype(np.int32)
    z = np.zeros(n_pts, np.int32)
    arrays = (X.astype(np.float32), np.zeros((n_pts, 3), np.uint8), i.astype(np.int32), off, obs_kf, obs_kp)
    m._check(m.lib.mo_map_add_points(m._h, n_pts, *[V._ptr(a) for a in arrays], V._ptr(z - 1), V._ptr(z)))
    m._sync_size()
    T = np.eye(4); T[:3, 3] = [0.02 - STEP * (n_kf - 2), -0.01, 0.03]
    x = (K @ (F @ T[:3, :3].T + T[:3, 3]).T).T
    qk = np.zeros(ROWS, V.KP_DTYPE)
    qk["x"] = x[:, 0] / x[:, 2]; qk["y"] = x[:, 1] / x[:, 2]
    qd = own.copy()
    qd[:, 0] ^= rng.integers(0, 8, ROWS).astype(np.uint8)
    pose0 = T.copy(); pose0[0, 3] += 0.01
    return m, qk, qd, pose0


def _device_ms(ctx):
    agg = {}
    for name, ms in ctx.stage_times():
        agg[name] = agg.get(name, 0.0) + ms
    return sum(agg.values()), agg


def _native_grow(m, window):
    """the native call alone (the co-visibility bookkeeping of create_new_map_points is host work on downloaded arrays)"""
    import ctypes as C
    n_kf = len(m.keyframes)
    poses = np.array([np.asarray(kf["pose"], np.float64)[:3, :4].reshape(12) for kf in m.keyframes])
    Kf = np.ascontiguousarray(m.camera_matrix, np.float64).reshape(9)
    point = np.full(ROWS, -1, np.int32)
    prm = V.MapGrowParams(window, 50, 1.2, 3.84, 5.991, 0.9998, 1.8, 100.0)
    out = V.MapGrowOut(point.ctypes.data, None)
    m._check(m.lib.mo_map_grow(m._h, V._ptr(Kf), V._ptr(poses), C.byref(prm), C.byref(out)))
    m._version += 1; m._cache = None; m._sync_size()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", default="16,64")
    ap.add_argument("--points", default="100000,1000000")
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--calls", type=int, default=5)
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    ctx = V.Context(device=0, max_w=W, max_h=H, max_batch=1)
    ctx.set_host_timing(True)
    for n_kf in [int(x) for x in args.keyframes.split(",")]:
        for n_pts in [int(x) for x in args.points.split(",")]:
            m, qk, qd, pose0 = build(ctx, n_kf, n_pts, args.window, rng)
            first = _native_grow(m, args.window)
            g_ms, g_st = _device_ms(ctx)
            later, stages = [], []
            for _ in range(args.calls):
                out = _native_grow(m, args.window)
                ms, st = _device_ms(ctx)
                later.append(ms); stages.append(st)
            med = {k: np.median([s.get(k, 0.0) for s in stages]) for k in stages[0]}
            fi = m.fuse_map_points(window=args.window, image_size=(W, H))
            f_ms, _ = _device_ms(ctx)
            m.track_local_map(qk, qd, pose0, window=args.window)
            trk = []
            for _ in range(args.calls):
                ok, _, ti = m.track_local_map(qk, qd, pose0, window=args.window)
                trk.append(_device_ms(ctx)[0])
            t = float(np.median(trk))
            print("keyframes %3d  rows %d  map_points %8d  window %2d  neighbours %2d  free %4d  epipolar passes %9d  accepted %6d  matches %6d"
                  "  | first grow %.3f ms (%d new points, %d observations: %s; search %.0f %%)  later grow median %.3f ms (%d free, %d new: %s; search %.0f %%)"
                  "  | one fuse %.3f ms (%d pairs, %d proposals)  track device median %.3f ms (ok %s)  | grow / fuse %.2f first, %.2f later  grow / track %.2f first"
                  % (n_kf, ROWS, n_pts, args.window, first.n_neighbours, first.n_free, first.n_epi, first.n_accepted, first.n_matches, g_ms, first.n_new,
                     first.n_obs_new, "  ".join("%s %.3f" % kv for kv in g_st.items()), 100.0 * g_st.get("grow_search", 0.0) / max(g_ms, 1e-9),
                     np.median(later), out.n_free, out.n_new, "  ".join("%s %.3f" % kv for kv in med.items()),
                     100.0 * med.get("grow_search", 0.0) / max(float(np.median(later)), 1e-9), f_ms, fi["n_pairs"], fi["n_proposals"], t, ok,
                     g_ms / f_ms, np.median(later) / f_ms, g_ms / t), flush=True)
            m.close()
    ctx.close()


if __name__ == "__main__":
    main()
