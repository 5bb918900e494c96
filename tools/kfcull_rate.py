"""The keyframe cull by ORB-SLAM2's rule (LocalMapper.cull_keyframes / erase_keyframes) on synthetic maps: 16 / 64 / 256 keyframes of 2000
rows, 10^5 / 10^6 points with five observations each at keyframes drawn at random (octaves 0 .. 3), so that every keyframe is a candidate of
the last one: the longest walk a map of that size can ask for.

Per (keyframes, map points), device time per stage (mo_stage_times), medians over the warm calls:
  decide, one workgroup      cull_keyframes(erase=False, walk=1): covis, kfcull_order, kfcull_list, kfcull_walk
  decide, launch/candidate   cull_keyframes(erase=False, walk=2): the same with kfcull_steps in place of kfcull_walk
  covisibility()             the matrix alone
then, each once (they change the map; the buffers they use are warm):
  erase_keyframes([1])       the rebuild alone (its first call on the map sizes three buffers and is not reported; position 2 follows)
  cull_keyframes()           decide + erase in one chain, with what it removed
  add_observations           one mo_map_add_observations call of 2000 entries on the same map: the same rebuild (wall time, it marks no stages)
For the rebuild: the bytes it must move (the point fields read and written, the observation arrays read by the count and again by the
scatter, the surviving observations written) and the share of 8 TB/s that gives.
python tools/kfcull_rate.py [--out profiles/kfcull_rate.txt]   (one MI355X)
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "visual-slam_amd"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402

import vslam_amd as V  # noqa: E402
from vslam_amd.mapper import LocalMapper  # noqa: E402

ROWS, N_OBS = 2000, 5
K = np.array([[500.0, 0, 320.0], [0, 500.0, 240.0], [0, 0, 1.0]])
HBM_BYTES_PER_S = 8.0e12
RATIO = 0.5   # (at 0.9 these maps remove nothing: the erase would have nothing to rebuild)


def build(ctx, n_kf, n_pts, rng):
    m = LocalMapper(K, save_every_keyframe=False, context=ctx, capacity=(max(n_kf, 2), ROWS, n_pts, (N_OBS + 1) * n_pts))
    img = np.zeros((480, 640), np.uint8)
    for k in range(n_kf):
        T = np.eye(4); T[0, 3] = -0.01 * k
        kp = np.zeros(ROWS, V.KP_DTYPE)
        kp["octave"] = rng.integers(0, 4, ROWS)
        m.add_keyframe(img, kp, rng.integers(0, 256, (ROWS, 32)).astype(np.uint8), T)
    i = np.arange(n_pts)
    first = rng.integers(0, n_kf, n_pts)
    step = rng.integers(1, max((n_kf - 1) // (N_OBS - 1), 1) + 1, (n_pts, N_OBS - 1))   # distinct keyframes: increasing offsets below n_kf
    obs_kf = ((first[:, None] + np.concatenate([np.zeros((n_pts, 1), np.int64), np.cumsum(step, 1)], 1)) % n_kf).reshape(-1).astype(np.int32)
    obs_kp = rng.integers(0, ROWS, n_pts * N_OBS).astype(np.int32)
    off = (np.arange(n_pts + 1) * N_OBS).astype(np.int32)
    z = np.zeros(n_pts, np.int32)
    X = np.column_stack([rng.uniform(-3, 3, n_pts), rng.uniform(-2, 2, n_pts), rng.uniform(4, 10, n_pts)]).astype(np.float32)
    arrays = (X, np.zeros((n_pts, 3), np.uint8), i.astype(np.int32), off, obs_kf, obs_kp)
    m._check(m.lib.mo_map_add_points(m._h, n_pts, *[V._ptr(a) for a in arrays], V._ptr(z - 1), V._ptr(z)))
    m._sync_size()
    return m


def _stages(ctx):
    agg = {}
    for name, ms in ctx.stage_times():
        agg[name] = agg.get(name, 0.0) + ms
    return agg


def _median(runs):
    return {k: float(np.median([r.get(k, 0.0) for r in runs])) for k in runs[0]}


def _fmt(st):
    return "%.3f ms (%s)" % (sum(st.values()), "  ".join("%s %.3f" % kv for kv in st.items()))


def _rebuild_bytes(n_pts, n_obs_before, n_obs_after):
    return n_pts * (2 * 27 + 3 * 4) + 2 * 8 * n_obs_before + 8 * n_obs_after


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", default="16,64,256")
    ap.add_argument("--points", default="100000,1000000")
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kfcull_rate.txt"))
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    ctx = V.Context(device=0, max_w=640, max_h=480, max_batch=1)
    ctx.set_host_timing(True)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    for n_kf in [int(x) for x in args.keyframes.split(",")]:
        for n_pts in [int(x) for x in args.points.split(",")]:
            m = build(ctx, n_kf, n_pts, rng)
            say("keyframes %d  rows %d  map_points %d  observations %d  (ratio %.2f, min_weight 15)" % (n_kf, ROWS, n_pts, m._n_obs, RATIO))
            res = {}
            for walk, label in ((1, "decide, one workgroup   "), (2, "decide, launch/candidate")):
                runs = []
                for _ in range(args.calls + 1):   # (the first call sizes the buffers: dropped)
                    removed, info = m.cull_keyframes(erase=False, walk=walk, ratio=RATIO)
                    runs.append(_stages(ctx))
                res[walk] = (removed, info)
                say("  %s  %s  candidates %d  removed %d" % (label, _fmt(_median(runs[1:])), info["n_local"], info["n_removed"]))
            assert res[1][0] == res[2][0] and all(np.array_equal(res[1][1][k], res[2][1][k]) for k in ("pos", "n_points", "n_redundant", "removed"))
            runs = []
            for _ in range(args.calls + 1):
                m.covisibility()
                runs.append(_stages(ctx))
            say("  covisibility()            %s" % _fmt(_median(runs[1:])))
            m.erase_keyframes([1])
            for what in ("erase_keyframes([2])", "cull_keyframes()"):
                before = m._n_obs
                if what.startswith("erase"):
                    m.erase_keyframes([2]); n_rem = 1
                else:
                    removed, info = m.cull_keyframes(ratio=RATIO); n_rem = len(removed)
                st = _stages(ctx)
                b = _rebuild_bytes(n_pts, before, m._n_obs)
                t = st.get("kfcull_erase", 0.0) * 1e-3
                say("  %-24s  %s  removed %d  observations %d -> %d  | rebuild must move %.1f MB: %.2f TB/s, %.0f %% of %.0f TB/s"
                    % (what, _fmt(st), n_rem, before, m._n_obs, b / 1e6, b / t / 1e12 if t else 0.0, 100.0 * b / t / HBM_BYTES_PER_S if t else 0.0,
                       HBM_BYTES_PER_S / 1e12))
            pt = rng.integers(0, n_pts, ROWS).astype(np.int32)
            wall = []
            for pos in (0, len(m.keyframes) - 1):   # (two different keyframes: the second call is warm)
                t0 = time.perf_counter()
                m.add_observations(pos, pt)
                wall.append(time.perf_counter() - t0)
            say("  add_observations          wall %.3f ms (warm call, with its synchronisation and the size query)" % (1e3 * wall[1]))
            m.close()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
