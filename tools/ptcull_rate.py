"""The life of a map point (LocalMapper.note_tracking / cull_map_points / erase_map_points) on the synthetic maps of tools/kfcull_rate.py:
16 / 64 keyframes of 2000 rows, 10^5 / 10^6 points with five observations each.

Per (keyframes, map points), device time per stage (mo_stage_times), median [min .. max] over the warm calls:
  note_tracking              the whole map local (window=0), 2000 keypoints matched to random points; plain and frustum=True
  cull_map_points(erase=0)   the decision alone: every point's ratio is low by then, two thirds are protected
  cull_map_points()          the decision and the erase of the unprotected third in one chain; between two calls the removed number of
                             points is injected again and noted four times, so that every call removes a third of a map of the same size
  erase_keyframes([1])       the yardstick: the keyframe erase's rebuild on the same map (it moves the same fields); every call takes one
                             keyframe's observations out, so its bytes shrink from call to call - the bytes of the median call are shown
For both rebuilds: the bytes they must move and the share of 8 TB/s that gives.
  point erase     per point 8 read by the two scans, 8 written by them, 12 read and 4 (remap) written by the scatter; per survivor its
                  fields (27) and life record (16) read and written and its offset read and written (8); per surviving entry 8 read, 8 written
  keyframe erase  per point 43 read and written and 12 for the count, the offsets and their scan; per entry 8 read by the count and 8 by
                  the scatter; per surviving entry 8 written
python tools/ptcull_rate.py [--out profiles/ptcull_rate.txt]   (one MI355X)
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "visual-slam_amd"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402

import vslam_amd as V  # noqa: E402
from kfcull_rate import HBM_BYTES_PER_S, N_OBS, ROWS, _stages, build  # noqa: E402


def _inject(m, n, n_kf, rng):
    """n more points like build()'s: five observations at distinct keyframes"""
    first = rng.integers(0, n_kf, n)
    step = rng.integers(1, max((n_kf - 1) // (N_OBS - 1), 1) + 1, (n, N_OBS - 1))
    obs_kf = ((first[:, None] + np.concatenate([np.zeros((n, 1), np.int64), np.cumsum(step, 1)], 1)) % n_kf).reshape(-1).astype(np.int32)
    obs_kp = rng.integers(0, ROWS, n * N_OBS).astype(np.int32)
    off = (np.arange(n + 1) * N_OBS).astype(np.int32)
    z = np.zeros(n, np.int32)
    X = np.column_stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(4, 10, n)]).astype(np.float32)
    arrays = (X, np.zeros((n, 3), np.uint8), np.arange(n, dtype=np.int32), off, obs_kf, obs_kp)
    m._check(m.lib.mo_map_add_points(m._h, n, *[V._ptr(a) for a in arrays], V._ptr(z - 1), V._ptr(z)))
    m._version += 1; m._cache = None
    m._sync_size()


def _spread(runs, keys=None):
    tot = [sum(v for k, v in r.items() if keys is None or k in keys) for r in runs]
    return float(np.median(tot)), float(min(tot)), float(max(tot))


def _fmt(runs):
    med = {k: float(np.median([r.get(k, 0.0) for r in runs])) for k in runs[0]}
    return "%.3f ms [%.3f .. %.3f] (%s)" % (_spread(runs) + ("  ".join("%s %.3f" % kv for kv in med.items()),))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", default="16,64")
    ap.add_argument("--points", default="100000,1000000")
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ptcull_rate.txt"))
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    ctx = V.Context(device=0, max_w=640, max_h=480, max_batch=1)
    ctx.set_host_timing(True)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    pose = np.eye(4)
    empty = {"point": np.zeros(0, np.int32), "inlier": np.zeros(0, bool)}
    for n_kf in [int(x) for x in args.keyframes.split(",")]:
        for n_pts in [int(x) for x in args.points.split(",")]:
            m = build(ctx, n_kf, n_pts, rng)
            say("keyframes %d  rows %d  map_points %d  observations %d" % (n_kf, ROWS, n_pts, m._n_obs))
            info = {"point": rng.integers(0, n_pts, ROWS).astype(np.int32), "inlier": rng.random(ROWS) < 0.7}
            for frustum in (False, True):
                runs = []
                for _ in range(args.calls + 1):   # (the first call sizes the buffers: dropped)
                    cnt = m.note_tracking(pose, info, window=0, frustum=frustum, image_size=(640, 480))
                    runs.append(_stages(ctx))
                say("  note_tracking%s   %s  local %d  seen %d  matched %d" % (", frustum" if frustum else "         ", _fmt(runs[1:]), cnt["n_local"],
                                                                                cnt["n_seen"], cnt["n_matched"]))
            protect = (np.arange(n_pts) % 3 != 0).astype(np.uint8)
            runs = []
            for _ in range(args.calls + 1):
                removed, ci = m.cull_map_points(erase=False, protect=protect)
                runs.append(_stages(ctx))
            say("  cull_map_points(erase=0)  %s  tested %d  reasons %s  removed %d" % (_fmt(runs[1:]), ci["n_tested"], ci["n_reason"], ci["n_removed"]))
            assert abs(ci["n_removed"] - n_pts / 3) < 0.02 * n_pts   # (a third: the unprotected points less the few that were found often enough)
            runs, moved = [], []
            for _ in range(args.calls + 1):
                before = m._n_obs
                removed, ci = m.cull_map_points(protect=protect)
                st = _stages(ctx)
                runs.append(st)
                kept, okept = ci["n_points"], ci["n_obs"]
                assert abs(len(removed) - n_pts / 3) < 0.02 * n_pts and before == N_OBS * n_pts
                moved.append(n_pts * 32 + kept * (2 * 43 + 8) + 16 * okept)
                _inject(m, len(removed), n_kf, rng)
                for _ in range(4):
                    m.note_tracking(pose, empty, window=0, image_size=(640, 480))
            med, lo, hi = _spread(runs[1:], ("ptcull_erase",))
            b = float(np.median(moved[1:]))
            say("  cull_map_points()         %s  removed %d of %d" % (_fmt(runs[1:]), len(removed), n_pts))
            say("    its rebuild (ptcull_erase) %.3f ms [%.3f .. %.3f]  must move %.1f MB: %.2f TB/s, %.0f %% of %.0f TB/s"
                % (med, lo, hi, b / 1e6, b / (med * 1e-3) / 1e12, 100.0 * b / (med * 1e-3) / HBM_BYTES_PER_S, HBM_BYTES_PER_S / 1e12))
            runs, moved = [], []
            for _ in range(args.calls + 1):
                before = m._n_obs
                m.erase_keyframes([1])
                runs.append(_stages(ctx))
                moved.append(n_pts * (2 * 43 + 12) + 16 * before + 8 * m._n_obs)
            med, lo, hi = _spread(runs[1:], ("kfcull_erase",))
            b = float(np.median(moved[1:]))
            say("  erase_keyframes([1])      %s" % _fmt(runs[1:]))
            say("    its rebuild (kfcull_erase) %.3f ms [%.3f .. %.3f]  must move %.1f MB: %.2f TB/s, %.0f %% of %.0f TB/s"
                % (med, lo, hi, b / 1e6, b / (med * 1e-3) / 1e12, 100.0 * b / (med * 1e-3) / HBM_BYTES_PER_S, HBM_BYTES_PER_S / 1e12))
            m.close()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
