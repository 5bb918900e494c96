"""The set form of the local bundle adjustment (LocalMapper.bundle_adjust(free= / local="covisible")) and the observation erase
(LocalMapper.erase_observations) on one MI355X: device time per stage (mo_stage_times), median [min .. max] over the warm calls.

  set form   the maps of tools/ba_rate.py (16 keyframes of 2000 rows, three-view tracks), 10^5 / 10^6 points, the same 10 free keyframes:
             bundle_adjust(window=10), bundle_adjust(free=the last 10) and bundle_adjust(local="covisible", n_best=9, min_weight=1), whose
             set is what the last keyframe shares points with (a smaller problem on these maps: its stages "covis" and "covis_select" are
             what the selection costs).  Calls without steps (max_steps (0, 0): candidates, problem, start cost, classification,
             write; nothing moves, so every call sees the same problem) give the medians of the stages in which the forms differ; one
             full call each on a map built alike gives the whole.
  erase      the maps of tools/kfcull_rate.py (16 / 64 keyframes, 10^5 / 10^6 points, five observations each), a twentieth and a third of
             the entries flagged at random.  In one process, alternating, each on a map of the full size (between two calls every point is
             erased and the same number injected again): erase_observations, erase_map_points of a third of the points, erase_keyframes([1])
             (which does shrink the map by a keyframe per round, as in profiles/ptcull_rate.txt).
             Bytes the entry erase must move: per entry 1 (flag) + 4 (keep) written, 4 read and 4 written by the scan, 4 + 4 (keep, S) and
             8 (okf, okp) read by the copy, 8 written per surviving entry; per point 43 (fields and life record) read and written, 8 read
             (two offsets) and 2 x 4 of S, 4 written.  The other two: the formulas of tools/ptcull_rate.py.  erase_map_points' stage also
             holds its mask upload and flag kernel (it marks no stage in between); erase_observations marks its upload apart.
  sequence   (--sequence) run_frames.py on the 60-frame synthetic sequence of profiles/ptcull_sequence.txt with --cull-points, without
             and with --ba-covisible --ba-erase-outliers: the summary lines and the distance between the tracked poses.
python tools/ba_local_rate.py [--out profiles/ba_local_rate.txt] [--sequence profiles/ba_local_sequence.txt]
"""
import argparse
import contextlib
import io
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "visual-slam_amd"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "visual-slam_amd", "examples")]

import numpy as np  # noqa: E402

import vslam_amd as V  # noqa: E402
import ba_rate  # noqa: E402
from kfcull_rate import HBM_BYTES_PER_S, N_OBS, _stages, build  # noqa: E402
from ptcull_rate import _inject, _spread  # noqa: E402


def _fmt(runs):
    med = {k: float(np.median([r.get(k, 0.0) for r in runs])) for k in runs[0]}
    return "%.3f ms [%.3f .. %.3f] (%s)" % (_spread(runs) + ("  ".join("%s %.3f" % kv for kv in med.items()),))


def _rate(say, label, runs, key, moved):
    med, lo, hi = _spread(runs, (key,))
    b = float(np.median(moved))
    say("  %-34s %s" % (label, _fmt(runs)))
    say("    its rebuild (%s) %.3f ms [%.3f .. %.3f]  must move %.1f MB: %.2f TB/s, %.0f %% of %.0f TB/s"
        % (key, med, lo, hi, b / 1e6, b / (med * 1e-3) / 1e12, 100.0 * b / (med * 1e-3) / HBM_BYTES_PER_S, HBM_BYTES_PER_S / 1e12))


def set_form(ctx, say, points, calls):
    w = np.deg2rad(1.0)
    P = np.eye(4)
    P[:3, :3] = [[np.cos(w), -np.sin(w), 0], [np.sin(w), np.cos(w), 0], [0, 0, 1]]
    P[:3, 3] = [0.03, 0.0, 0.0]
    n_kf, window = 16, 10
    forms = (("window=10", dict(window=window)), ("free=the last 10", dict(free=list(range(n_kf - window, n_kf)))),
             ("covisible, n_best=9", dict(local="covisible", n_best=window - 1, min_weight=1)))
    for n_pts in points:
        say("set form: keyframes %d  map_points %d  (three observations each)" % (n_kf, n_pts))
        prep = {}
        for label, kw in forms:
            m, X, poses = ba_rate.build(ctx, n_kf, n_pts, np.random.default_rng(1))
            for k, kf in enumerate(m.keyframes):
                kf["pose"][:] = P @ poses[k] if k >= n_kf - window else poses[k]
            runs = []
            for _ in range(calls + 1):   # (the first call sizes the buffers: dropped)
                ok, info = m.bundle_adjust(max_steps=(0, 0), **kw)
                runs.append(_stages(ctx))
            prep[label] = _spread(runs[1:])
            say("  %-20s no steps   %s  free %s" % (label, _fmt(runs[1:]), info["free"]))
            ok, info = m.bundle_adjust(**kw)
            st = _stages(ctx)
            say("  %-20s full call  %.3f ms (%s)  steps %s accepted %s, %d of %d edges inliers"
                % (label, sum(st.values()), "  ".join("%s %.3f" % kv for kv in st.items()), info["steps"], info["accepted"], info["n_inliers"], info["n_edges"]))
            m.close()
        base = prep["window=10"]
        for label, _ in forms[1:2]:
            say("  %-20s adds %.3f ms to the call without steps (the window form's own range: %.3f .. %.3f ms)"
                % (label, prep[label][0] - base[0], base[1], base[2]))


def _reset(m, n_pts, rng):
    """every point erased, n_pts injected again: a map of the full size"""
    if m._n_points:
        m.erase_map_points(np.ones(m._n_points, bool))
    _inject(m, n_pts, len(m.keyframes), rng)


def erase(ctx, say, keyframes, points, calls):
    rng = np.random.default_rng(2)
    for n_kf in keyframes:
        for n_pts in points:
            m = build(ctx, n_kf, n_pts, rng)
            say("erase: keyframes %d  map_points %d  observations %d" % (n_kf, n_pts, m._n_obs))
            runs = {k: [] for k in ("obs 1/20", "obs 1/3", "points 1/3", "keyframe")}
            moved = {k: [] for k in runs}
            for _ in range(calls + 1):
                for key, frac in (("obs 1/20", 1 / 20), ("obs 1/3", 1 / 3)):
                    no = m._n_obs
                    r = m.erase_observations(rng.random(no) < frac)
                    runs[key].append(_stages(ctx))
                    moved[key].append(no * (1 + 4 + 8 + 8 + 8) + 8 * r["n_obs"] + n_pts * (2 * 43 + 8 + 8 + 4))
                    _reset(m, n_pts, rng)
                no = m._n_obs
                remap = m.erase_map_points(np.arange(n_pts) % 3 == 0)
                runs["points 1/3"].append(_stages(ctx))
                kept = int((remap >= 0).sum())
                moved["points 1/3"].append(n_pts * 32 + kept * (2 * 43 + 8) + 16 * m._n_obs)
                _reset(m, n_pts, rng)
                no = m._n_obs
                m.erase_keyframes([1])
                runs["keyframe"].append(_stages(ctx))
                moved["keyframe"].append(n_pts * (2 * 43 + 12) + 16 * no + 8 * m._n_obs)
                _reset(m, n_pts, rng)
            _rate(say, "erase_observations, a twentieth", runs["obs 1/20"][1:], "obs_erase", moved["obs 1/20"][1:])
            _rate(say, "erase_observations, a third", runs["obs 1/3"][1:], "obs_erase", moved["obs 1/3"][1:])
            _rate(say, "erase_map_points, a third", runs["points 1/3"][1:], "ptcull_erase", moved["points 1/3"][1:])
            _rate(say, "erase_keyframes([1]) (%d left)" % len(m.keyframes), runs["keyframe"][1:], "kfcull_erase", moved["keyframe"][1:])
            m.close()


def sequence(path):
    import run_frames
    base = ["--max-frames", "60", "--keyframe-every", "5", "--track-map", "--frustum", "--local-ba", "--ba-window", "8", "--grow-neighbours", "--fuse",
            "--cull-points", "--cull-keyframes"]
    lines = ["run_frames.py --map PATH " + " ".join(base) + " on the synthetic sequence (one MI355X), without and with --ba-covisible --ba-erase-outliers", ""]
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for tag, extra in (("without", []), ("with", ["--ba-covisible", "--ba-erase-outliers"])):
            buf = io.StringIO()
            old = sys.argv
            sys.argv = ["run_frames.py", "--map", os.path.join(tmp, tag + ".ply")] + base + extra
            try:
                with contextlib.redirect_stdout(buf):
                    state, poses, n_map = run_frames.main()
            finally:
                sys.argv = old
            out[tag] = poses
            keep = ("frames in", "map statistics", "bundle adjustment", "growth from", "point cull:", "keyframe cull:", "fusion:", "bundle adjust over")
            lines += ["%-8s %s" % (tag, ln) for ln in buf.getvalue().splitlines() if any(k in ln for k in keep)]
            lines.append("")
    a, b = out["without"], out["with"]
    n = min(len(a), len(b))
    ca = np.array([(-R.T @ t).reshape(3) for R, t in a[:n]]); cb = np.array([(-R.T @ t).reshape(3) for R, t in b[:n]])
    step = float(np.median(np.linalg.norm(np.diff(ca, axis=0), axis=1)))
    d = np.linalg.norm(ca - cb, axis=1) / step
    rot = np.array([np.linalg.norm(a[i][0] - b[i][0]) for i in range(n)])
    lines.append("tracked poses: %d and %d; camera centres apart by %.3g of a trajectory step at the median, %.3g at most; rotations (Frobenius) %.3g at the "
                 "median, %.3g at most" % (len(a), len(b), np.median(d), d.max(), np.median(rot), rot.max()))
    print("\n".join(lines), flush=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", default="16,64")
    ap.add_argument("--points", default="100000,1000000")
    ap.add_argument("--calls", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ba_local_rate.txt"))
    ap.add_argument("--sequence", default="", help="PATH: also run the 60-frame sequence with and without the two flags and write PATH")
    args = ap.parse_args()
    ctx = V.Context(device=0, max_w=640, max_h=480, max_batch=1)
    ctx.set_host_timing(True)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    points = [int(x) for x in args.points.split(",")]
    set_form(ctx, say, points, args.calls)
    erase(ctx, say, [int(x) for x in args.keyframes.split(",")], points, args.calls)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if args.sequence:
        sequence(args.sequence)


if __name__ == "__main__":
    main()
