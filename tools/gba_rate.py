"""Global bundle adjustment (mo_map_global_ba) against the size of the map, on the maps of tools/posegraph_rate.py (tools/bow_rate.py:
2000-row keyframes, point i observed from the keyframes (i // 2000) % n_kf and the next, so every point has two edges; with 10^5 points
the first 51 positions take part, with 10^6 all of them, each row then seen by several points).  The keypoint of a row is the projection
of ONE of the points that observe it, so most residuals start far beyond the Huber width: a workload for the clock, not a map to admire.
Position 0 is fixed.

Per size, three calls in a row on the map as the call before left it (an accepted call moves the points and kP, so no two calls see the
same map; the figures are normalised per step and per iteration): device time per call (the stages gba_prep, gba_steps, gba_write:
device events around the stage, the host's looks at the result block included), per Levenberg-Marquardt step and per conjugate-gradient
iteration (the stage gba_steps over the counts, so the iteration figure carries its share of the linearisation and the
back-substitution), iterations per step, the wall time; then one call of one step, whose iteration count says how many of the enqueued
iteration launches returned at their first read (the host looks every 32 iterations); the bytes one iteration has to move (every array
once per pass, the gathers per edge) against gba_steps per iteration.  --local: on an 18-keyframe map (16 free keyframes) one step of
mo_map_bundle_adjust beside one step of this call.
python tools/gba_rate.py   (one MI355X; VSLAM_AMD_LIB names another build of the library)
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "visual-slam_amd"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402

import vslam_amd as V  # noqa: E402
import bow_rate  # noqa: E402

CG_CHUNK = 32   # GBA_CG_CHUNK of map_gba.hip


def build(ctx, n_kf, n_pts):
    bow_rate.N_PTS = n_pts
    try:
        return bow_rate.build(ctx, n_kf, np.random.default_rng(1))[0]
    finally:
        bow_rate.N_PTS = 100000


def timed(ctx, call):
    t0 = time.perf_counter()
    ok, info = call()
    wall = 1e3 * (time.perf_counter() - t0)
    return info, dict(ctx.stage_times()), wall


def iteration_bytes(n_points, n_edges, n_free):
    """what one iteration has to move: pass (a) per edge its position, keypoint and information (20 B) and the 48 B of p it gathers, per
    point X, V^-1, the held flag and q (97 B); pass (b) per edge its list entry, point, position, keypoint and information (28 B) and the
    X and q it gathers (48 B), per keyframe H_kk, p, S p and the partial dot (392 B); the update 6 vectors of 6 n_free."""
    a = n_edges * (20 + 48) + n_points * 97
    b = n_edges * (28 + 48) + n_free * 392
    return a + b + 6 * 48 * n_free


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", default="64,256,1024")
    ap.add_argument("--points", default="100000,1000000")
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--max-steps", type=int, default=10)
    ap.add_argument("--max-cg", type=int, default=200)
    ap.add_argument("--local", action="store_true")
    args = ap.parse_args()
    ctx = V.Context(device=0, max_w=640, max_h=480, max_batch=1)
    ctx.set_host_timing(True)
    print("library: %s" % V.LIB_PATH, flush=True)
    m = build(ctx, 18, 36000)                                   # (loads the kernels: every timed call below is warm)
    m.global_bundle_adjust(fixed=[0, 1], max_steps=2)
    m.bundle_adjust(window=16, max_steps=(1, 0))
    m.close()
    if args.local:
        for rep in range(3):
            m = build(ctx, 18, 36000)
            li, ls, lw = timed(ctx, lambda: m.bundle_adjust(window=16, max_steps=(1, 0)))
            m.close()
            m = build(ctx, 18, 36000)
            gi, gs, gw = timed(ctx, lambda: m.global_bundle_adjust(fixed=[0, 1], max_steps=1, max_cg=args.max_cg))
            m.close()
            print("18 keyframes, 36000 points, one step: mo_map_bundle_adjust free %d edges %d: ba_round0 %.3f ms (wall %.3f)  |  mo_map_global_ba free %d edges %d: "
                  "gba_steps %.3f ms, %d iterations (wall %.3f)" % (li["n_free"], li["n_edges"], ls.get("ba_round0", 0.0), lw, gi["n_free"], gi["n_edges"],
                                                                     gs.get("gba_steps", 0.0), gi["cg_iters"], gw), flush=True)
    for n_pts in [int(x) for x in args.points.split(",")]:
        for n_kf in [int(x) for x in args.keyframes.split(",")]:
            t0 = time.perf_counter()
            m = build(ctx, n_kf, n_pts)
            t_build = time.perf_counter() - t0
            for call in range(args.calls):
                info, st, wall = timed(ctx, lambda: m.global_bundle_adjust(max_steps=args.max_steps, max_cg=args.max_cg))
                steps, its = max(info["steps"], 1), max(info["cg_iters"], 1)
                dev = sum(st.values())
                by = iteration_bytes(info["n_points"], info["n_edges"], info["n_free"])
                print("keyframes %4d points %7d call %d: free %d points %d edges %d | device %.3f ms (prep %.3f steps %.3f write %.3f) wall %.3f ms | steps %d accepted %d "
                      "iterations %d (%.1f per step) | %.3f ms per step, %.1f us per iteration | %.2f MB per iteration -> %.1f GB/s | cost %.6g -> %.6g"
                      % (n_kf, n_pts, call, info["n_free"], info["n_points"], info["n_edges"], dev, st.get("gba_prep", 0.0), st.get("gba_steps", 0.0),
                         st.get("gba_write", 0.0), wall, info["steps"], info["accepted"], info["cg_iters"], info["cg_iters"] / steps, st.get("gba_steps", 0.0) / steps,
                         1e3 * st.get("gba_steps", 0.0) / its, by / 1e6, by / (1e6 * st.get("gba_steps", 1.0) / its), info["cost"][0], info["cost"][1]), flush=True)
            info, st, wall = timed(ctx, lambda: m.global_bundle_adjust(max_steps=1, max_cg=args.max_cg))
            enq = min(args.max_cg, -(-max(info["cg_iters"], 1) // CG_CHUNK) * CG_CHUNK)
            print("keyframes %4d points %7d one step: %d iterations of %d enqueued: %.0f %% of the iteration launches returned at their first read; gba_steps %.3f ms "
                  "(map built in %.1f s)" % (n_kf, n_pts, info["cg_iters"], enq, 100.0 * (enq - info["cg_iters"]) / enq, st.get("gba_steps", 0.0), t_build), flush=True)
            m.close()
    ctx.close()


if __name__ == "__main__":
    main()
