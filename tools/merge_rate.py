"""mo_map_absorb, the masked loop candidates and LocalMapper.merge_map on the synthetic maps of tools/kfcull_rate.py: 64 / 1024 keyframes
of 2000 rows, 10^5 / 10^6 points with five observations each.  A map absorbs a map of its own size (its twin: an import of its export).

Per shape, median [min .. max] over the warm calls:
  absorb            wall time of mo_map_absorb into a map whose capacities already hold the sum (nothing is regrown), and its device
                    stages (mo_stage_times): absorb_rows = the two row launches (keypoints, descriptors), absorb_points, absorb_obs;
                    once more into a map of its own size (the keyframe store and the point store are regrown inside the call)
  the floor         in the same run, one device-to-device hipMemcpyAsync between two events of the bytes each stage moves: the rows'
                    (60 bytes a row), the points' (47 bytes a point, its offset among them), the entries' (8 bytes an entry)
  the host route    what there was before: mo_map_export of both maps, the renumbering in numpy (tests/absorb_restatement.absorb) and
                    mo_map_import of the result, each timed on its own (export and import are the code they were)
On the 64-keyframe shape, with a vocabulary trained on the device: mo_map_loop_candidates against mo_map_loop_candidates_among with an
all-ones mask (the same work and the mask launch), and merge_map of an unrelated map of the same size (it does not align: absorb, the
tries, the erase of the absorbed side).
python tools/merge_rate.py [--out profiles/merge_rate.txt]   (one MI355X)
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "visual-slam_amd"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402

import vslam_amd as V  # noqa: E402
from kfcull_rate import ROWS, _stages, build  # noqa: E402
from snapshot_rate import D2D, _hip, _spread, _stage_line  # noqa: E402
from tests import absorb_restatement as AR  # noqa: E402
from vslam_amd import snapshot as S  # noqa: E402


def _d2d(hip, nbytes, calls):
    a, b = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(a), max(nbytes, 16)) == 0 and hip.hipMalloc(C.byref(b), max(nbytes, 16)) == 0
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    assert hip.hipMemset(a, 1, max(nbytes, 16)) == 0 and hip.hipMemset(b, 2, max(nbytes, 16)) == 0   # (written: a page never touched is not a copy's work)
    ev = [C.c_void_p(), C.c_void_p()]
    assert hip.hipEventCreate(C.byref(ev[0])) == 0 and hip.hipEventCreate(C.byref(ev[1])) == 0
    out = []
    for _ in range(calls + 1):
        assert hip.hipDeviceSynchronize() == 0
        assert hip.hipEventRecord(ev[0], None) == 0 and hip.hipMemcpyAsync(b.value, a.value, nbytes, D2D, None) == 0
        assert hip.hipEventRecord(ev[1], None) == 0 and hip.hipEventSynchronize(ev[1]) == 0
        ms = C.c_float(0)
        assert hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]) == 0
        out.append(float(ms.value))
    hip.hipFree(a); hip.hipFree(b)
    for e in ev:
        hip.hipEventDestroy(e)
    return out[1:]


def measure_absorb(ctx, hip, m, calls, say):
    lib = m.lib
    e = m.export_state()
    d = AR.dims_of(e)
    src = S.import_map(lib, ctx.h, e, (0, 0, 0, 0), m._check)
    prm, out = V.MapAbsorbParams(1), V.MapAbsorbOut()
    big = (2 * d["n_kf"], ROWS, 2 * d["n_pts"], 2 * d["n_obs"])
    for cap, tag in ((big, "absorb           "), ((0, 0, 0, 0), "absorb, regrowing")):
        wall, runs = [], []
        for _ in range(calls + 1):
            dst = S.import_map(lib, ctx.h, e, cap, m._check)
            t = time.perf_counter()
            m._check(lib.mo_map_absorb(dst, src, C.byref(prm), C.byref(out)))
            wall.append((time.perf_counter() - t) * 1e3)
            runs.append(_stages(ctx))
            lib.mo_map_destroy(dst)
        say("  %s %s  stages: %s" % (tag, _spread(wall[1:]), _stage_line(runs[1:])))
        if cap is big:
            warm = runs[1:]
    sizes = {"absorb_rows": d["kf_rows"] * 60, "absorb_points": d["n_pts"] * 47, "absorb_obs": d["n_obs"] * 8}
    for name, nbytes in sizes.items():
        floor = _d2d(hip, nbytes, calls)
        st = [r.get(name, 0.0) for r in warm]
        say("  %-14s %s against %s for one device-to-device copy of its %.1f MB: %.0f %% of the copy"
            % (name, _spread(st), _spread(floor), nbytes / 1e6, 100.0 * np.median(floor) / max(np.median(st), 1e-9)))
    # the host route
    t_exp, t_np, t_imp = [], [], []
    for _ in range(3):
        t = time.perf_counter()
        a = m.export_state()
        b = S.export_map(lib, src, m._check)
        t_exp.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        r = AR.absorb(a, b, 1)
        t_np.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        h = S.import_map(lib, ctx.h, r, (0, 0, 0, 0), m._check)
        t_imp.append((time.perf_counter() - t) * 1e3)
        lib.mo_map_destroy(h)
    say("  host route        export of both %s, numpy renumbering %s, import %s (arrays allocated inside export: first touch included)"
        % (_spread(t_exp[1:]), _spread(t_np[1:]), _spread(t_imp[1:])))
    lib.mo_map_destroy(src)


def measure_loop_and_merge(ctx, m, other, calls, say):
    m.train_vocabulary(1024, iters=3)
    n_kf = len(m.keyframes)
    ones = np.ones(n_kf, bool)
    res = {}
    for tag, among in (("plain", None), ("masked", ones)):
        wall, runs = [], []
        for _ in range(calls + 1):
            t = time.perf_counter()
            m.loop_candidates(-1, min_weight=1, among=among)
            wall.append((time.perf_counter() - t) * 1e3)
            runs.append(_stages(ctx))
        res[tag] = (wall[1:], runs[1:])
        say("  loop_candidates, %-6s %s  stages: %s" % (tag, _spread(wall[1:]), _stage_line(runs[1:])))
    dev = lambda runs: [sum(r.values()) for r in runs]
    say("  the mask adds %.3f ms of device time (loop_among %.3f ms) and %.3f ms of wall time at the medians"
        % (np.median(dev(res["masked"][1])) - np.median(dev(res["plain"][1])), np.median([r.get("loop_among", 0.0) for r in res["masked"][1]]),
           np.median(res["masked"][0]) - np.median(res["plain"][0])))
    wall = []
    for _ in range(3):
        t = time.perf_counter()
        r = m.merge_map(other)
        wall.append((time.perf_counter() - t) * 1e3)
        assert not r["aligned"] and len(m.keyframes) == n_kf
    say("  merge_map of an unrelated map of the same size (not aligned after %d tries, taken out again) %s" % (r["tries"], _spread(wall[1:])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64:100000,1024:1000000")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_rate.txt"))
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    ctx = V.Context(device=0, max_w=640, max_h=480, max_batch=1)
    ctx.set_host_timing(True)
    hip = _hip()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    for shape in args.shapes.split(","):
        n_kf, n_pts = (int(x) for x in shape.split(":"))
        m = build(ctx, n_kf, n_pts, rng)
        m._injected = [{"id": 0, "position": np.zeros(3)}]   # (build() hands the points to the library itself, all naming injected dict 0)
        say("keyframes %d  rows %d  map_points %d  observations %d, absorbing a map of the same size" % (n_kf, ROWS, n_pts, m._n_obs))
        measure_absorb(ctx, hip, m, args.calls, say)
        if n_kf <= 64:
            other = build(ctx, n_kf, n_pts, rng)
            other._injected = [{"id": 0, "position": np.zeros(3)}]
            measure_loop_and_merge(ctx, m, other, args.calls, say)
            other.close()
        m.close()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
