"""The snapshot of the device map (mo_map_export / mo_map_import, LocalMapper.save_state / load_state) on the synthetic maps of
tools/kfcull_rate.py: 64 / 1024 keyframes of 2000 rows, 10^5 / 10^6 points with five observations each; and, per keyframe count, a map
of keyframes of 1500 .. 2000 rows without points, where three of four keypoint runs are not 16-byte aligned in the packed array.

Per (keyframes, map points), median [min .. max] over the warm calls:
  export            wall time of mo_map_export into arrays that were touched before, and its device stages (mo_stage_times):
                    snapshot_pack = the two gather launches (keypoints, descriptors) with the upload of their two small tables,
                    snapshot_copy = the copies to the host
  import            wall time of mo_map_import (a new map: its allocations included) and its stages: snapshot_copy = every copy from the
                    host, snapshot_unpack = the two scatter launches behind them
  the floor         in the same run, plain hipMemcpy calls moving the same bytes between the same kind of memory: one device-to-host copy
                    per snapshot array into touched pageable arrays (export), one host-to-device copy per array (import), and for the
                    pack launches one device-to-device hipMemcpyAsync of the packed rows' bytes between two events (the rows are read once and
                    written once; the stages are event spans too)
  save_state        wall time to an uncompressed .npz under --dir (export included), the file's size; load_state the same file back
python tools/snapshot_rate.py [--out profiles/snapshot_rate.txt]   (one MI355X)
"""
import argparse
import ctypes as C
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "visual-slam_amd"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402

import vslam_amd as V  # noqa: E402
from kfcull_rate import K, ROWS, _stages, build  # noqa: E402
from ptcull_rate import _inject  # noqa: E402
from vslam_amd import snapshot as S  # noqa: E402
from vslam_amd.mapper import LocalMapper  # noqa: E402


def _hip():
    """the HIP runtime this process already runs on (by the path it was loaded from: a second copy would be a second runtime)"""
    with open("/proc/self/maps") as f:
        paths = {ln.split()[-1] for ln in f if "libamdhip64" in ln}
    hip = C.CDLL(sorted(paths)[0])
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventDestroy.argtypes = [C.c_void_p]
    return hip


H2D, D2H, D2D = 1, 2, 3


def _spread(v):
    return "%.3f ms [%.3f .. %.3f]" % (float(np.median(v)), min(v), max(v))


def _stage_line(runs):
    names = list(runs[0])
    return "  ".join("%s %.3f" % (k, float(np.median([r.get(k, 0.0) for r in runs]))) for k in names)


def measure(ctx, hip, m, calls, tmp, say):
    lib = m.lib
    d = V.MapSnapshotDims()
    m._check(lib.mo_map_snapshot_dims(m._h, C.byref(d)))
    arrays = {"dims": S._dims_to_vector(d)}
    for name, (dtype, shape) in S.array_specs(arrays["dims"]).items():
        arrays[name] = np.zeros(shape, dtype)
        if arrays[name].size:
            arrays[name].reshape(-1).view(np.uint8).fill(0)   # (touched: no first-touch page faults inside a copy)
    s = S._struct_of(arrays)
    sizes = [a.nbytes for k, a in arrays.items() if k != "dims" and a.nbytes]
    total = sum(sizes)
    row_bytes = arrays["kf_kps"].nbytes + arrays["kf_desc"].nbytes
    say("  snapshot %.1f MB in %d arrays, %.1f MB of them keyframe rows" % (total / 1e6, len(sizes), row_bytes / 1e6))
    # export
    wall, runs = [], []
    for _ in range(calls + 1):
        t = time.perf_counter()
        m._check(lib.mo_map_export(m._h, C.byref(s)))
        wall.append((time.perf_counter() - t) * 1e3)
        runs.append(_stages(ctx))
    say("  export            %s  stages: %s" % (_spread(wall[1:]), _stage_line(runs[1:])))
    pack = [r.get("snapshot_pack", 0.0) for r in runs[1:]]
    # import
    wall_i, runs_i = [], []
    for _ in range(calls + 1):
        h = C.c_void_p()
        t = time.perf_counter()
        m._check(lib.mo_map_import(ctx.h, C.byref(s), 0, 0, 0, 0, C.byref(h)))
        wall_i.append((time.perf_counter() - t) * 1e3)
        runs_i.append(_stages(ctx))
        lib.mo_map_destroy(h)
    say("  import            %s  stages: %s" % (_spread(wall_i[1:]), _stage_line(runs_i[1:])))
    unpack = [r.get("snapshot_unpack", 0.0) for r in runs_i[1:]]
    # the floor: plain hipMemcpy of the same bytes
    dev = C.c_void_p()
    assert hip.hipMalloc(C.byref(dev), max(total, 16)) == 0
    dev2 = C.c_void_p()
    assert hip.hipMalloc(C.byref(dev2), max(row_bytes, 16)) == 0
    host = [a for k, a in arrays.items() if k != "dims" and a.nbytes]
    f_d2h, f_h2d, f_d2d = [], [], []
    ev = [C.c_void_p(), C.c_void_p()]
    assert hip.hipEventCreate(C.byref(ev[0])) == 0 and hip.hipEventCreate(C.byref(ev[1])) == 0
    for _ in range(calls + 1):
        t = time.perf_counter()
        at = 0
        for a in host:
            assert hip.hipMemcpy(a.ctypes.data, dev.value + at, a.nbytes, D2H) == 0
            at += a.nbytes
        f_d2h.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        at = 0
        for a in host:
            assert hip.hipMemcpy(dev.value + at, a.ctypes.data, a.nbytes, H2D) == 0
            at += a.nbytes
        f_h2d.append((time.perf_counter() - t) * 1e3)
        assert hip.hipDeviceSynchronize() == 0
        assert hip.hipEventRecord(ev[0], None) == 0 and hip.hipMemcpyAsync(dev2.value, dev.value, row_bytes, D2D, None) == 0
        assert hip.hipEventRecord(ev[1], None) == 0 and hip.hipEventSynchronize(ev[1]) == 0
        ms = C.c_float(0)
        assert hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]) == 0
        f_d2d.append(float(ms.value))
    hip.hipFree(dev); hip.hipFree(dev2)
    for e in ev:
        hip.hipEventDestroy(e)
    say("  floor, export     %s  (%d hipMemcpy device -> host, %.2f GB/s)" % (_spread(f_d2h[1:]), len(host), total / np.median(f_d2h[1:]) / 1e6))
    say("  floor, import     %s  (%d hipMemcpy host -> device, %.2f GB/s)" % (_spread(f_h2d[1:]), len(host), total / np.median(f_h2d[1:]) / 1e6))
    say("  floor, pack       %s  (one hipMemcpyAsync device -> device of the rows' %.1f MB between two events, as the stages are timed)"
        % (_spread(f_d2d[1:]), row_bytes / 1e6))
    say("  export is %.2f x its floor, import %.2f x; snapshot_pack %s is %.2f x and snapshot_unpack %s %.2f x the device-to-device copy: "
        "the pack launches reach %.0f %% and the unpack launches %.0f %% of the copy floor"
        % (np.median(wall[1:]) / np.median(f_d2h[1:]), np.median(wall_i[1:]) / np.median(f_h2d[1:]), _spread(pack), np.median(pack) / np.median(f_d2d[1:]),
           _spread(unpack), np.median(unpack) / np.median(f_d2d[1:]), 100.0 * np.median(f_d2d[1:]) / max(np.median(pack), 1e-9),
           100.0 * np.median(f_d2d[1:]) / max(np.median(unpack), 1e-9)))
    # the file (build() and _inject() hand the points to the library themselves, all naming injected dict 0: the mapper gets that dict)
    m._injected = [{"id": 0, "position": np.zeros(3)}]
    path = os.path.join(tmp, "state.npz")
    t_save, t_load = [], []
    for _ in range(3):
        t = time.perf_counter()
        m.save_state(path)
        t_save.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        l = LocalMapper.load_state(path, context=ctx)
        t_load.append((time.perf_counter() - t) * 1e3)
        l.close()
    say("  save_state        %s  file %.1f MB" % (_spread(t_save[1:]), os.path.getsize(path) / 1e6))
    say("  load_state        %s" % _spread(t_load[1:]))
    os.remove(path)


def build_uneven(ctx, n_kf, rng):
    """n_kf keyframes of 1500 .. 2000 rows each and no points: the packed offset of a keyframe is a multiple of 4 rows for one in four,
    so three of four keypoint runs take k_snap_rows' 4-byte path (the descriptor runs always take the 16-byte one)"""
    m = LocalMapper(K, save_every_keyframe=False, context=ctx, capacity=(n_kf, ROWS, 16, 32))
    img = np.zeros((480, 640), np.uint8)
    for k in range(n_kf):
        n = int(rng.integers(1500, ROWS + 1))
        T = np.eye(4); T[0, 3] = -0.01 * k
        m.add_keyframe(img, np.zeros(n, V.KP_DTYPE), rng.integers(0, 256, (n, 32)).astype(np.uint8), T)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", default="64,1024")
    ap.add_argument("--points", default="100000,1000000")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--dir", default=tempfile.gettempdir())
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snapshot_rate.txt"))
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    ctx = V.Context(device=0, max_w=640, max_h=480, max_batch=1)
    ctx.set_host_timing(True)
    hip = _hip()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    for n_kf in [int(x) for x in args.keyframes.split(",")]:
        m, have = None, 0
        for n_pts in sorted(int(x) for x in args.points.split(",")):
            if m is None:
                m = build(ctx, n_kf, n_pts, rng)
            else:
                _inject(m, n_pts - have, n_kf, rng)   # (the same keyframes, more points)
            have = n_pts
            say("keyframes %d  rows %d  map_points %d  observations %d" % (n_kf, ROWS, n_pts, m._n_obs))
            measure(ctx, hip, m, args.calls, args.dir, say)
        m.close()
        m = build_uneven(ctx, n_kf, rng)
        off = np.concatenate([[0], np.cumsum([kf._rows for kf in m.keyframes])])[:-1]
        say("keyframes %d  rows 1500 .. %d, uneven  map_points 0  (%d of %d keypoint runs start at a multiple of 4 rows: the others copy in 4-byte units)"
            % (n_kf, ROWS, int((off % 4 == 0).sum()), n_kf))
        measure(ctx, hip, m, args.calls, args.dir, say)
        m.close()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
