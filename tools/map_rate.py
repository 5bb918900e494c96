"""add_keyframe against map size (PLY deferred), beside the reference's per-keyframe loops restated on the host.

A map of n points, two observations each, all reprojecting onto keypoint 0 of keyframes 0 and 1 (they survive every cull), then ten
more keyframes of 2000 keypoints with random descriptors (a growth step that finds no model, so the map stays at n).  Per size:
  device   wall time of LocalMapper.add_keyframe (median of 10) and the device time of its stages (sum of the stage events)
  host     tests/map_restatement.RefMapper.cull_map_points on the same map: the reference's cull loop and per-keyframe list rebuild
           (one call; --host-max caps the sizes it runs at, the loop takes ~10-30 us per point)
python tools/map_rate.py [--host-max N]   (one MI355X; under rocprofv3 --kernel-trace --stats for the per-kernel times)
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

K = np.array([[320.0, 0, 320.0], [0, 320.0, 240.0], [0, 0, 1.0]])


def host_time(n, xy0):
    from tests.map_restatement import RefMapper
    ref = RefMapper(K)
    for k in range(4):
        ref.keyframes.append({"id": k, "image": None, "xy": xy0, "pose": np.eye(4), "P": K @ np.hstack((np.eye(3), np.zeros((3, 1)))),
                              "map_points": []})
    pos = np.float32([(xy0[0, 0] - 320) / 320, (xy0[0, 1] - 240) / 320, 1.0])
    ref.map_points = [{"id": i, "position": pos, "color": np.zeros(3, np.uint8), "observed_keyframes": {0: 0, 1: 0}} for i in range(n)]
    t0 = time.perf_counter()
    ref.cull_map_points()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,10000,100000,1000000")
    ap.add_argument("--host-max", type=int, default=10 ** 6, help="largest map the host restatement is timed on (0: none)")
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    ctx = V.Context(device=0, max_w=640, max_h=480, max_batch=1)
    ctx.set_host_timing(True)
    for n in [int(x) for x in args.sizes.split(",")]:
        m = LocalMapper(K, save_every_keyframe=False, context=ctx)
        kps = np.zeros(2000, V.KP_DTYPE)
        kps["x"] = rng.uniform(0, 640, 2000); kps["y"] = rng.uniform(0, 480, 2000)
        img = np.zeros((480, 640), np.uint8)
        for k in range(3):
            m.add_keyframe(img, kps, rng.integers(0, 256, (2000, 32)).astype(np.uint8), np.eye(4))
        x0, y0 = kps["x"][0], kps["y"][0]
        xyz = np.tile(np.float32([(x0 - 320) / 320, (y0 - 240) / 320, 1.0]), (n, 1))
        off = (np.arange(n + 1) * 2).astype(np.int32)
        okf = np.tile(np.int32([0, 1]), n)
        okp = np.zeros(2 * n, np.int32)
        z = np.zeros(n, np.int32)
        arrays = (xyz, np.zeros((n, 3), np.uint8), np.arange(n, dtype=np.int32), off, okf, okp)
        m._check(m.lib.mo_map_add_points(m._h, n, *[V._ptr(a) for a in arrays], V._ptr(z - 1), V._ptr(z)))
        m._sync_size()
        wall, dev = [], []
        for k in range(10):
            d = rng.integers(0, 256, (2000, 32)).astype(np.uint8)
            t0 = time.perf_counter()
            m.add_keyframe(img, kps, d, np.eye(4))
            wall.append(time.perf_counter() - t0)
            dev.append(sum(ms for _, ms in ctx.stage_times()))
        assert len(m.map_points) == n
        line = "map_points %8d  add_keyframe wall median %.3f ms (min %.3f), device stages median %.3f ms" % (
            n, 1e3 * np.median(wall), 1e3 * min(wall), np.median(dev))
        if n <= args.host_max:
            xy0 = np.stack([kps["x"], kps["y"]], 1).astype(np.float32)
            h = host_time(n, xy0)
            line += "  |  host restatement cull + lists %.1f ms (%.1f us / point)" % (1e3 * h, 1e6 * h / n)
        print(line, flush=True)
        m.close()
    ctx.close()


if __name__ == "__main__":
    main()
