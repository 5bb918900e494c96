"""Place recognition against the number of keyframes: the bow_* stages of LocalMapper.query_keyframes, relocalize plain against
relocalize(preselect=8), and the training time of a vocabulary.

Maps of 2000-row keyframes built like tools/reloc_rate.py's (random descriptors, 100000 injected points with two observations each;
the query is keyframe 0's rows with a few flipped bits seen from a nearby pose), at 64, 256 and 1024 keyframes.  Vocabularies of 1024
and 4096 words trained on 10^5 random rows (50 images).  Per map and vocabulary: the first query (every keyframe still to be counted),
then the device medians of 10 warm calls, same process, same map: the four bow_* stages, relocalize plain, relocalize(preselect=8).
Then the wall time of Vocabulary.train (10 iterations asked for) at 10^5 and 10^6 rows.
python tools/bow_rate.py   (one MI355X)
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
N_PTS = 100000


def build(ctx, n_kf, rng):
    m = LocalMapper(K, save_every_keyframe=False, context=ctx)
    img = np.zeros((8, 8), np.uint8)
    X = np.column_stack([rng.uniform(-3, 3, N_PTS), rng.uniform(-2, 2, N_PTS), rng.uniform(4, 10, N_PTS)])
    d0 = None
    for k in range(n_kf):
        T = np.eye(4); T[0, 3] = -0.01 * k
        kps = np.zeros(ROWS, V.KP_DTYPE)
        x = (K @ (X[:ROWS] + T[:3, 3]).T).T
        kps["x"] = x[:, 0] / x[:, 2]; kps["y"] = x[:, 1] / x[:, 2]
        d = rng.integers(0, 256, (ROWS, 32)).astype(np.uint8)
        m.add_keyframe(img, kps, d, T)
        m.keyframes[-1]["descriptors"] = None   # (the host copy is not needed here: 64 KB per keyframe)
        d0 = d if k == 0 else d0
    i = np.arange(N_PTS)
    k0 = (i // ROWS) % n_kf
    obs_kf = np.stack([k0, (k0 + 1) % n_kf], 1).reshape(-1).astype(np.int32)
    obs_kp = np.repeat(i % ROWS, 2).astype(np.int32)
    off = (np.arange(N_PTS + 1) * 2).astype(np.int32)
    z = np.zeros(N_PTS, np.int32)
    arrays = (X.astype(np.float32), np.zeros((N_PTS, 3), np.uint8), i.astype(np.int32), off, obs_kf, obs_kp)
    m._check(m.lib.mo_map_add_points(m._h, N_PTS, *[V._ptr(a) for a in arrays], V._ptr(z - 1), V._ptr(z)))
    m._sync_size()
    xq = (K @ (X[:ROWS] + np.array([0.02, -0.01, 0.03])).T).T
    qk = np.zeros(ROWS, V.KP_DTYPE)
    qk["x"] = xq[:, 0] / xq[:, 2]; qk["y"] = xq[:, 1] / xq[:, 2]
    qd = d0.copy()
    qd[:, 0] ^= rng.integers(0, 8, ROWS).astype(np.uint8)
    return m, qk, qd


def medians(ctx, call, n=10):
    """per-stage device medians (ms), their sum's median and the wall median of n warm calls"""
    call()
    wall, dev, stages = [], [], []
    for _ in range(n):
        t0 = time.perf_counter()
        res = call()
        wall.append(time.perf_counter() - t0)
        st = ctx.stage_times()
        dev.append(sum(ms for _, ms in st))
        stages.append(dict(st))
    return {k: float(np.median([s[k] for s in stages])) for k in stages[0]}, float(np.median(dev)), 1e3 * float(np.median(wall)), res


def train_time(ctx, rng, n, words):
    arrays = [rng.integers(0, 256, (ROWS, 32)).astype(np.uint8) for _ in range(n // ROWS)]
    V.Vocabulary.train(arrays[:2], 64, 1, context=ctx).close()   # warm: kernels loaded
    t0 = time.perf_counter()
    v = V.Vocabulary.train(arrays, words, 10, context=ctx)
    dt = time.perf_counter() - t0
    return v, dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", default="64,256,1024")
    ap.add_argument("--words", default="1024,4096")
    ap.add_argument("--train-rows", default="100000,1000000")
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    ctx = V.Context(device=0, max_w=640, max_h=480, max_batch=1)
    ctx.set_host_timing(True)
    vocs = {}
    for n in [int(x) for x in args.train_rows.split(",")]:
        for W in [int(x) for x in args.words.split(",")]:
            v, dt = train_time(ctx, rng, n, W)
            print("train  rows %8d  images %4d  words %5d  iterations %2d  wall %.1f ms" % (n, n // ROWS, W, v.iterations, 1e3 * dt), flush=True)
            if W not in vocs:
                vocs[W] = v
            else:
                v.close()
    for n_kf in [int(x) for x in args.keyframes.split(",")]:
        m, qk, qd = build(ctx, n_kf, rng)
        _, plain_dev, plain_wall, (ok, _, info) = medians(ctx, lambda: m.relocalize(qk, qd))
        print("keyframes %4d  rows %d  map_points %d  relocalize plain: device median %.3f ms  wall median %.3f ms  ok %s keyframe %d inliers %d"
              % (n_kf, ROWS, N_PTS, plain_dev, plain_wall, ok, info["kf_pos"], info["n_inliers"]), flush=True)
        for W, v in vocs.items():
            m.set_vocabulary(v)
            t0 = time.perf_counter()
            m.query_keyframes(qk, qd, 8)
            first = dict(ctx.stage_times())
            first_wall = time.perf_counter() - t0
            st, dev, wall, (pos, sc) = medians(ctx, lambda: m.query_keyframes(qk, qd, 8))
            print("keyframes %4d  words %5d  first query (all keyframes counted): wall %.3f ms  %s" % (n_kf, W, 1e3 * first_wall,
                  "  ".join("%s %.3f" % kv for kv in first.items())), flush=True)
            print("keyframes %4d  words %5d  query_keyframes(8): device median %.3f ms  wall median %.3f ms  first %s  | %s"
                  % (n_kf, W, dev, wall, pos[:3].tolist(), "  ".join("%s %.3f" % kv for kv in st.items())), flush=True)
            st, dev, wall, (ok, _, info) = medians(ctx, lambda: m.relocalize(qk, qd, preselect=8))
            print("keyframes %4d  words %5d  relocalize(preselect=8): device median %.3f ms (plain %.3f ms, %.2fx)  wall median %.3f ms  ok %s keyframe %d "
                  "inliers %d  | %s" % (n_kf, W, dev, plain_dev, plain_dev / dev, wall, ok, info["kf_pos"], info["n_inliers"],
                                        "  ".join("%s %.3f" % kv for kv in st.items())), flush=True)
        m.close()
    ctx.close()


if __name__ == "__main__":
    main()
