"""LocalMapper.relocalize_batch against a loop of LocalMapper.relocalize on the same map in the same process.

Maps as tools/bow_rate.py builds them: keyframes of 2000 rows with random descriptors (no growth step finds a model), points injected
with two observations each.  Frame j of a batch is the rows of keyframe j % 8 seen from a pose of its own (descriptors with a few
flipped bits), so every frame has a keyframe to be found in and its own P3P problem.  Per (keyframes, frames), plain and with
preselect=8 (a vocabulary of 1024 words trained on 10^5 random rows): the wall time of one warm batch call and of the loop (median of
`--reps` after a warm-up call; both calls synchronise once per call, so the wall time holds everything), the device time of the batch
as the sum of its stage events where the call's marks fit the 16 a call keeps (2 + 4 per group), and the per-stage medians.  Then the
batch of one against the single call, and the P3P stage at 64 frames x 4 candidates x 512 hypotheses on a 10^6-point map.
A library without mo_map_relocalize_batch (an older build under VSLAM_AMD_LIB) runs the loops only.
python tools/reloc_batch_rate.py   (one MI355X)
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
N_QKF = 8   # keyframes the query frames are drawn from


def build(ctx, n_kf, n_pts, rng):
    """(mapper, X, descriptors of the first N_QKF keyframes)"""
    m = LocalMapper(K, save_every_keyframe=False, context=ctx)
    img = np.zeros((8, 8), np.uint8)
    X = np.column_stack([rng.uniform(-3, 3, n_pts), rng.uniform(-2, 2, n_pts), rng.uniform(4, 10, n_pts)])
    descs = []
    for k in range(n_kf):
        T = np.eye(4); T[0, 3] = -0.01 * k
        kps = np.zeros(ROWS, V.KP_DTYPE)
        x = (K @ (X[:ROWS] + T[:3, 3]).T).T
        kps["x"] = x[:, 0] / x[:, 2]; kps["y"] = x[:, 1] / x[:, 2]
        d = rng.integers(0, 256, (ROWS, 32)).astype(np.uint8)
        m.add_keyframe(img, kps, d, T)
        m.keyframes[-1]["descriptors"] = None   # (the host copy is not needed here: 64 KB per keyframe)
        if k < N_QKF:
            descs.append(d)
    # point i observed by rows i % ROWS of keyframes (i // ROWS) % n_kf and the next one
    i = np.arange(n_pts)
    k0 = (i // ROWS) % n_kf
    obs_kf = np.stack([k0, (k0 + 1) % n_kf], 1).reshape(-1).astype(np.int32)
    obs_kp = np.repeat(i % ROWS, 2).astype(np.int32)
    off = (np.arange(n_pts + 1) * 2).astype(np.int32)
    z = np.zeros(n_pts, np.int32)
    arrays = (X.astype(np.float32), np.zeros((n_pts, 3), np.uint8), i.astype(np.int32), off, obs_kf, obs_kp)
    m._check(m.lib.mo_map_add_points(m._h, n_pts, *[V._ptr(a) for a in arrays], V._ptr(z - 1), V._ptr(z)))
    m._sync_size()
    return m, X, descs


def query(X, descs, j, rng):
    """frame j: keyframe j % N_QKF's rows - row r of keyframe k >= 1 belongs to point (k - 1) * ROWS + r, the lowest that observes it -
    seen from a pose of its own"""
    k = j % len(descs)
    base = max(k - 1, 0) * ROWS
    shift = np.array([0.02 + 0.001 * j, -0.01, 0.03 - 0.0005 * j])
    xq = (K @ (X[base:base + ROWS] + shift).T).T
    qk = np.zeros(ROWS, V.KP_DTYPE)
    qk["x"] = xq[:, 0] / xq[:, 2]; qk["y"] = xq[:, 1] / xq[:, 2]
    qd = descs[k].copy()
    qd[:, 0] ^= rng.integers(0, 8, ROWS).astype(np.uint8)
    return qk, qd


def timed(ctx, call, reps, per_call_stages=False):
    """(wall median ms, device median ms or None, stage medians) of `reps` warm calls; per_call_stages: call() returns its own list of
    stage dicts (a loop of single calls), else the stages are the last call's"""
    call()
    wall, dev, stages = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = call()
        wall.append(1e3 * (time.perf_counter() - t0))
        sts = r if per_call_stages else [ctx.stage_times()]
        tot = {}
        for st in sts:
            for name, ms in st:
                tot[name] = tot.get(name, 0.0) + ms
        stages.append(tot)
        dev.append(sum(tot.values()))
    names = list(stages[0])
    return float(np.median(wall)), float(np.median(dev)), {k: float(np.median([s.get(k, 0.0) for s in stages])) for k in names}


def fmt(st):
    return "  ".join("%s %.3f" % kv for kv in st.items())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", default="64,256,1024")
    ap.add_argument("--frames", default="1,8,64,256")
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--p3p-points", type=int, default=1000000, help="map points of the P3P comparison (0: skipped)")
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    ctx = V.Context(device=0, max_w=640, max_h=480, max_batch=1)
    ctx.set_host_timing(True)
    have_batch = hasattr(ctx.lib, "mo_map_relocalize_batch")
    voc = V.Vocabulary.train([rng.integers(0, 256, (ROWS, 32)).astype(np.uint8) for _ in range(50)], 1024, 10, context=ctx)
    frames_list = [int(x) for x in args.frames.split(",")]

    def loop(m, frames, pre):
        def run():
            out = []
            for kps, d in frames:
                m.relocalize(kps, d, preselect=pre)
                out.append(ctx.stage_times())
            return out
        return run
    for n_kf in [int(x) for x in args.keyframes.split(",")]:
        m, X, descs = build(ctx, n_kf, args.points, rng)
        m.set_vocabulary(voc)
        all_frames = [query(X, descs, j, rng) for j in range(max(frames_list))]
        for pre in (None, 8):
            for nf in frames_list:
                frames = all_frames[:nf]
                lw, ld, lst = timed(ctx, loop(m, frames, pre), args.reps, per_call_stages=True)
                line = "keyframes %4d  %-11s frames %3d  loop: wall %9.3f ms  device %9.3f ms" % (n_kf, "plain" if pre is None else "preselect=8", nf, lw, ld)
                if have_batch:
                    bw, bd, bst = timed(ctx, lambda: m.relocalize_batch(frames, preselect=pre), args.reps)
                    ok = m.relocalize_batch(frames, preselect=pre)[0]
                    groups = m.last_reloc_groups
                    dev = "%9.3f ms" % bd if 2 + 4 * groups <= 16 else "      n/a   "
                    line += "  | batch: wall %9.3f ms  device %s  groups %d  ok %d  | per frame: loop %.3f  batch %.3f ms  ratio %.2fx  | %s" % (
                        bw, dev, groups, int(ok.sum()), lw / nf, bw / nf, lw / bw, fmt(bst))
                else:
                    line += "  | " + fmt(lst)
                print(line, flush=True)
        m.close()
    if args.p3p_points:
        m, X, descs = build(ctx, 64, args.p3p_points, rng)
        frames = [query(X, descs, j, rng) for j in range(64)]
        lw, ld, lst = timed(ctx, loop(m, frames, None), args.reps, per_call_stages=True)
        print("p3p  keyframes 64  map_points %d  64 frames x 4 candidates x 512 hypotheses  loop of 64 calls: reloc_p3p %.3f ms in all (%.3f per call)  "
              "reloc_refine %.3f  wall %.3f ms" % (args.p3p_points, lst["reloc_p3p"], lst["reloc_p3p"] / 64, lst["reloc_refine"], lw), flush=True)
        if have_batch:
            bw, bd, bst = timed(ctx, lambda: m.relocalize_batch(frames), args.reps)
            n_cand = np.mean([len(x["candidates"]) for x in m.relocalize_batch(frames)[2]])
            print("p3p  keyframes 64  map_points %d  64 frames x 4 candidates x 512 hypotheses  one batch: rlb_p3p %.3f ms  rlb_refine %.3f  wall %.3f ms  "
                  "(%.1f of the 4 candidate places filled per frame)  | %s" % (args.p3p_points, bst["rlb_p3p"], bst["rlb_refine"], bw, n_cand, fmt(bst)), flush=True)
        m.close()
    voc.close()
    ctx.close()


if __name__ == "__main__":
    main()
