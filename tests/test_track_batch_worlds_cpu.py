"""The worlds of tests/track_batch_worlds.py, checked in numpy on the restatement alone: what tests/test_gpu_track_batch_regimes.py asks
of the device is only worth asking when these worlds reach the code it is about - a local list longer than two rounds of a frame's
workgroups with matches in every round, a list that is not the identity, matches on both sides of k_tb_scan's chunk boundary and in
the last partial block, and ties that only the lower index resolves.  These are conditions, not measurements: a seed that fails one is
changed, the condition is not.  No GPU."""
import numpy as np
import pytest

from tests import track_restatement as TR
from tests import track_batch_worlds as TB


@pytest.mark.parametrize("window", [0, 1, 3])
def test_the_vectorised_local_map_is_the_restatement(window):
    """on a 3000-point instance of the scan world's construction (the same builder, smaller parameters)"""
    w = TB.small_scan_world()
    rep, ref, n_local = TR.local_map(w.obs_off, w.obs_kf, w.obs_kp, w.kf_desc, w.kf_oct, window)
    vrep, vref, vn = TB.scan_local_map(w, window)
    assert vn == n_local and vref == ref and vrep.dtype == rep.dtype and np.array_equal(vrep, rep)
    assert all(type(a) is type(b) for a, b in zip(vref, ref))
    n = len(w.xyz)
    print("window %d: %d of %d points local" % (window, n_local, n))
    in3 = int((~w.not_local).sum())   # what the construction puts into the window of 3
    assert 0 < in3 < n and n_local == {0: n, 3: in3}.get(window, n_local) and (window != 1 or 0 < n_local < in3)


def test_the_grid_world_walks_three_rounds_with_matches_in_each():
    w = TB.grid_world()
    rep, ref, n_local = TB.grid_local_map()
    frames, pose0, at = TB.grid_batch()
    nf = len(frames)
    # lb_per_frame = min(pblocks, max(128, ceil(2048 / nf))) = 128: a workgroup's rounds cover 32768 list entries each
    pblocks = (len(w.xyz) + 255) // 256
    assert nf >= 17 and min(pblocks, max(128, -(-2048 // nf))) * 256 == TB.ROUND
    assert n_local > 2 * TB.ROUND and n_local % 256 != 0 and n_local < len(w.xyz) * 0.7   # three rounds, the last partial; a third not local
    pos = TB.list_positions(ref)
    assert int(pos.max()) == n_local - 1
    r = TB.grid_restated(1025)
    ps = r["passes"][0]
    assert r["n_local"] == n_local and ps["radius"] == 15.0
    per_round, lp = TB.matches_per_round(ps["point"], pos)
    matched = ps["point"][ps["point"] >= 0]
    print("n_local %d, n = 1025: %d matches, %s in the three rounds, %d candidates" % (n_local, ps["matches"], per_round, ps["cand"]))
    assert len(per_round) == 3 and min(per_round) >= 1 and sum(per_round) == ps["matches"] >= 20
    assert not (lp == matched).any()          # no matched point stands at its own index: list[j] is not j
    # the other frames: distinct row counts, one empty, the 1500-keypoint cell in the largest
    ns = [len(k) for k, _ in frames]
    assert sorted(ns)[0] == 0 and sorted(ns)[1] == 1 and max(ns) == TB.GRID_STRIDE and all(200 <= n <= 900 for n in ns if n not in TB.GRID_NS and n)
    k5 = frames[at[5000]][0]
    W, H = w.image_size
    cells = (np.clip(k5["y"] * 48 / H, 0, 47).astype(int) * 64 + np.clip(k5["x"] * 64 / W, 0, 63).astype(int))
    assert np.bincount(cells).max() >= 1500


def test_the_scan_world_reaches_both_chunks_the_last_block_and_the_ties():
    w = TB.scan_world()
    n = len(w.xyz)
    pblocks = (n + 255) // 256
    assert pblocks == 1027 and n % 256 == 37 and w.ranges == [(0, 256), (262144 - 300, 262144), (262144, 262144 + 300), (1026 * 256, n)]
    frames, pose0, marks, (rep, ref, n_local), r = TB.scan_case()
    # the launch arithmetic the GPU test names: 1 frame - 1027 list blocks per frame in a launch of 1032; 2 frames - 1024; 3 frames - 683,
    # fewer than the list has blocks, so the end of the list is reached in a second round only
    lbpf = [min(pblocks, max(128, -(-2048 // nf))) for nf in (1, 2, 3)]
    assert lbpf == [1027, 1024, 683] and [-(-(l * nf) // 8) * 8 - l * nf for l, nf in zip(lbpf, (1, 2, 3))] == [5, 0, 7]
    assert 683 * 256 < n_local < 0.7 * n
    counts = np.add.reduceat(np.array([x is not None for x in ref], np.int64), np.arange(0, n, 256))
    assert len(set(counts.tolist())) > 10 and counts[:1024].sum() > 0 and counts[1024:].sum() > 0   # per-block counts differ; both chunks hold local points
    pos = TB.list_positions(ref)
    ps = r["passes"][0]
    matched = ps["point"][ps["point"] >= 0]
    in_range = np.bincount(w.range_of(matched) + 1, minlength=5)
    print("n_local %d of %d, first frame: %d keypoints, %d candidates, %d matches, per range %s (outside %d)"
          % (n_local, n, len(frames[0][0]), ps["cand"], ps["matches"], in_range[1:].tolist(), in_range[0]))
    assert in_range[0] == 0 and (in_range[1:] >= 1).all() and ps["matches"] >= 20 and ps["radius"] == 15.0
    assert not w.not_local[matched].any() and not (pos[matched] == matched)[matched >= 256].any()
    assert (pos[matched[w.range_of(matched) >= 1]] >= 683 * 256).all()   # with 3 frames: reached in the second round
    # the duplicate points: both project to one place with one descriptor, one keypoint there; the lower index takes it
    lo, hi = w.dup_points
    assert lo < 256 and hi >= 1026 * 256 and np.array_equal(w.xyz[lo], w.xyz[hi]) and np.array_equal(rep[lo], rep[hi]) and ref[lo] == ref[hi]
    q = marks["dup_points"]
    assert ps["point"][q] == lo and hi not in matched and np.array_equal(frames[0][1][q], rep[lo]) and ps["dist"][q] == 0
    # the duplicate keypoint: the lower row takes the point at distance 0, the higher stays unmatched
    q1, q2 = marks["dup_kp"]
    k0, d0 = frames[0]
    assert q1 < q2 and k0[q1] == k0[q2] and np.array_equal(d0[q1], d0[q2]) and np.array_equal(d0[q1], rep[w.dup_kp_point])
    assert ps["point"][q1] == w.dup_kp_point and ps["dist"][q1] == 0 and ps["point"][q2] == -1
    # the tie rules are what decides: with the order of either pair turned round the restatement would answer differently, so a kernel
    # that took the higher index would not equal it
    for f in frames[1:]:
        assert 20 <= len(f[0]) != len(k0)


def test_the_scan_world_with_every_point_local_fills_1027_list_blocks():
    """window = 0 on the same map: the list is the identity and has 1027 blocks, so with 2 frames (1024 list blocks per frame) blocks
    1024 .. 1026 are reached in a second round; the last range's matches stand there"""
    w = TB.scan_world()
    frames, pose0, marks, (rep, ref, n_local), r = TB.scan_case(0)
    assert n_local == len(w.xyz)
    matched = r["passes"][0]["point"][r["passes"][0]["point"] >= 0]
    assert (matched >= 1024 * 256).sum() >= 1 and (matched < 256).sum() >= 1
    assert w.not_local[matched].any()   # points the window of 3 leaves out are matched here
