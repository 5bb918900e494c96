"""tests/fuse_restatement.py on hand-worked maps of three keyframes: the rules of mo_map_fuse (include/vslam_amd.h) pinned without a
device.  Camera f = 100, centre (50, 50), image 100 x 100; keyframe k looks down z from x = 0.1 k, so a point (a, b, 10) lands at
(50 + 10 a - k, 50 + 10 b): every number below is exact in binary."""
import numpy as np

from tests import fuse_restatement as FR

K = np.array([[100.0, 0, 50.0], [0, 100.0, 50.0], [0, 0, 1.0]])
W = H = 100


def _poses():
    out = []
    for k in range(3):
        T = np.eye(4)
        T[0, 3] = -0.1 * k
        out.append(T)
    return out


def _desc(code, flips=()):
    """32 bytes of one Walsh pattern (any two 128 bits apart), the given bits flipped"""
    d = np.full(32, (0x00, 0x0F, 0x33, 0x55)[code], np.uint8)
    for b in flips:
        d[b // 8] ^= np.uint8(1 << (b % 8))
    return d


def _run(kfs, xyz, obs, **kw):
    """kfs: per keyframe [(x, y, descriptor)]; obs: per point [(key, row)] as stored"""
    kf_xy = [np.array([[p[0], p[1]] for p in kf], np.float32).reshape(-1, 2) for kf in kfs]
    kf_desc = [np.array([p[2] for p in kf], np.uint8).reshape(-1, 32) for kf in kfs]
    kf_oct = [np.zeros(len(kf), np.int32) for kf in kfs]
    a = FR.as_arrays(xyz, obs, ids=np.arange(len(obs)) + 100)
    out, into, cnt, margins = FR.fuse(a, FR.store_P(K, _poses()), kf_xy, kf_oct, kf_desc, W, H, window=0, **kw)
    assert margins["min"] > 1e-9, margins
    assert cnt["n_points"] == len(out["id"]) == len(out["obs_off"]) - 1 and cnt["n_obs"] == len(out["obs_kf"]) == out["obs_off"][-1]
    return FR.lists_of(out), into.tolist(), cnt, out


def _counts(cnt, **want):
    assert {k: cnt[k] for k in want} == want, cnt


D0 = _desc(0)
LINE = [[(50, 50, D0)], [(49, 50, D0)], [(48, 50, D0)]]   # the point (0, 0, 10) in the three keyframes


def test_simple_merge():
    """A {0, 1} and B {1, 2} at one place: each finds the other's keypoint in the keyframe it lacks.  Two observations each: the lower
    index survives and takes B's observation of keyframe 2; B's observation of keyframe 1 is already there."""
    lists, into, cnt, out = _run(LINE, [[0, 0, 10]] * 2, [[(0, 0), (1, 0)], [(1, 0), (2, 0)]])
    assert lists == [[(0, 0), (1, 0), (2, 0)]] and into == [0, 0]
    _counts(cnt, n_targets=3, n_local=2, n_pairs=2, n_cand=2, n_proposals=2, n_gained=0, n_edges=2, n_absorbed=1, n_points=1, n_obs=3)
    assert out["id"].tolist() == [100]


def test_free_row_gain():
    """keyframe 2 holds the keypoint, no point observes it: A gains (2, 0)"""
    lists, into, cnt, _ = _run(LINE, [[0, 0, 10]], [[(0, 0), (1, 0)]])
    assert lists == [[(0, 0), (1, 0), (2, 0)]] and into == [0]
    _counts(cnt, n_pairs=1, n_cand=1, n_proposals=1, n_gained=1, n_edges=0, n_absorbed=0, n_points=1, n_obs=3)


def test_two_points_claim_one_free_row():
    """A and B 1.25 px apart, one free keypoint in keyframe 2 at A's projection: B's descriptor is 3 bits from it, A's 13: the lower
    distance wins over the lower index.  C and D likewise with equal descriptors: distance 0 both, the lower index wins."""
    db = _desc(1)
    da, df = _desc(1, range(100, 110)), _desc(1, (3, 4, 5))
    dc = _desc(2)
    kfs = [[(50, 50, da), (51.25, 50, db), (50, 70, dc), (51.25, 70, dc)],
           [(49, 50, da), (50.25, 50, db), (49, 70, dc), (50.25, 70, dc)],
           [(48, 50, df), (48, 70, dc)]]
    xyz = [[0, 0, 10], [0.125, 0, 10], [0, 2, 10], [0.125, 2, 10]]
    obs = [[(0, r), (1, r)] for r in range(4)]
    lists, into, cnt, _ = _run(kfs, xyz, obs)
    assert lists == [[(0, 0), (1, 0)], [(0, 1), (1, 1), (2, 0)], [(0, 2), (1, 2), (2, 1)], [(0, 3), (1, 3)]]
    assert into == [0, 1, 2, 3]
    _counts(cnt, n_pairs=4, n_cand=4, n_proposals=4, n_gained=2, n_edges=0, n_absorbed=0, n_points=4, n_obs=10)


CHAIN_XYZ = [[0, 0, 10], [0.1875, 0, 10], [0.375, 0, 10]]   # 1.875 px apart: neighbours pass the chi2 gate (3.52), A and C (3.75 px) miss r = 3


def test_chain_survivor_by_index_when_counts_tie():
    """A in keyframe 0, B in 1, C in 2, one observation each: A - B and B - C are merge edges, A - C is not; one component, A survives.
    Four proposals: A and C both claim B's keypoint (1, 0) at distance 0, the lower index wins, so three rows have a winner"""
    kfs = [[(50, 50, D0)], [(50.875, 50, D0)], [(51.75, 50, D0)]]
    lists, into, cnt, out = _run(kfs, CHAIN_XYZ, [[(0, 0)], [(1, 0)], [(2, 0)]])
    assert lists == [[(0, 0), (1, 0), (2, 0)]] and into == [0, 0, 0]
    _counts(cnt, n_pairs=6, n_cand=6, n_proposals=4, n_gained=0, n_edges=3, n_absorbed=2, n_points=1, n_obs=3)
    assert out["id"].tolist() == [100] and np.array_equal(out["xyz"][0], np.float32(CHAIN_XYZ[0]))


def test_chain_survivor_by_observation_count():
    """C also observes keyframe 0 (row 1): two observations against one each, C survives; A's observation of keyframe 0 meets C's own
    and is dropped, B's of keyframe 1 is taken.  B's projection into keyframe 0 is 1.875 px from both rows: the lower row, A's"""
    kfs = [[(50, 50, D0), (53.75, 50, D0)], [(50.875, 50, D0)], [(51.75, 50, D0)]]
    lists, into, cnt, out = _run(kfs, CHAIN_XYZ, [[(0, 0)], [(1, 0)], [(2, 0), (0, 1)]])
    assert lists == [[(2, 0), (0, 1), (1, 0)]] and into == [0, 0, 0]
    _counts(cnt, n_pairs=5, n_cand=5, n_proposals=4, n_gained=0, n_edges=3, n_absorbed=2, n_points=1, n_obs=3)
    assert out["id"].tolist() == [102] and np.array_equal(out["xyz"][0], np.float32(CHAIN_XYZ[2]))


def test_same_position_conflict_is_dropped():
    """A {0: 0, 1: 0} and B {1: 1, 2: 0}: both observe keyframe 1, at different rows.  The survivor keeps its own; (1, 1) is dropped"""
    kfs = [[(50, 50, D0)], [(49, 50, D0), (50, 50, D0)], [(48, 50, D0)]]
    lists, into, cnt, _ = _run(kfs, [[0, 0, 10]] * 2, [[(0, 0), (1, 0)], [(1, 1), (2, 0)]])
    assert lists == [[(0, 0), (1, 0), (2, 0)]] and into == [0, 0]
    _counts(cnt, n_pairs=2, n_proposals=2, n_edges=2, n_absorbed=1, n_obs=3)


def test_stale_and_negative_keys():
    """A stored (0, 0), (7, 3) - no keyframe 7 - and (-2, 0) = keyframe 1; B stored (1, 5) - no row 5 - and (-1, 0) = keyframe 2.  A has
    two valid observations, B one: A survives with its bytes as stored; B's valid entry arrives written (2, 0), its stale one is gone"""
    lists, into, cnt, _ = _run(LINE, [[0, 0, 10]] * 2, [[(0, 0), (7, 3), (-2, 0)], [(1, 5), (-1, 0)]])
    assert lists == [[(0, 0), (7, 3), (-2, 0), (2, 0)]] and into == [0, 0]
    _counts(cnt, n_local=2, n_pairs=3, n_cand=3, n_proposals=3, n_gained=0, n_edges=3, n_absorbed=1, n_points=1, n_obs=4)


def test_nothing_to_fuse_and_the_gates():
    """a point every keyframe observes: no pair.  A free keypoint 2.5 px off: inside r, outside chi2 (6.25 > 5.991): a candidate, no
    proposal; with chi2 = 7 it is gained.  A free keypoint 60 bits off: over max_dist"""
    lists, into, cnt, out = _run(LINE, [[0, 0, 10]], [[(0, 0), (1, 0), (2, 0)]])
    assert lists == [[(0, 0), (1, 0), (2, 0)]]
    _counts(cnt, n_targets=3, n_local=1, n_pairs=0, n_cand=0, n_proposals=0, n_gained=0, n_edges=0, n_absorbed=0, n_points=1, n_obs=3)
    off = [LINE[0], LINE[1], [(50.5, 50, D0)]]
    lists, _, cnt, _ = _run(off, [[0, 0, 10]], [[(0, 0), (1, 0)]])
    assert lists == [[(0, 0), (1, 0)]]
    _counts(cnt, n_pairs=1, n_cand=1, n_proposals=0, n_points=1, n_obs=2)
    lists, _, cnt, _ = _run(off, [[0, 0, 10]], [[(0, 0), (1, 0)]], chi2=7.0)
    assert lists == [[(0, 0), (1, 0), (2, 0)]] and cnt["n_gained"] == 1
    far = [LINE[0], LINE[1], [(48, 50, _desc(0, range(60)))]]
    lists, _, cnt, _ = _run(far, [[0, 0, 10]], [[(0, 0), (1, 0)]])
    assert lists == [[(0, 0), (1, 0)]] and cnt["n_proposals"] == 0
    lists, _, cnt, _ = _run(far, [[0, 0, 10]], [[(0, 0), (1, 0)]], max_dist=60)
    assert lists == [[(0, 0), (1, 0), (2, 0)]]


def test_co_visibility_delta_of_a_merge():
    """A {0, 1} + B {1, 2} -> {0, 1, 2}: the pair (0, 1) and (1, 2) were counted once each before and once after; (0, 2) is new"""
    a = FR.as_arrays([[0, 0, 10]] * 2, [[(0, 0), (1, 0)], [(1, 0), (2, 0)]])
    kf_xy = [np.array([[p[0], p[1]] for p in kf], np.float32) for kf in LINE]
    out, into, _, _ = FR.fuse(a, FR.store_P(K, _poses()), kf_xy, [np.zeros(1, np.int32)] * 3, [D0[None]] * 3, W, H, window=0)
    assert FR.co_visibility_delta(a, out, into, [1, 1, 1]) == {(0, 2): 1}


def test_library_exports_the_call():
    import vslam_amd as V
    lib = V.load_library()
    assert hasattr(lib, "mo_map_fuse") and "mo_map_fuse" in V.SIGNATURES
    assert C_sizes() == (48, 56)


def C_sizes():
    import ctypes as C

    import vslam_amd as V
    return C.sizeof(V.MapFuseParams), C.sizeof(V.MapFuseOut)


# ---- keyframes past 1024 rows: the worlds and row cases of tests/fuse_worlds.py, which tests/test_gpu_fuse.py runs on the device ---------
def test_large_split_world_is_put_together_again():
    """rows [921, 1117, 1924, 1830]: 1693 points in two, every one put together again; the observation sets are the unsplit world's"""
    from tests import fuse_worlds as FW
    from tests.test_grow_cpu import ratio_survivors
    w, unsplit, n_split = FW.large_split_world()
    assert w.counts.tolist() == [921, 1117, 1924, 1830] and n_split == 1693 and set(ratio_survivors(w)) == {0}
    out, into, cnt, margins = FW.restate_world(w, window=0)
    assert margins["min"] > 1e-7 > 1e-9, margins
    assert cnt["n_absorbed"] == n_split and cnt["n_points"] == len(unsplit.obs) and cnt["n_gained"] == 0 and cnt["n_edges"] == 2 * n_split
    u = FW.world_inputs(unsplit)[0]
    assert sorted(map(sorted, FW.obs_sets(out, w.counts))) == sorted(map(sorted, FW.obs_sets(u, w.counts)))
    # with the rows behind the first 1024 of every keyframe missing, fewer points find their other half
    cut = ([x[:FW.TILE] for x in w.kf_xy], [x[:FW.TILE] for x in w.kf_oct], [x[:FW.TILE] for x in w.kf_desc], FW.world_inputs(w)[1])
    assert FW.restate_world(w, lists=cut, window=0)[2]["n_absorbed"] < n_split - 100


def test_large_stale_split_world():
    """six keyframes, position 1 removed, keys decorated: rows [548, 693, 1087, 1785, 1656]; read without the position -> slot table the
    restatement gives another map"""
    from orbslam2.utils import compute_projection_matrix
    from tests import fuse_worlds as FW
    from tests.test_grow_cpu import ratio_survivors
    w, unsplit, n_split = FW.large_split_world(stale=True)
    assert w.counts.tolist() == [548, 693, 1087, 1785, 1656] and w.survivors == [0, 2, 3, 4, 5] and set(ratio_survivors(w)) == {0}
    kinds = [(k < 0, r < 0, k >= 50) for k, r in zip(w.obs_kf.tolist(), w.obs_kp.tolist())]
    assert min(sum(x[j] for x in kinds) for j in range(3)) >= 100
    out, into, cnt, margins = FW.restate_world(w, window=0)
    assert margins["min"] > 1e-6 > 1e-9, margins
    assert n_split == 1928 and cnt["n_absorbed"] == n_split
    xy, octv, desc, poses = w.slot_order()
    P = [np.ascontiguousarray(compute_projection_matrix(T[:3, :3], T[:3, 3], w.K), np.float64) for T in poses]
    wrong = FW.restate_world(w, lists=(xy, octv, desc, P), window=0)
    assert wrong[2]["n_points"] != cnt["n_points"]


def _row_cases():
    from tests import fuse_worlds as FW
    return FW.row_cases()


def test_row_cases():
    from tests import fuse_worlds as FW
    for name, (kfs, xyz, obs, want) in _row_cases().items():
        out, into, cnt, margins = FW.run_rows(kfs, xyz, obs)
        assert margins["min"] > 0.2 > 1e-9, (name, margins)
        assert FW.missed(want, out, into, cnt) == [], (name, cnt, FR.lists_of(out))


def test_row_cases_fail_under_a_wrong_reading():
    """the wrong readings each row case must fail under, by its construction: a target row behind the first 1024 is the answer
    (target_row_past_1024, crowded_cell); the answer is the lower of two rows at equal distance (crowded_cell, empty_target)"""
    from tests import fuse_worlds as FW
    bites = {"target_row_past_1024": {"targets_cut"}, "crowded_cell": {"targets_cut", "ties_high"}, "empty_target": {"ties_high"}}
    cases = _row_cases()
    assert set(cases) == set(bites)
    for name, (kfs, xyz, obs, want) in cases.items():
        got = {mu for mu in FW.MUTATIONS if FW.missed(want, *FW.run_rows(kfs, xyz, obs, mutation=mu)[:3])}
        assert got == bites[name] != set(), (name, got)
