"""The rules of reference-keyframe tracking (mo_map_track_reference in include/vslam_amd.h) on their numpy restatement
(tests/trackref_restatement.py): the orientation stage and the search on hand-made inputs, the whole call on the RelocWorld at three
vocabulary sizes, the frame a projection search cannot follow, and the library's new symbols.  No GPU."""
import numpy as np
import pytest

from tests import bow_worlds as BW
from tests import track_restatement as TR
from tests import trackref_restatement as TF
from tests import trackref_worlds as TW
from tests.map_worlds import with_bits


# ---- rule 6 -------------------------------------------------------------------------------------------------------------------------
def test_rotation_bins_at_the_wrap():
    assert TF.rotation_bin(354.0, 0.0) == 0          # 29.5 rounds to the even 30, which wraps to bin 0
    assert TF.rotation_bin(353.9, 0.0) == 29
    assert TF.rotation_bin(0.0, 6.0) == 0            # -6 + 360 = 354
    assert TF.rotation_bin(10.0, 4.0) == 0 and TF.rotation_bin(18.0, 0.0) == 2   # 0.5 -> 0, 1.5 -> 2: half to even
    assert TF.rotation_bin(30.0, 0.0) == 2 and TF.rotation_bin(31.0, 0.0) == 3   # 2.5 -> 2
    assert TF.rotation_bin(-1.0, -1.0) == 0
    assert TF.rotation_bin(np.nan, 0.0) == -1 and TF.rotation_bin(1000.0, 0.0) == -1


def _hist(counts):
    h = np.zeros(30, np.int64)
    for b, c in counts.items():
        h[b] = c
    return h


def test_three_maxima():
    assert TF.three_maxima(_hist({7: 50, 3: 40, 12: 20, 9: 20})) == [7, 3, 9]      # the third and fourth tie: the lower bin
    assert TF.three_maxima(_hist({7: 50, 12: 50, 3: 50})) == [3, 7, 12]
    assert TF.three_maxima(_hist({5: 100, 6: 9, 7: 9})) == [5, -1, -1]             # 9 against 100 drops the second, and with it the third
    assert TF.three_maxima(_hist({5: 100, 6: 10, 7: 9})) == [5, 6, -1]             # 10 against 100 keeps it
    assert TF.three_maxima(_hist({5: 100, 6: 10, 7: 10})) == [5, 6, 7]
    assert TF.three_maxima(_hist({5: 100, 6: 9, 7: 100})) == [5, 7, -1]
    assert TF.three_maxima(_hist({4: 3})) == [4, -1, -1]                           # bins of count 0 are never kept
    assert TF.three_maxima(_hist({})) == [-1, -1, -1]


def test_orientation_drops_the_claims_outside_the_kept_bins():
    kf_angle = np.array([100.0, 100.0, 100.0, 100.0, 200.0], np.float32)
    f_angle = np.array([70.0, 71.0, 69.0, 10.0, 200.0, 0.0], np.float32)           # rot 30, 29, 31, 90, 0
    key = {0: (3, 10), 1: (4, 11), 2: (5, 12), 3: (6, 13), 4: (7, 14)}
    kf_row = np.array([0, 1, 2, 3, 4, -1])
    hist, kept, left = TF.orientation(key, kf_row, kf_angle, f_angle)
    assert hist[2] == 2 and hist[3] == 1 and hist[8] == 1 and hist[0] == 1 and hist.sum() == 5
    assert kept == [2, 0, 3] and sorted(left) == [0, 1, 2, 4]


# ---- rules 4 and 5 on 8-row keyframes -------------------------------------------------------------------------------------------------
def _eight(seed=1):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (8, 32)).astype(np.uint8), np.zeros(8, np.int64)


def test_two_frame_rows_at_distance_zero_claim_the_lower():
    kd, kw = _eight()
    tab = np.full(8, -1)
    tab[0] = 5
    fd = np.random.default_rng(2).integers(0, 256, (7, 32)).astype(np.uint8)
    fd[2] = kd[0]; fd[5] = kd[0]
    woff, wrows = TF.buckets(np.zeros(7, np.int64), 2)
    assert woff.tolist() == [0, 7, 7] and wrows.tolist() == list(range(7))
    key, cq, cd, n_cand, n_claims = TF.search(kd, kw, tab, fd, woff, wrows)
    assert key == {2: (0, 5)} and cq[0] == 2 and cd[0] == 0 and (n_cand, n_claims) == (1, 1)   # 0 <= 0.7 * 0 holds
    assert TF.keyframe_rows(key, cq, cd, tab, 7).tolist() == [-1, -1, 0, -1, -1, -1, -1]


def test_two_frame_rows_at_the_same_best_distance_fail_the_ratio():
    kd, kw = _eight()
    tab = np.full(8, -1)
    tab[0] = 5
    fd = np.random.default_rng(2).integers(0, 256, (7, 32)).astype(np.uint8)
    fd[2] = with_bits(kd[0], [9]); fd[5] = with_bits(kd[0], [77])
    woff, wrows = TF.buckets(np.zeros(7, np.int64), 2)
    key, cq, cd, n_cand, n_claims = TF.search(kd, kw, tab, fd, woff, wrows)
    assert key == {} and (cq < 0).all() and (cd < 0).all() and (n_cand, n_claims) == (1, 0)
    # the same two rows in different buckets: each is alone in its bucket, no second distance, the candidate's word decides
    woff, wrows = TF.buckets(np.array([0, 0, 1, 0, 0, 0, 0]), 2)
    assert wrows.tolist() == [0, 1, 3, 4, 5, 6, 2]
    kw[0] = 1
    key, cq, cd, _, _ = TF.search(kd, kw, tab, fd, woff, wrows)
    assert key == {2: (1, 5)}


def test_two_candidates_on_one_frame_row_the_lower_point_wins():
    kd, kw = _eight()
    kd[3] = kd[1]
    tab = np.full(8, -1)
    tab[1] = 7; tab[3] = 4; tab[6] = 2
    fd = np.random.default_rng(2).integers(0, 256, (5, 32)).astype(np.uint8)
    fd[4] = with_bits(kd[1], [3, 100])
    woff, wrows = TF.buckets(np.zeros(5, np.int64), 2)
    key, cq, cd, n_cand, n_claims = TF.search(kd, kw, tab, fd, woff, wrows, max_dist=50)
    assert key == {4: (2, 4)} and cq[1] == 4 and cq[3] == 4 and cq[6] == -1 and (n_cand, n_claims) == (3, 2)
    assert TF.keyframe_rows(key, cq, cd, tab, 5).tolist() == [-1, -1, -1, -1, 3]   # the row of the point that holds the claim
    tab[1] = 4                                                                      # both rows observe one point: the lower row
    key, cq, cd, _, _ = TF.search(kd, kw, tab, fd, woff, wrows)
    assert TF.keyframe_rows(key, cq, cd, tab, 5)[4] == 1


# ---- the RelocWorld -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_words", [64, 256, 1024])
def test_reloc_world_keeps_a_thousand_inliers(n_words):
    w = BW.reloc_world()
    r = TW.reloc_restated("near", n_words)
    T = TW.reloc_frame("near")[2]
    print("W", n_words, "cand", r["n_cand"], "claims", r["n_claims"], "raw", r["n_matches_raw"], "matches", r["n_matches"], "inliers", r["n_inliers"],
          "kept", r["kept_bin"], "err", np.abs(r["pose"] - T).max())
    assert r["ok"] and r["n_inliers"] >= 1000
    assert np.abs(r["pose"] - T).max() < 1e-6
    assert r["kept_bin"][:2] in ([2, 3], [3, 2]) and r["n_matches"] < r["n_matches_raw"]   # the random angles are dropped
    assert r["n_cand"] == int((TW.reloc_point_of()[TW.KF] >= 0).sum()) and r["n_claims"] >= r["n_matches_raw"]
    assert len(w.kf_desc[TW.KF]) == len(r["cq"])


def test_the_frame_a_projection_search_cannot_follow():
    w = BW.reloc_world()
    kps, d, T = TW.reloc_frame("far")
    kf_oct = [np.zeros(len(x), np.int64) for x in w.kf_desc]
    t = TR.track(BW.K, w.poses[TW.KF], w.X[w.world], w.obs_off, w.obs_kf, w.obs_kp, w.kf_desc, kf_oct, kps, d, BW.W_IMG, BW.H_IMG)
    assert not t["ok"]
    r = TW.reloc_restated("far", 256)
    print("projection passes", [(p["matches"], p["radius"]) for p in t["passes"]], "reference inliers", r["n_inliers"], "err", np.abs(r["pose"] - T).max())
    assert r["ok"] and r["n_inliers"] >= 800
    assert np.abs(r["pose"] - T).max() < 1e-6


# ---- the library ------------------------------------------------------------------------------------------------------------------------
def test_the_library_has_the_new_symbols():
    import ctypes as C
    import vslam_amd as V
    lib = V.load_library()
    assert lib.mo_abi_version() == 7 and V.ABI_VERSION == 7
    f = lib.mo_map_track_reference
    assert f.restype is C.c_int and len(f.argtypes) == 6 and all(a is C.c_void_p for a in f.argtypes)
    g = lib.mo_map_keyframe_words
    assert g.restype is C.c_int and g.argtypes == [C.c_void_p, C.c_int32, C.c_void_p]
    assert C.sizeof(V.MapTrackRefParams) == 48 and C.sizeof(V.MapTrackRefOut) == 32 + 96 + 5 * 4 + 33 * 4 + 8
    assert V.MapTrackRefOut.hist.offset == 32 + 96 + 20 and V.MapTrackRefOut.ok.offset == 32 + 96 + 20 + 132
    from vslam_amd.mapper import LocalMapper
    assert callable(LocalMapper.track_reference_keyframe) and callable(LocalMapper.keyframe_words)
