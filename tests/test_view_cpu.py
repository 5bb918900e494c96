"""The inputs of tests/test_gpu_view.py and the restatement they are compared with (tests/view_restatement.py, tests/view_worlds.py),
checked without a GPU: the worlds decide every gate clearly, the scale model keeps the true octave inside [L - 1, L], the product form
of the predicted level is ORB-SLAM2's logarithm form, the approach query is one the plain search loses and the frustum search finds, and
the views of the small cases come out as constructed."""
import numpy as np
import pytest

from tests import fuse_restatement as FR
from tests import track_restatement as TR
from tests import view_restatement as VR
from tests import view_worlds as VW

MARGIN = 1e-9   # above the relative error of a handful of f64 operations (1e-15) by six orders: no last bit flips a decision


def _local_views(w, **kw):
    a = w.arrays()
    return a, VR.local_views(a["xyz"], a["obs_off"], a["obs_kf"], a["obs_kp"], w.kf_desc, w.kf_oct, w.kf_P(), **kw)


def test_true_octave_lies_in_the_predicted_gate():
    checked = 0
    for name in VW.TRACK_CASES:
        c = VW.track_case(name)
        checked += VW.scale_gate_holds(c["w"], c["T"])
    for w in (VW.world("scaled"), VW.world("duplicates")):
        for T in w.kf_poses:
            checked += VW.scale_gate_holds(w, T)
    assert checked > 5000


@pytest.mark.parametrize("name", VW.TRACK_CASES)
@pytest.mark.parametrize("window", [10, 0])
def test_tracking_cases_decide_every_gate_clearly(name, window):
    """both passes of every case, the second from the restated refinement of the first (the device's differs from it by 1e-9 at most,
    tests/test_gpu_view.py asserts the same margin on the pose the device used)"""
    c = VW.track_case(name)
    a, lv = _local_views(c["w"], window=window)
    mg = VR.new_margins()
    r = VR.track_frustum(VW.K, c["pose0"], a["xyz"], lv, c["kps"], c["desc"], VW.W_IMG, VW.H_IMG, margins=mg, refine_pose=True)
    assert r["passes"] and r["passes"][0]["in_image"] > 0
    assert VR.min_margin(mg) > MARGIN, mg


def test_fusion_world_decides_every_gate_clearly_and_merges_every_duplicate():
    w = VW.world("duplicates")
    a = w.arrays()
    assert len(w.pairs) > 100
    for i, j in w.pairs:   # two observations three octaves apart
        (ki, ri), = w.obs[i].items()
        (kj, rj), = w.obs[j].items()
        assert abs(int(w.kf_oct[ki][ri]) - int(w.kf_oct[kj][rj])) == 3
    _, into, cnt, mg = VR.fuse_frustum(a, w.kf_P(), w.kf_xy, w.kf_oct, w.kf_desc, VW.W_IMG, VW.H_IMG, window=0)
    assert VR.min_margin(mg) > MARGIN, mg
    assert all(into[i] == into[j] for i, j in w.pairs) and cnt["n_absorbed"] == len(w.pairs)
    _, into0, cnt0, mg0 = FR.fuse(a, w.kf_P(), w.kf_xy, w.kf_oct, w.kf_desc, VW.W_IMG, VW.H_IMG, window=0)
    assert not any(into0[i] == into0[j] for i, j in w.pairs) and cnt0["n_absorbed"] == 0


def test_level_by_products_is_the_clamped_logarithm():
    rng = np.random.default_rng(3)
    ratio = np.exp(rng.uniform(np.log(0.2), np.log(8.0), 100000))   # max_dist / dist: below level 0 to beyond level 7
    e = np.log(ratio) / np.log(1.2)
    ratio = ratio[np.abs(e - np.round(e)) * np.log(1.2) > 1e-9]     # not within 1e-9 (relative) of a power of 1.2
    assert len(ratio) > 99000
    seen = set()
    for r in ratio.tolist():
        dist = 3.0
        mx = float(np.float32(dist * r))
        ok, L = VR.frustum(np.array([0.0, 0.0, dist]), np.array([0.0, 0.0, 1.0], np.float32), mx, np.zeros(3), range_lo=0.0, range_hi=np.inf)
        assert ok and L == VR.level_by_log(dist, mx), (r, L)
        seen.add(L)
    assert seen == set(range(8))


def test_approach_is_lost_by_the_plain_search_and_found_under_the_frustum():
    c = VW.track_case("approach")
    w = c["w"]
    a, lv = _local_views(w)
    _, local, rep, ref, views, _ = lv
    # every keyframe that built the map stands at least twice as deep as the query
    assert all(d >= 2.0 * np.abs(VW.centre_of(c["T"])[2]) for d in w.depths)
    min_matches = 20
    for radius in (15.0, 30.0):   # the pass and its retry
        point, _, n_cand = TR.search(VW.K, c["pose0"], a["xyz"], rep, ref, c["kps"], c["desc"], VW.W_IMG, VW.H_IMG, radius)
        assert n_cand > 500 and (point >= 0).sum() < min_matches
    point, _, level, n_img, n_cand = VR.search_frustum(VW.K, c["pose0"], a["xyz"], rep, ref, views, c["kps"], c["desc"], VW.W_IMG, VW.H_IMG, 15.0)
    truth = c["truth"]
    cand_truth = [q for q in np.flatnonzero(truth >= 0) if VR.frustum(a["xyz"][truth[q]].astype(np.float64), views["normal"][truth[q]],
                                                                      views["max_dist"][truth[q]], VR.camera_centre(c["pose0"]))[0]]
    assert len(cand_truth) > 300
    # the constructed matches of the points the frustum lets through: found, but for a few lost to the ratio test or a displaced neighbour
    found = sum(point[q] == truth[q] for q in cand_truth)
    assert found >= 0.97 * len(cand_truth), (found, len(cand_truth))
    assert (level[point >= 0] - c["kps"]["octave"][point >= 0]).min() >= 0 and (level[point >= 0] - c["kps"]["octave"][point >= 0]).max() <= 1


def _hand_views(xyz, obs, poses, octaves):
    kf_P = [TR.projection_matrix(VW.K, T) for T in poses]
    C = VR.centres(kf_P)
    return VR.point_views(np.array(xyz, np.float32), obs, octaves, C), C


def test_view_of_a_point_with_one_observation():
    T = VW.camera("A", 10.0, 0.5, -0.25)
    v, C = _hand_views([[0.5, -0.25, 2.0]], [[(0, 1)]], [T], [np.array([0, 3])])
    assert np.allclose(C[0], [0.5, -0.25, -10.0], atol=1e-12)
    assert v["ref_pos"][0] == 0 and v["ref_octave"][0] == 3 and v["n_valid"][0] == 1
    assert np.allclose(v["normal"][0], [0.0, 0.0, 1.0], atol=1e-7)
    assert np.isclose(v["max_dist"][0], 12.0 * 1.2 ** 3, rtol=1e-6) and np.isclose(v["min_dist"][0], 12.0 * 1.2 ** 3 / 1.2 ** 7, rtol=1e-6)


def test_view_when_the_first_observation_is_stale():
    """the first stored key names a keyframe that is gone: the reference passes to the next observation, as mpRefKF does"""
    poses = [VW.camera("A", 10.0), VW.camera("A", 5.0, 5.0)]
    octaves = [np.array([2]), np.array([4])]
    off, okf, okp = np.array([0, 3]), np.array([7, 1, 0]), np.array([0, 0, 0])   # position 7 does not exist
    obs = TR.valid_observations(off, okf, okp, [1, 1])
    assert obs == [[(1, 0), (0, 0)]]
    v, C = _hand_views([[0.0, 0.0, 0.0]], obs, poses, octaves)
    assert v["ref_pos"][0] == 1 and v["ref_octave"][0] == 4 and v["n_valid"][0] == 2
    d1 = np.sqrt(50.0)
    assert np.isclose(v["max_dist"][0], d1 * 1.2 ** 4, rtol=1e-6)
    want = (np.array([-5.0, 0.0, 5.0]) / d1 + np.array([0.0, 0.0, 1.0])) / 2.0
    assert np.allclose(v["normal"][0], want, atol=1e-7) and np.linalg.norm(v["normal"][0]) < 0.95   # (not renormalised)


def test_views_of_points_without_a_usable_observation():
    """no observation, an observation at a keyframe whose P is singular, a point in its reference centre: max_dist 0 or no reference,
    never a candidate"""
    T = VW.camera("A", 10.0)
    kf_P = [TR.projection_matrix(VW.K, T), np.zeros((3, 4))]
    C = VR.centres(kf_P)
    assert np.isnan(C[1]).all() and np.isfinite(C[0]).all()
    v = VR.point_views(np.array([[0, 0, 0], [1, 1, 1], [0, 0, -10]], np.float32), [[], [(1, 0)], [(0, 0)]], [np.array([1]), np.array([1])], C)
    assert v["ref_pos"].tolist() == [-1, -1, 0] and v["n_valid"].tolist() == [0, 0, 0] and (v["max_dist"] == 0).all()
    for i in range(3):
        assert not VR.frustum(np.array([0.0, 0.0, 5.0]), v["normal"][i], v["max_dist"][i], np.zeros(3))[0]
