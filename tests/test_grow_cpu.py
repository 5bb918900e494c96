"""tests/grow_restatement.py on constructed maps: the rules of mo_map_grow (include/vslam_amd.h) pinned without a device.  The worlds
and the hand-made gate cases are those of tests/grow_worlds.py, which tests/test_gpu_grow.py runs on the device."""
import numpy as np
import pytest

from tests import fuse_worlds as FW
from tests import grow_restatement as GR
from tests import grow_worlds as GW

MARGIN = 1e-9
_R = {}


def withheld(window):
    """the withheld world and its restated call, computed once per window"""
    if "w" not in _R:
        _R["w"] = GW.withheld_points_world()
    if window not in _R:
        _R[window] = GW.restate_world(_R["w"][0], window=window)
    return _R["w"] + _R[window]


def check_recovery(w, held, a, point, points, cnt, lo):
    """every withheld point with two or more observations from position `lo` on is back with exactly those observations and its
    position; nothing else was made"""
    back = GW.recovered(held, a, point, w.counts, lo)
    assert len(back) > 20
    n0 = cnt["n_points"] - cnt["n_new"]
    for i, want, got, xyz in back:
        assert i >= n0 and got == want, (i, want, got)
        assert np.abs(points[i - n0] - xyz.astype(np.float64)).max() < 1e-4
        assert a["xyz"][i].tobytes() == points[i - n0].astype(np.float32).tobytes()
    assert cnt["n_new"] == len(back)   # no point from the random rows, none from a point with one observation in the window
    assert np.array_equal(a["id"][n0:], np.arange(n0, cnt["n_points"])) and np.array_equal(np.sort(point[point >= 0]), a["id"][n0:])
    assert (a["dref_kf"][n0:] == w.survivors[-1]).all() and np.array_equal(a["dref_row"][n0:], np.flatnonzero(point >= 0))


def test_withheld_points_come_back():
    w, held, a, point, points, cnt, margins = withheld(0)
    assert margins["min"] > MARGIN, margins
    assert cnt["n_neighbours"] == 9 and cnt["n_free"] >= len(held) + 60 and cnt["n_epi"] > cnt["n_accepted"] >= cnt["n_matches"] > cnt["n_new"]
    check_recovery(w, held, a, point, points, cnt, 0)
    assert (a["color"][cnt["n_points"] - cnt["n_new"]:] == (0, 0, 255)).all()   # (no image)
    a0 = FW.world_inputs(w)[0]
    n0 = len(a0["id"])
    for f in GR.FIELDS:   # existing points keep their bytes
        k = len(a0[f]) - (1 if f == "obs_off" else 0)
        assert a[f][:k].tobytes() == a0[f][:k].tobytes(), f
    assert cnt["n_points"] == n0 + cnt["n_new"] == len(a["id"]) and cnt["n_obs"] == len(a["obs_kf"]) == a["obs_off"][-1]
    assert cnt["n_obs_new"] == sum(len(want) for _, want, _, _ in GW.recovered(held, a, point, w.counts, 0))


def test_window_of_three():
    w, held, a, point, points, cnt, margins = withheld(3)
    assert margins["min"] > MARGIN, margins
    assert cnt["n_neighbours"] == 3
    n0 = cnt["n_points"] - cnt["n_new"]
    assert n0 < len(a["id"]) and set(a["obs_kf"][a["obs_off"][n0]:].tolist()) <= {6, 7, 8, 9}
    check_recovery(w, held, a, point, points, cnt, 6)
    assert cnt["n_obs_new"] < withheld(0)[5]["n_obs_new"]   # (the observations at position 5 stay out)


@pytest.mark.parametrize("name", sorted(GW.cases()))
def test_gate_cases(name):
    kfs, obs, xyz, T, kw, want = GW.cases()[name]
    a, point, points, cnt, margins = GW.run(kfs, obs, xyz, T, **kw)
    assert margins["min"] > MARGIN, margins
    assert {k: cnt[k] for k in want if k in GR.COUNTS} == {k: v for k, v in want.items() if k in GR.COUNTS}, cnt
    if "point" in want:
        assert (point >= 0).tolist() == want["point"]
    if "lists" in want:
        assert FW.FR.lists_of(a) == want["lists"]
    assert len(points) == cnt["n_new"] and np.array_equal(a["xyz"][len(obs):], points.astype(np.float32))


def test_an_epipole_at_infinity_excludes_nothing():
    """sideways motion: c2[2] = 0, the epipole is (inf, NaN); the comparison with the zone is false for every row"""
    cam = [GR.camera(T) for T in GW.poses((0.0, 1.0))]
    _, ex, ey = GR.pair_geometry((100.0, 100.0, 50.0, 50.0), cam[1], cam[0])
    assert np.isinf(ex) and np.isnan(ey)
    kfs = GW.cases()["epi_octave0"][0]
    assert GW.run(kfs, epipole_r2=1e30)[3]["n_new"] == 1


def test_base_pair_is_the_lowest_cosine():
    kfs, T = GW.base_pair_case()
    a, point, points, cnt, margins = GW.run(kfs, T=T)
    assert margins["min"] > MARGIN and cnt["n_matches"] == 3 and cnt["n_new"] == 1
    assert np.abs(points[0] - [2.0, 0.0, 10.0]).max() < 1e-9   # exact in positions 0 and 3: triangulated from them
    # positions 1 and 2 see it half a pixel off: kept as observations (0.25 <= 5.991)
    assert FW.FR.lists_of(a) == [[(0, 0), (1, 0), (2, 0), (3, 0)]]
    # without position 0 the base pair is position 1, and the point is another
    _, _, p2, c2, _ = GW.run(kfs[1:], T=T[1:])
    assert c2["n_new"] == 1 and np.abs(p2[0] - [2.0, 0.0, 10.0]).max() > 1e-2


def test_stale_keys_read_the_same_free_rows():
    w, _ = GW.withheld_points_world()
    d, _ = GW.withheld_points_world(decorated=True)
    assert not np.array_equal(w.obs_kf, d.obs_kf) and (d.obs_kf < 0).sum() >= 20 and (d.obs_kp < 0).sum() >= 20
    fa, fb = GR.free_rows(FW.world_inputs(w)[0], w.counts), GR.free_rows(FW.world_inputs(d)[0], d.counts)
    assert all(np.array_equal(x, y) for x, y in zip(fa, fb))
    ra, rb = GW.restate_world(w, window=0), GW.restate_world(d, window=0)
    assert all(ra[3][k] == rb[3][k] for k in GR.COUNTS[:7]) and np.array_equal(ra[1], rb[1]) and np.array_equal(ra[2], rb[2]) and rb[4]["min"] > MARGIN


def test_no_work():
    e = FW.FR.as_arrays(np.zeros((0, 3)), [])
    for kfs in ([], GW.cases()["epi_octave0"][0][:1]):
        a, point, points, cnt, _ = GW.run(kfs, T=GW.poses()[:len(kfs)])
        assert all(v == 0 for v in cnt.values()) and len(points) == 0 and all(a[f].tobytes() == e[f].tobytes() for f in GR.FIELDS)
    kfs = [[(60, 30, GW.desc(0))], [(50, 30, GW.desc(0))]]
    a, point, points, cnt, _ = GW.run(kfs, [[(1, 0)]], [[1, -2, 10]], GW.poses((0.0, 1.0)))
    assert cnt["n_neighbours"] == 1 and all(cnt[k] == 0 for k in ("n_free", "n_epi", "n_accepted", "n_matches", "n_new", "n_obs_new"))
    assert cnt["n_points"] == 1 and point.tolist() == [-1]


def test_library_exports_the_call():
    import ctypes as C

    import vslam_amd as V
    lib = V.load_library()
    assert hasattr(lib, "mo_map_grow") and "mo_map_grow" in V.SIGNATURES
    assert (C.sizeof(V.MapGrowParams), C.sizeof(V.MapGrowOut)) == (56, 64)
    from vslam_amd.mapper import LocalMapper
    assert callable(LocalMapper.create_new_map_points)


# ---- keyframes past 1024 rows: the worlds and row cases of tests/grow_worlds.py, which tests/test_gpu_grow.py runs on the device ---------
_L = {}
ROWS = GW.row_cases()


def large(stale, window):
    """a large world and its restated call, computed once"""
    if (stale, window) not in _L:
        _L[stale, window] = GW.restate_world(GW.large_world(stale)[0], window=window)
    return GW.large_world(stale) + _L[stale, window]


def ratio_survivors(w):
    """per pair of consecutive keyframes in slot order (the order build_map adds them in): the rows of the earlier one whose best match
    in the later one passes the ratio test at 0.8"""
    from tests.reloc_restatement import hamming
    out = []
    for k in range(1, len(w.slot_desc)):
        d = np.sort(hamming(w.slot_desc[k - 1], w.slot_desc[k]).astype(np.int64), axis=1)[:, :2]
        out.append(int((d[:, 0] < 0.8 * d[:, 1]).sum()))
    return out


@pytest.mark.parametrize("window", [0, 2])
def test_large_world_withheld_points_come_back(window):
    """rows [921, 1117, 1924, 1830]: the target's 1830 free rows are two trips of k_grow_free and 29 waves, the neighbour of 1924 rows two
    tiles.  847 withheld points have two observations; with window 2 (positions 1 and 2) the same, since a point seen at position 3
    is seen at position 1 and never at 0 or 2 (the skip pattern)"""
    w, held, a, point, points, cnt, margins = large(False, window)
    assert margins["min"] > 1e-4 > MARGIN, margins
    assert w.counts.tolist() == [921, 1117, 1924, 1830] and cnt["n_free"] == 1830 and cnt["n_neighbours"] == (2 if window else 3)
    assert cnt["n_new"] == 847 and cnt["n_epi"] > 20000
    check_recovery(w, held, a, point, points, cnt, 1 if window else 0)
    assert (np.flatnonzero(point >= 0) >= 1024).sum() > 300   # points made by rows of the second trip


def test_large_worlds_have_no_match_for_a_growth_step():
    for stale in (False, True):
        assert set(ratio_survivors(GW.large_world(stale)[0])) == {0}


def test_large_stale_world():
    """six keyframes, position 1 removed, keys decorated: rows [548, 693, 1087, 1785, 1656].  Read without the position -> slot table, or
    with the rows behind the first 1024 of the neighbours or of the target missing, the restatement gives another map"""
    w, held, a, point, points, cnt, margins = large(True, 0)
    assert margins["min"] > 1e-4 > MARGIN, margins
    assert w.counts.tolist() == [548, 693, 1087, 1785, 1656] and w.survivors == [0, 2, 3, 4, 5]
    assert (w.obs_kf < 0).sum() >= 100 and (w.obs_kp < 0).sum() >= 100 and (w.obs_kf >= 50).sum() >= 100
    assert cnt["n_free"] == 1656 and cnt["n_new"] == 953
    check_recovery(w, held, a, point, points, cnt, 0)
    wrong = GW.restate_world(w, lists=w.slot_order(), window=0)
    assert wrong[3]["n_new"] != cnt["n_new"]
    lists = (w.kf_xy, w.kf_oct, w.kf_desc, w.kf_poses)
    cut_nb = tuple([x[:GW.TILE] for x in f[:-1]] + [f[-1]] for f in lists[:3]) + (w.kf_poses,)
    cut_tgt = tuple(list(f[:-1]) + [f[-1][:GW.TILE]] for f in lists[:3]) + (w.kf_poses,)
    for cut in (cut_nb, cut_tgt):
        assert GW.restate_world(w, lists=cut, window=0)[3]["n_new"] < cnt["n_new"]


@pytest.mark.parametrize("name", sorted(ROWS))
def test_row_cases(name):
    kfs, obs, xyz, T, kw, want = ROWS[name]
    a, point, points, cnt, margins = GW.run(kfs, obs, xyz, T, **kw)
    assert margins["min"] > 1e-3 > MARGIN, margins
    assert GW.missed(want, a, point, cnt, len(obs)) == [], cnt
    assert len(points) == cnt["n_new"] and np.array_equal(a["xyz"][len(obs):], points.astype(np.float32))
    assert len(a["id"]) == len(obs) + cnt["n_new"] and FW.FR.lists_of(a)[:len(obs)] == [list(o) for o in obs]
    if name == "empty_and_full_neighbours":   # the counts of the normal neighbour alone
        alone = GW.run(kfs[2:], T=T[2:], **kw)[3]
        assert all(alone[k] == cnt[k] for k in GR.COUNTS[1:7]) and alone["n_neighbours"] == 1


# the wrong readings each family of row cases must fail under, by its construction: a neighbour row behind the first tile is (or
# takes part in) the answer; the answer comes from target rows behind k_grow_free's first trip; the answer is the lower of two rows at
# equal distance.  tile_counts fails for n2 = 1025, 2048, 2049 (1023 and 1024 are the edge below: the same answer from one tile);
# first_tile_owned fails in the variant with the match in the second tile
BITES = {"tile_counts": {"neighbours_cut"}, "first_tile_owned": {"neighbours_cut"}, "tie_across_tiles": {"neighbours_cut", "ties_high"},
         "tie_inside_a_tile": {"ties_high"}, "two_waves_one_row": {"ties_high"}, "free_rows_past_1024": {"target_cut"},
         "empty_and_full_neighbours": {"ties_high"}}


def bitten(name):
    kfs, obs, xyz, T, kw, want = ROWS[name]
    out = set()
    for mu in GW.MUTATIONS:
        a, point, _, cnt, _ = GW.run_mutated(kfs, obs, xyz, T, kw, mu)
        if GW.missed(want, a, point, cnt, len(obs)):
            out.add(mu)
    return out


@pytest.mark.parametrize("family", GW.families(ROWS))
def test_row_cases_fail_under_a_wrong_reading(family):
    """every family's expectations stop holding under at least one wrong reading of the rows - the ones its construction aims at"""
    per_case = {name: bitten(name) for name in ROWS if name.split(":")[0] == family}
    assert set().union(*per_case.values()) == BITES[family] != set(), per_case
    if family == "tile_counts":
        assert {n for n, b in per_case.items() if b} == {"tile_counts:1025", "tile_counts:2048", "tile_counts:2049"}
    if family == "free_rows_past_1024":
        assert all(b == {"target_cut"} for b in per_case.values())
    if family == "tie_across_tiles":
        assert per_case == {"tie_across_tiles:equal": {"neighbours_cut", "ties_high"}, "tie_across_tiles:second_closer": {"neighbours_cut"}}
