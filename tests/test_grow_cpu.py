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
