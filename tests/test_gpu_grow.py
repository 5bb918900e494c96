"""LocalMapper.create_new_map_points (mo_map_grow) on the device against tests/grow_restatement.py: byte for byte on every integer map
array, on `point` and on every count; the f64 points at rtol = atol = 1e-9 (the bound of the one-step bundle adjustment test,
profiles/ba_parity.txt), the stored xyz exactly float32 of them.  Each map first shows that no threshold decision of the restatement
comes within 1e-9 of its threshold.  The worlds and hand-made cases are those of tests/grow_worlds.py and tests/test_grow_cpu.py."""
import numpy as np
import pytest

from tests import fuse_restatement as FR
from tests import fuse_worlds as FW
from tests import grow_restatement as GR
from tests import grow_worlds as GW
from tests import track_restatement as TR
from tests.map_worlds import build_map, kps_array, pose_near, perturbed_pose

pytestmark = pytest.mark.gpu

MARGIN = 1e-9
TINY = (2, 16, 16, 32)
INT_FIELDS = ("color", "id", "obs_off", "obs_kf", "obs_kp", "dref_kf", "dref_row")


def _ctx():
    import vslam_amd as V
    return V.Context(device=0, max_w=640, max_h=480, max_batch=1)


def _snapshot(m):
    m._cache = None; m._lists = None
    return {f: v.copy() for f, v in m.arrays().items()}, [x.copy() for x in m.list_arrays()]


def _grow_equals_restatement(m, **kw):
    """one call on the device against the restatement of the map as it stood; returns (info, restated arrays, point, points, counts)"""
    want, point, points, cnt, margins = GW.restate(m, **kw)
    assert margins["min"] > MARGIN, margins
    info = m.create_new_map_points(want_points=True, **kw)
    got = m.arrays()
    for f in INT_FIELDS:
        assert got[f].dtype == want[f].dtype and got[f].tobytes() == want[f].tobytes(), (f, got[f].shape, want[f].shape)
    assert np.array_equal(info["point"], point)
    assert {k: info[k] for k in GR.COUNTS} == cnt, (info, cnt)
    assert info["points"].shape == points.shape and np.allclose(info["points"], points, rtol=1e-9, atol=1e-9)
    n0 = cnt["n_points"] - cnt["n_new"]
    assert got["xyz"][:n0].tobytes() == want["xyz"][:n0].tobytes()
    assert got["xyz"][n0:].tobytes() == info["points"].astype(np.float32).tobytes()
    assert len(m.map_points) == cnt["n_points"]
    return info, want, point, points, cnt


@pytest.mark.parametrize("window", [0, 3])
def test_withheld_points_come_back(window):
    """(1) every map point seen from the last keyframe taken out of the map, its keypoints left in the keyframes: the call gives back
    every one with two observations inside the window, with exactly those observations, within 1e-4 of its place; nothing else"""
    from tests.test_grow_cpu import check_recovery
    ctx = _ctx()
    w, held = GW.withheld_points_world()
    m = build_map(ctx, w)
    lists0 = _snapshot(m)[1]
    info, want, point, points, cnt = _grow_equals_restatement(m, window=window)
    assert info["n_neighbours"] == (3 if window else 9) and info["n_new"] > 20
    check_recovery(w, held, m.arrays(), info["point"], info["points"], cnt, 6 if window else 0)
    assert all(np.array_equal(x, y) for x, y in zip(_snapshot(m)[1], lists0))   # the per-keyframe lists stay those of the last cull
    assert ctx.dev_status() == 0
    m.close(); ctx.close()


def test_gate_cases_on_hand_made_maps():
    """(2) the cases of tests/test_grow_cpu.py, one row just inside each gate and one just outside, on the device"""
    ctx = _ctx()
    for name, (kfs, obs, xyz, T, kw, want) in sorted(GW.cases().items()):
        m = GW.hand(ctx, kfs, obs, xyz, T)
        info, a, point, points, cnt = _grow_equals_restatement(m, window=0, **kw)
        assert {k: info[k] for k in want if k in GR.COUNTS} == {k: v for k, v in want.items() if k in GR.COUNTS}, (name, info)
        if "point" in want:
            assert (info["point"] >= 0).tolist() == want["point"], name
        if "lists" in want:
            assert FR.lists_of(m.arrays()) == want["lists"], name
        m.close()
    kfs, T = GW.base_pair_case()
    m = GW.hand(ctx, kfs, [], [], T)
    info, _, _, _, _ = _grow_equals_restatement(m, window=0)
    assert info["n_new"] == 1 and np.abs(info["points"][0] - [2.0, 0.0, 10.0]).max() < 1e-9
    m.close()
    assert ctx.dev_status() == 0
    ctx.close()


@pytest.mark.parametrize("decorated", [False, True], ids=["clean", "stale"])
def test_position_is_not_slot(decorated):
    """(3) positions (1, 4) removed: from position 1 on a keyframe's slot is not its position.  Read without the table (position p
    taken for slot p: other keypoints, descriptors and poses) the restatement gives another map"""
    ctx = _ctx()
    w, held = GW.withheld_points_world(removed=(1, 4), seed=43, decorated=decorated)
    m = build_map(ctx, w)
    assert [w.survivors[p] != p for p in range(len(w.survivors))].count(True) >= 6
    info, want, point, points, cnt = _grow_equals_restatement(m, window=0)
    assert info["n_new"] > 20 and (m.arrays()["dref_kf"][-info["n_new"]:] == w.survivors[-1]).all()
    wrong = GW.restate_world(w, lists=w.slot_order(), window=0)
    assert wrong[3] != cnt and wrong[3]["n_new"] != cnt["n_new"]
    assert ctx.dev_status() == 0
    m.close(); ctx.close()


def test_no_work_determinism_and_growth_from_a_tiny_capacity():
    """(4) an empty map, one keyframe, a target without a free row: every growth count is 0 and the bytes stay.  (5) Two maps built
    alike give the same bytes; a map made with capacities every store outgrows gives them too."""
    from vslam_amd.mapper import LocalMapper
    ctx = _ctx()
    w, held = GW.withheld_points_world()
    m = LocalMapper(w.K, save_every_keyframe=False, context=ctx)
    info = m.create_new_map_points()
    assert all(info[k] == 0 for k in GR.COUNTS) and len(info["point"]) == 0
    m.add_keyframe(np.zeros((480, 640), np.uint8), kps_array(w.slot_xy[0]), w.slot_desc[0], w.slot_poses[0])
    info = m.create_new_map_points()
    assert all(info[k] == 0 for k in GR.COUNTS) and (info["point"] == -1).all() and len(info["point"]) == len(w.slot_xy[0])
    m.close()
    D = GW.desc(0)
    m = GW.hand(ctx, [[(60, 30, D)], [(50, 30, D)]], [[(1, 0)]], [[1, -2, 10]], GW.poses((0.0, 1.0)))
    snap = _snapshot(m)
    info, _, _, _, cnt = _grow_equals_restatement(m, window=0)
    assert info["n_neighbours"] == 1 and all(info[k] == 0 for k in GR.COUNTS[1:7]) and info["n_points"] == 1
    again = _snapshot(m)
    assert all(again[0][f].tobytes() == snap[0][f].tobytes() for f in snap[0]) and all(np.array_equal(x, y) for x, y in zip(again[1], snap[1]))
    m.close()
    out = []
    for cap in (None, None, TINY):
        m = build_map(ctx, w, capacity=cap)
        info = m.create_new_map_points(window=0, want_points=True)
        a = m.arrays()
        out.append([a[f].tobytes() for f in GR.FIELDS] + [info["point"].tobytes(), info["points"].tobytes()] + [info[k] for k in GR.COUNTS])
        m.close()
    assert out[0] == out[1] == out[2] and out[0][-4] > 20   # (n_new)
    assert ctx.dev_status() == 0
    ctx.close()


def test_colour_is_the_pixel_under_the_keypoint():
    """(6) a non-constant image: the new points carry the target image's pixel at (int(x), int(y)), gray and 3-channel"""
    ctx = _ctx()
    kfs, _, _, T, _, _ = GW.cases()["scale_ratio"]
    yy, xx = np.mgrid[0:100, 0:100]
    gray = ((3 * xx + 7 * yy) % 251).astype(np.uint8)
    for img in (gray, np.dstack([gray, gray[::-1], gray.T]).copy()):
        m = GW.hand(ctx, kfs, [], [], T, image=img)
        info, _, _, _, _ = _grow_equals_restatement(m, window=0)
        assert info["n_new"] == 2
        col = m.arrays()["color"]
        for c, (x, y) in zip(col, [(50, 20), (50, 60)]):
            assert c.tolist() == (img[y, x].tolist() if img.ndim == 3 else [int(img[y, x])] * 3)
        m.close()
    assert ctx.dev_status() == 0
    ctx.close()


def test_the_grown_map_serves_every_reader():
    """(7) on the grown map: track_local_map and bundle_adjust(max_steps=(0, 0)) agree with their restatements on the grown arrays, the
    co-visibility graph equals the recount, a second call creates nothing, fuse_map_points merges none of the new points, and the
    cull of a further keyframe keeps every new point"""
    from tests.ba_restatement import bundle_adjust as restate_ba
    ctx = _ctx()
    w, held = GW.withheld_points_world()
    size = w.image_size
    m = build_map(ctx, w)
    info, want, point, points, cnt = _grow_equals_restatement(m, window=0)
    n0 = cnt["n_points"] - cnt["n_new"]
    a = {f: v.copy() for f, v in m.arrays().items()}
    # the co-visibility graph: empty before (no growth step found a model), the recount of the new points after
    g = m.co_visibility_graph
    recount = GR.co_visibility_recount(a, w.counts, first=n0)
    assert recount and {(p, q): g[p][q] for p in g for q in g[p] if p < q and g[p][q]} == recount
    assert all(g[q][p] == d for (p, q), d in recount.items())
    # a second call: the rows are owned now
    info2, _, _, _, _ = _grow_equals_restatement(m, window=0)
    assert info2["n_new"] == 0 and info2["n_free"] == info["n_free"] - info["n_new"] and info2["n_points"] == cnt["n_points"]
    assert all(m.arrays()[f].tobytes() == a[f].tobytes() for f in a)
    # tracking reads the grown map
    T = pose_near(w, 8)
    kps, desc = w.world0.track_query(T, wrong=0.0)
    pose0 = perturbed_pose(T)
    ok, pose, ti = m.track_local_map(kps, desc, pose0, radii=(15.0,), image_size=size)
    r = TR.track(w.K, pose0, a["xyz"], a["obs_off"], a["obs_kf"], a["obs_kp"], w.kf_desc, w.kf_oct, kps, desc, size[0], size[1], radii=(15.0,),
                 refine_pose=False)
    assert ti["n_local"] == r["n_local"] and np.array_equal(ti["point"], r["passes"][0]["point"]) and np.array_equal(ti["dist"], r["passes"][0]["dist"])
    assert (ti["point"] >= n0).sum() >= 20
    # bundle adjustment: the problem on the grown arrays
    okb, bi = m.bundle_adjust(window=6, max_steps=(0, 0), want_points=True)
    rb = restate_ba(a["obs_off"], a["obs_kf"], a["obs_kp"], w.counts, w.kf_xy, w.kf_oct, a["xyz"], w.K, np.array([T_[:3, :4] for T_ in w.kf_poses]),
                    window=6, max_steps=(0, 0))
    for k in ("n_free", "n_fixed", "n_local", "n_edges", "n_inliers", "free", "fixed"):
        assert bi[k] == rb[k], (k, bi[k], rb[k])
    assert np.array_equal(bi["edge_inlier"], rb["edge_inlier"]) and bi["n_edges"] > 100
    # fusion finds nothing to merge among the new points
    fi = m.fuse_map_points(image_size=size, window=0)
    assert (np.bincount(fi["into"])[fi["into"][n0:]] == 1).all()
    b = m.arrays()
    assert np.array_equal(b["xyz"][fi["into"][n0:]], a["xyz"][n0:])
    # a further keyframe: its cull keeps every new point (noise-free: reprojection errors ~ 1e-5 px)
    rng = np.random.default_rng(3)
    kp = kps_array(np.column_stack([rng.uniform(0, size[0], 200), rng.uniform(0, size[1], 200)]))
    m.add_keyframe(np.zeros((size[1], size[0]), np.uint8), kp, rng.integers(0, 256, (200, 32)).astype(np.uint8), w.kf_poses[-1])
    assert m.last["n_new"] == 0
    c = m.arrays()
    assert set(map(bytes, a["xyz"][n0:])) <= set(map(bytes, c["xyz"]))
    assert ctx.dev_status() == 0
    m.close(); ctx.close()


# ---- keyframes past 1024 rows (tests/grow_worlds.py: large_world, row_cases) --------------------------------------------------------------
@pytest.mark.parametrize("window", [0, 2])
def test_large_world_withheld_points_come_back(window):
    """(8) the withheld world at the mapper's keyframe size, rows [921, 1117, 1924, 1830]: k_grow_free takes two trips over the target's
    1830 free rows, the search 29 waves per neighbour and two tiles in the neighbour of 1924 rows.  Every withheld point with two
    observations inside the window is back with exactly those"""
    from tests.test_grow_cpu import check_recovery
    ctx = _ctx()
    w, held = GW.large_world()
    m = build_map(ctx, w)
    info, want, point, points, cnt = _grow_equals_restatement(m, window=window)
    assert info["n_free"] > 1024 and max(w.counts[:-1]) > 1024 and info["n_neighbours"] == (2 if window else 3) and info["n_new"] > 500
    check_recovery(w, held, m.arrays(), info["point"], info["points"], cnt, 1 if window else 0)
    assert ctx.dev_status() == 0
    m.close(); ctx.close()


def test_large_stale_world_position_is_not_slot():
    """(9) six keyframes of up to 1785 rows, position 1 removed, keys decorated: slot != position behind tables strided by the row
    capacity, read past row 1024"""
    ctx = _ctx()
    w, held = GW.large_world(stale=True)
    m = build_map(ctx, w)
    assert [w.survivors[p] != p for p in range(len(w.survivors))].count(True) == 4 and (w.counts > 1024).sum() >= 3
    info, want, point, points, cnt = _grow_equals_restatement(m, window=0)
    assert info["n_new"] > 500 and (m.arrays()["dref_kf"][-info["n_new"]:] == w.survivors[-1]).all()
    wrong = GW.restate_world(w, lists=w.slot_order(), window=0)
    assert wrong[3] != cnt and wrong[3]["n_new"] != cnt["n_new"]
    assert ctx.dev_status() == 0
    m.close(); ctx.close()


def test_large_world_from_a_tiny_capacity():
    """(10) the large world in a map made with capacities every store outgrows - the keyframe store regrows its row stride across 1024
    rows - gives the bytes of the default build"""
    ctx = _ctx()
    w, held = GW.large_world()
    out = []
    for cap in (None, TINY):
        m = build_map(ctx, w, capacity=cap)
        info = m.create_new_map_points(window=0, want_points=True)
        a = m.arrays()
        out.append([a[f].tobytes() for f in GR.FIELDS] + [info["point"].tobytes(), info["points"].tobytes()] + [info[k] for k in GR.COUNTS])
        m.close()
    assert out[0] == out[1] and out[0][-4] > 500   # (n_new)
    assert ctx.dev_status() == 0
    ctx.close()


def test_the_grown_large_map_serves_every_reader():
    """(11) the reader checks of (7) on the grown large map: a second call creates nothing, track_local_map and
    bundle_adjust(max_steps=(0, 0)) agree with their restatements on the grown arrays, fuse_map_points merges none of the new points"""
    from tests.ba_restatement import bundle_adjust as restate_ba
    ctx = _ctx()
    w, held = GW.large_world()
    size = w.image_size
    m = build_map(ctx, w)
    info, want, point, points, cnt = _grow_equals_restatement(m, window=0)
    n0 = cnt["n_points"] - cnt["n_new"]
    a = {f: v.copy() for f, v in m.arrays().items()}
    info2, _, _, _, _ = _grow_equals_restatement(m, window=0)
    assert info2["n_new"] == 0 and info2["n_free"] == info["n_free"] - info["n_new"] and info2["n_points"] == cnt["n_points"]
    assert all(m.arrays()[f].tobytes() == a[f].tobytes() for f in a)
    T = pose_near(w, 2)
    kps, desc = w.world0.track_query(T, wrong=0.0)
    pose0 = perturbed_pose(T)
    ok, pose, ti = m.track_local_map(kps, desc, pose0, radii=(15.0,), image_size=size)
    r = TR.track(w.K, pose0, a["xyz"], a["obs_off"], a["obs_kf"], a["obs_kp"], w.kf_desc, w.kf_oct, kps, desc, size[0], size[1], radii=(15.0,),
                 refine_pose=False)
    assert ti["n_local"] == r["n_local"] and np.array_equal(ti["point"], r["passes"][0]["point"]) and np.array_equal(ti["dist"], r["passes"][0]["dist"])
    assert (ti["point"] >= n0).sum() >= 500
    okb, bi = m.bundle_adjust(window=6, max_steps=(0, 0), want_points=True)
    rb = restate_ba(a["obs_off"], a["obs_kf"], a["obs_kp"], w.counts, w.kf_xy, w.kf_oct, a["xyz"], w.K, np.array([T_[:3, :4] for T_ in w.kf_poses]),
                    window=6, max_steps=(0, 0))
    for k in ("n_free", "n_fixed", "n_local", "n_edges", "n_inliers", "free", "fixed"):
        assert bi[k] == rb[k], (k, bi[k], rb[k])
    assert np.array_equal(bi["edge_inlier"], rb["edge_inlier"]) and bi["n_edges"] > 1000
    fi = m.fuse_map_points(image_size=size, window=0)
    assert (np.bincount(fi["into"])[fi["into"][n0:]] == 1).all()
    assert np.array_equal(m.arrays()["xyz"][fi["into"][n0:]], a["xyz"][n0:])
    assert ctx.dev_status() == 0
    m.close(); ctx.close()


@pytest.mark.parametrize("family", GW.families(GW.row_cases()))
def test_row_cases_on_hand_made_maps(family):
    """(12) the row cases of tests/test_grow_cpu.py on the device: tile counts of the neighbour, tiles without a free row, ties across and
    inside a tile and between two waves, free target rows behind row 1024 with n_free at the edges of a wave, neighbours without a
    (free) row"""
    ctx = _ctx()
    for name, (kfs, obs, xyz, T, kw, want) in sorted(GW.row_cases().items()):
        if name.split(":")[0] != family:
            continue
        m = GW.hand(ctx, kfs, obs, xyz, T)
        info, a, point, points, cnt = _grow_equals_restatement(m, window=0, **kw)
        assert GW.missed(want, m.arrays(), info["point"], {k: info[k] for k in GR.COUNTS}, len(obs)) == [], (name, info)
        m.close()
    assert ctx.dev_status() == 0
    ctx.close()
