"""LocalMapper.fuse_map_points (mo_map_fuse) on the device against tests/fuse_restatement.py: byte for byte on every map array, on
`into` and on every count.  Each world first shows that no threshold decision of the restatement comes within 1e-9 of its threshold
(the device forms the same f64 expressions; at such a margin a differently rounded last bit cannot flip a decision).  The seeds of
tests/fuse_worlds.py were chosen on the CPU so that this holds."""
import numpy as np
import pytest

from tests import fuse_restatement as FR
from tests import fuse_worlds as FW
from tests import track_restatement as TR
from tests.map_worlds import build_map, kps_array, pose_near, perturbed_pose

pytestmark = pytest.mark.gpu

MARGIN = 1e-9
TINY = (2, 16, 16, 32)


def _ctx():
    import vslam_amd as V
    return V.Context(device=0, max_w=640, max_h=480, max_batch=1)


def _snapshot(m):
    m._cache = None; m._lists = None
    return {f: v.copy() for f, v in m.arrays().items()}, [x.copy() for x in m.list_arrays()]


def _fuse_equals_restatement(m, size, **kw):
    """one call on the device against the restatement of the map as it stood; returns (info, restated arrays, counts, arrays before)"""
    before = FW.map_inputs(m)[0]
    want, into, cnt, margins = FW.restate(m, size, **kw)
    assert margins["min"] > MARGIN, margins
    info = m.fuse_map_points(image_size=size, **kw)
    got = m.arrays()
    for f in FR.FIELDS:
        assert got[f].dtype == want[f].dtype and got[f].tobytes() == want[f].tobytes(), (f, got[f].shape, want[f].shape)
    assert np.array_equal(info["into"], into)
    assert {k: info[k] for k in FR.COUNTS} == cnt, (info, cnt)
    assert len(m.map_points) == cnt["n_points"]
    return info, want, cnt, before


def test_split_world_is_put_together_again_and_serves_every_reader():
    """(1) every multi-view point of a skip world injected as two: after the call the observation sets and the point count are the
    unsplit world's, one point absorbed per split; a second call changes nothing (a property of this noise-free world).  (8) On the
    fused map track_local_map, relocalize and bundle_adjust agree with their restatements on the fused arrays, the co-visibility
    graph equals the recount, and the cull of a further keyframe keeps every fused point with two observations.  The bundle
    adjustment is compared at max_steps = (0, 0): the problem fusion changes - free and fixed keyframes, local points, edges and
    their classification - in exact integers; its arithmetic has tests of its own."""
    from tests.ba_restatement import bundle_adjust as restate_ba
    from tests.reloc_restatement import restate as restate_reloc
    ctx = _ctx()
    w, unsplit, n_split = FW.split_world()
    size = w.image_size
    m = build_map(ctx, w)
    lists0 = _snapshot(m)[1]
    info, want, cnt, before = _fuse_equals_restatement(m, size, window=0)
    assert n_split > 100 and info["n_absorbed"] == n_split and info["n_points"] == len(unsplit.obs) and info["n_gained"] == 0
    a = m.arrays()
    u = FW.world_inputs(unsplit)[0]
    assert sorted(map(sorted, FW.obs_sets(a, w.counts))) == sorted(map(sorted, FW.obs_sets(u, w.counts)))
    assert np.array_equal(np.sort(a["id"]), np.sort(u["id"]))
    assert all(np.array_equal(x, y) for x, y in zip(_snapshot(m)[1], lists0))   # the per-keyframe lists stay those of the last cull
    # the co-visibility graph: empty before (no growth step found a model), the recount's changes after
    delta = FR.co_visibility_delta(before, want, info["into"], w.counts)
    assert delta and all(d > 0 for d in delta.values())
    g = m.co_visibility_graph
    assert {(p, q): g[p][q] for p in g for q in g[p] if p < q and g[p][q]} == delta
    assert all(g[q][p] == d for (p, q), d in delta.items())
    # a second call
    snap = _snapshot(m)
    info2, _, _, _ = _fuse_equals_restatement(m, size, window=0)
    assert info2["n_proposals"] == info2["n_absorbed"] == info2["n_gained"] == 0 and np.array_equal(info2["into"], np.arange(info["n_points"]))
    again = _snapshot(m)
    assert all(np.array_equal(again[0][f], snap[0][f]) for f in snap[0])
    # downstream: tracking and relocalization read the fused map
    T = pose_near(w, 4)
    kps, desc = unsplit.world0.track_query(T, wrong=0.0)
    pose0 = perturbed_pose(T)
    ok, pose, ti = m.track_local_map(kps, desc, pose0, radii=(15.0,), image_size=size)
    r = TR.track(w.K, pose0, a["xyz"], a["obs_off"], a["obs_kf"], a["obs_kp"], w.kf_desc, w.kf_oct, kps, desc, size[0], size[1], radii=(15.0,),
                 refine_pose=False)
    assert ti["n_local"] == r["n_local"] and np.array_equal(ti["point"], r["passes"][0]["point"]) and np.array_equal(ti["dist"], r["passes"][0]["dist"])
    assert r["passes"][0]["matches"] >= 20
    qk, qd = unsplit.world0.reloc_query(3, w.kf_poses[3])
    okr, rpose, ri = m.relocalize(qk, qd)
    rr = restate_reloc(qd, w.kf_desc, a["obs_off"], a["obs_kf"], a["obs_kp"], 0.75, 4)
    assert [c[0] for c in ri["candidates"]] == rr["candidates"] and [c[1] for c in ri["candidates"]] == [rr["scores"][p] for p in rr["candidates"]]
    assert okr and ri["kf_pos"] == 3
    # bundle adjustment: the problem on the fused arrays
    okb, bi = m.bundle_adjust(window=6, max_steps=(0, 0), want_points=True)
    rb = restate_ba(a["obs_off"], a["obs_kf"], a["obs_kp"], w.counts, w.kf_xy, w.kf_oct, a["xyz"], w.K, np.array([T_[:3, :4] for T_ in w.kf_poses]),
                    window=6, max_steps=(0, 0))
    for k in ("n_free", "n_fixed", "n_local", "n_edges", "n_inliers", "free", "fixed"):
        assert bi[k] == rb[k], (k, bi[k], rb[k])
    assert np.array_equal(bi["edge_inlier"], rb["edge_inlier"]) and bi["n_edges"] > 100
    # a further keyframe: its cull keeps every fused point with two observations (noise-free: reprojection errors ~ 1e-5 px)
    rng = np.random.default_rng(3)
    kp = kps_array(np.column_stack([rng.uniform(0, size[0], 200), rng.uniform(0, size[1], 200)]))
    m.add_keyframe(np.zeros((size[1], size[0]), np.uint8), kp, rng.integers(0, 256, (200, 32)).astype(np.uint8), w.kf_poses[-1])
    assert m.last["n_new"] == 0
    two = np.diff(a["obs_off"]) >= 2
    b = m.arrays()
    assert np.array_equal(b["id"], a["id"][two]) and np.array_equal(b["xyz"], a["xyz"][two])
    assert ctx.dev_status() == 0
    m.close(); ctx.close()


def test_withheld_observations_are_gained_and_a_contested_row_goes_to_one_point():
    """(2) the third observation of every three-view point is missing from the map, its keypoint is still in the keyframe: the call
    restores it.  Five such points have two more points at their place: three proposals for one free keypoint, one winner - the
    lowest (distance, index) by the restatement - and the three merge."""
    ctx = _ctx()
    w, held = FW.withheld_world()
    m = build_map(ctx, w)
    info, want, cnt, _ = _fuse_equals_restatement(m, w.image_size, window=0)
    assert info["n_gained"] == len(held) and info["n_proposals"] > info["n_gained"] + info["n_edges"]   # proposals lost their row
    assert info["n_absorbed"] == 10
    lists = FR.lists_of(m.arrays())
    for i, k, r in held:
        assert (k, r) in lists[info["into"][i]]
    assert ctx.dev_status() == 0
    m.close(); ctx.close()


def _hand(ctx, kfs, xyz, obs, capacity=None):
    from tests.test_fuse_cpu import K, _poses
    return FW.hand_map(ctx, K, _poses(), kfs, xyz, obs, capacity=capacity)


def test_components_on_hand_made_maps():
    """(3) the chains and conflicts of tests/test_fuse_cpu.py on the device: survivor by observation count, then by index; an entry at a
    position the survivor holds is dropped; stale and negative keys stay on the survivor and leave with an absorbed member"""
    from tests.test_fuse_cpu import CHAIN_XYZ, D0, LINE
    ctx = _ctx()
    cases = [
        ([[(50, 50, D0)], [(50.875, 50, D0)], [(51.75, 50, D0)]], CHAIN_XYZ, [[(0, 0)], [(1, 0)], [(2, 0)]], [[(0, 0), (1, 0), (2, 0)]], [100]),
        ([[(50, 50, D0), (53.75, 50, D0)], [(50.875, 50, D0)], [(51.75, 50, D0)]], CHAIN_XYZ, [[(0, 0)], [(1, 0)], [(2, 0), (0, 1)]],
         [[(2, 0), (0, 1), (1, 0)]], [102]),
        ([[(50, 50, D0)], [(49, 50, D0), (50, 50, D0)], [(48, 50, D0)]], [[0, 0, 10]] * 2, [[(0, 0), (1, 0)], [(1, 1), (2, 0)]],
         [[(0, 0), (1, 0), (2, 0)]], [100]),
        (LINE, [[0, 0, 10]] * 2, [[(0, 0), (7, 3), (-2, 0)], [(1, 5), (-1, 0)]], [[(0, 0), (7, 3), (-2, 0), (2, 0)]], [100]),
    ]
    for kfs, xyz, obs, lists, ids in cases:
        m = _hand(ctx, kfs, xyz, obs)
        info, _, _, _ = _fuse_equals_restatement(m, (100, 100), window=0)
        a = m.arrays()
        assert FR.lists_of(a) == lists and a["id"].tolist() == ids and info["into"].tolist() == [0] * len(obs)
        m.close()
    assert ctx.dev_status() == 0
    ctx.close()


@pytest.mark.parametrize("decorated", [False, True], ids=["clean", "stale"])
def test_position_is_not_slot(decorated):
    """(4) positions (1, 4) removed: from position 1 on a keyframe's slot is not its position.  The split world is put together again;
    read without the table (position p taken for slot p: other keypoints, descriptors and P) the restatement gives another map, so a
    kernel that skipped pos_slot fails here.  Stale variant: the same map with keys counted from the end, keys naming no keyframe or
    no row, mixed in (tests/fuse_worlds.py: decorate)."""
    from orbslam2.utils import compute_projection_matrix
    ctx = _ctx()
    w, unsplit, n_split = FW.split_world(removed=(1, 4), seed=43)
    if decorated:
        FW.decorate(w)
        kinds = [(k < 0, r < 0, k >= 50) for k, r in zip(w.obs_kf.tolist(), w.obs_kp.tolist())]
        assert min(sum(x[j] for x in kinds) for j in range(3)) >= 20
    m = build_map(ctx, w)
    assert [w.survivors[p] != p for p in range(len(w.survivors))].count(True) >= 6
    info, want, cnt, before = _fuse_equals_restatement(m, w.image_size, window=0)
    assert info["n_absorbed"] >= (0.5 if decorated else 1.0) * n_split > 50
    if not decorated:
        assert info["n_points"] == len(unsplit.obs)
    xy, octv, desc, poses = w.slot_order()
    P = [np.ascontiguousarray(compute_projection_matrix(T[:3, :3], T[:3, 3], w.K), np.float64) for T in poses]
    a0, _, _, _, _ = FW.world_inputs(w)
    wrong = FR.fuse(a0, P, xy, octv, desc, w.image_size[0], w.image_size[1], window=0)
    assert wrong[2] != cnt and len(wrong[0]["id"]) != cnt["n_points"]
    assert ctx.dev_status() == 0
    m.close(); ctx.close()


def test_octaves_radius_and_gates():
    """(5) reference octave 2 (both observations at octave 2), free keypoints in keyframe 2.  With chi2 out of the way (1e9):
    r = 3 * 1.2^2 = 4.32: a keypoint 4.30 px off is gained, one 4.34 px off is not; at the projection, octave 3 is gained and octave 4
    is not.  With chi2 = 5.991 and the keypoint's octave 2 the gate is 3.5246 px: 3.50 gained, 3.55 not."""
    from tests.test_fuse_cpu import _desc
    ctx = _ctx()
    d = [_desc(c) for c in range(4)]
    ys = (20, 40, 60, 80)   # points (0, b, 10), b = -3, -1, 1, 3
    xyz = [[0, (v - 50) / 10.0, 10] for v in ys]
    obs = [[(0, j), (1, j)] for j in range(4)]

    def scene(free):
        return [[(50, v, d[j], 2) for j, v in enumerate(ys)], [(49, v, d[j], 2) for j, v in enumerate(ys)],
                [(48 + dx, v, d[j], o) for j, (v, (dx, o)) in enumerate(zip(ys, free))]]
    for free, kw, gained in (([(4.30, 2), (4.34, 2), (0, 3), (0, 4)], {"chi2": 1e9}, [True, False, True, False]),
                             ([(3.50, 2), (3.55, 2), (3.50, 3), (5.10, 3)], {}, [True, False, True, False])):
        m = _hand(ctx, scene(free), xyz, obs)
        info, _, cnt, _ = _fuse_equals_restatement(m, (100, 100), window=0, **kw)
        assert cnt["n_pairs"] == cnt["n_cand"] == 4
        lists = FR.lists_of(m.arrays())
        assert [(2, j) in lists[j] for j in range(4)] == gained, lists
        # the scale factor in r and in the information: at 1.0 the radius is 3 and the chi2 gate 2.45 px, nothing is gained
        m2 = _hand(ctx, scene(free), xyz, obs)
        i2, _, _, _ = _fuse_equals_restatement(m2, (100, 100), window=0, scale_factor=1.0, **kw)
        assert i2["n_gained"] == sum(1 for dx, o in free if dx == 0 and o <= 3)
        m.close(); m2.close()
    assert ctx.dev_status() == 0
    ctx.close()


def test_window_of_three_on_ten_keyframes():
    """(6) only positions 7, 8, 9 receive proposals: the withheld observations there come back, those at earlier positions do not;
    points without an observation in the window keep their bytes"""
    ctx = _ctx()
    w, held = FW.withheld_world()
    m = build_map(ctx, w)
    info, want, cnt, before = _fuse_equals_restatement(m, w.image_size, window=3)
    assert info["n_targets"] == 3 and 0 < info["n_local"] < len(w.obs)
    a = m.arrays()
    lists, lists0 = FR.lists_of(a), FR.lists_of(before)
    back = [(k, r) in lists[info["into"][i]] for i, k, r in held]
    assert any(back) and all(k >= 7 for (i, k, r), b in zip(held, back) if b) and not all(back)
    assert all(b for (i, k, r), b in zip(held, back) if k >= 7 and any(kk >= 7 for kk in w.obs[i]))
    outside = [i for i, o in enumerate(w.obs) if all(k < 7 for k in o)]
    assert len(outside) > 50
    for i in outside:
        j = info["into"][i]
        assert lists[j] == lists0[i] and a["xyz"][j].tobytes() == before["xyz"][i].tobytes() and a["id"][j] == before["id"][i]
    assert ctx.dev_status() == 0
    m.close(); ctx.close()


def test_no_work_determinism_and_growth_from_a_tiny_capacity():
    """(7) an empty map, keyframes without points, a map with nothing to fuse: nothing is written, the proposal counts are 0.  Two maps
    built alike give the same bytes; a map made with capacities every store outgrows gives them too."""
    from vslam_amd.mapper import LocalMapper
    ctx = _ctx()
    w, unsplit, _ = FW.split_world()
    m = LocalMapper(w.K, save_every_keyframe=False, context=ctx)
    info = m.fuse_map_points(image_size=w.image_size)
    assert all(info[k] == 0 for k in FR.COUNTS) and len(info["into"]) == 0
    m.add_keyframe(np.zeros((480, 640), np.uint8), kps_array(w.slot_xy[0]), w.slot_desc[0], w.slot_poses[0])
    info = m.fuse_map_points(image_size=w.image_size)
    assert all(info[k] == 0 for k in FR.COUNTS)
    m.close()
    m = build_map(ctx, unsplit)
    snap = _snapshot(m)
    info, _, cnt, _ = _fuse_equals_restatement(m, w.image_size, window=0)
    assert cnt["n_pairs"] > 1000 and all(info[k] == 0 for k in ("n_proposals", "n_gained", "n_edges", "n_absorbed"))
    assert np.array_equal(info["into"], np.arange(len(unsplit.obs)))
    again = _snapshot(m)
    assert all(again[0][f].tobytes() == snap[0][f].tobytes() for f in snap[0]) and all(np.array_equal(x, y) for x, y in zip(again[1], snap[1]))
    m.close()
    out = []
    for cap in (None, None, TINY):
        m = build_map(ctx, w, capacity=cap)
        info = m.fuse_map_points(image_size=w.image_size, window=0)
        a = m.arrays()
        out.append([a[f].tobytes() for f in FR.FIELDS] + [info["into"].tobytes()] + [info[k] for k in FR.COUNTS])
        m.close()
    assert out[0] == out[1] == out[2] and out[0][-3] > 100   # (n_absorbed)
    assert ctx.dev_status() == 0
    ctx.close()


# ---- keyframes past 1024 rows (tests/fuse_worlds.py: large_split_world, row_cases) ---------------------------------------------------------
def test_large_split_world_is_put_together_again():
    """(9) the split world at the mapper's keyframe size, rows [921, 1117, 1924, 1830]: three targets past 1024 rows (k_trk_grid's strided
    loops take a second trip, keypoints in rows >= 1024 are matched and owned).  One point absorbed per split, the observation sets
    are the unsplit world's"""
    ctx = _ctx()
    w, unsplit, n_split = FW.large_split_world()
    m = build_map(ctx, w)
    assert (w.counts > 1024).sum() >= 2
    info, want, cnt, before = _fuse_equals_restatement(m, w.image_size, window=0)
    assert n_split > 1000 and info["n_absorbed"] == n_split and info["n_points"] == len(unsplit.obs) and info["n_gained"] == 0
    a = m.arrays()
    u = FW.world_inputs(unsplit)[0]
    assert sorted(map(sorted, FW.obs_sets(a, w.counts))) == sorted(map(sorted, FW.obs_sets(u, w.counts)))
    assert np.array_equal(np.sort(a["id"]), np.sort(u["id"]))
    assert ctx.dev_status() == 0
    m.close(); ctx.close()


def test_large_stale_world_position_is_not_slot():
    """(10) six keyframes of up to 1785 rows, position 1 removed, keys decorated: slot != position behind tables strided by the row
    capacity, read past row 1024"""
    from orbslam2.utils import compute_projection_matrix
    ctx = _ctx()
    w, unsplit, n_split = FW.large_split_world(stale=True)
    m = build_map(ctx, w)
    assert [w.survivors[p] != p for p in range(len(w.survivors))].count(True) == 4 and (w.counts > 1024).sum() >= 3
    info, want, cnt, before = _fuse_equals_restatement(m, w.image_size, window=0)
    assert info["n_absorbed"] >= 0.5 * n_split > 500
    xy, octv, desc, poses = w.slot_order()
    P = [np.ascontiguousarray(compute_projection_matrix(T[:3, :3], T[:3, 3], w.K), np.float64) for T in poses]
    wrong = FW.restate_world(w, lists=(xy, octv, desc, P), window=0)
    assert wrong[2] != cnt and wrong[2]["n_points"] != cnt["n_points"]
    assert ctx.dev_status() == 0
    m.close(); ctx.close()


def test_row_cases_on_hand_made_maps():
    """(11) the row cases of tests/test_fuse_cpu.py on the device: the matched keypoint in the last row of targets of 1025 and 2049 rows,
    free and owned; 200 keypoints of a 1500-row target in the cell under the projection with a tie for the best; a target without a row"""
    ctx = _ctx()
    for name, (kfs, xyz, obs, want) in sorted(FW.row_cases().items()):
        m = _hand(ctx, kfs, xyz, obs)
        info, _, _, _ = _fuse_equals_restatement(m, (100, 100), window=0)
        assert FW.missed(want, m.arrays(), info["into"], {k: info[k] for k in FR.COUNTS}) == [], (name, info)
        m.close()
    assert ctx.dev_status() == 0
    ctx.close()
