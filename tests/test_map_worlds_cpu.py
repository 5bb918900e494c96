"""The worlds of tests/map_worlds.py, checked in numpy on the restatements alone: what tests/test_gpu_map_reads.py asks of the device
is only worth asking when the expected result differs from what a kernel without the rule under test would produce.  Each test prints
how many entries tell the two apart.  No GPU."""
import numpy as np

from tests import track_restatement as TR
from tests.map_worlds import (BA_FIRST_FREE, PRE_N, PRE_QUERIES, PRE_WORDS, REMOVED, STALE_BA_STEPS, ba_case, ba_problem_edges, ba_restated,
                              clean_reloc_query, clean_vocabulary, cull_after_ba, decisions_are_clear, perturbed, perturbed_pose, pose_near,
                              project, stale_queries, track, world)
from tests.reloc_restatement import restate

def test_the_builder_is_consistent():
    """clean world, removed (1, 4) of 10 keyframes: position != slot; the lists by position are the store's slots read through the table
    mo_map_remove_keyframes leaves; every key names the keypoint its point projects to; no two neighbouring keyframes (in the store's
    order or the survivors') share a point, so no growth step finds a model in the map or in its twin; observation counts, ties"""
    w = world("clean")
    pos_slot = list(range(w.n_kf0))
    for p in sorted(REMOVED, reverse=True):
        pos_slot.pop(p)
    assert pos_slot == w.survivors and 8 <= len(pos_slot) <= 10 and any(p != s for p, s in enumerate(pos_slot))
    twin_desc, twin_xy = [w.slot_desc[s] for s in pos_slot], [w.slot_xy[s] for s in pos_slot]
    assert all(np.array_equal(a, b) for a, b in zip(twin_desc, w.kf_desc)) and all(np.array_equal(a, b) for a, b in zip(twin_xy, w.kf_xy))
    assert len(set(len(d) for d in w.slot_desc)) > 1   # keypoint counts differ
    for i, o in enumerate(w.obs):
        for k, r in o.items():
            xy, z = project(w.K, w.kf_poses[k], w.xyz[i:i + 1])
            assert z[0] > 0 and np.abs(xy[0] - w.kf_xy[k][r]).max() < 1e-3
    by_slot = [set() for _ in range(w.n_kf0)]
    for o, j in zip(w.obs, w.world):
        for k in o:
            by_slot[w.survivors[k]].add(int(j))
    for a, b in list(zip(range(w.n_kf0 - 1), range(1, w.n_kf0))) + list(zip(w.survivors[:-1], w.survivors[1:])):
        assert not by_slot[a] & by_slot[b], (a, b)
    cnt = np.bincount([len(o) for o in w.obs])
    assert cnt[1] > 0 and cnt[2] > 0 and cnt[3] > 0 and len(w.ties) >= 10
    b = world("ba")
    cb = np.bincount([len(o) for o in b.obs], minlength=7)
    print("observations per point: skip world %s, consecutive world %s" % (cnt.tolist(), cb.tolist()))
    assert (cb[1:7] > 0).all() and any(len(b.obs[b.index_of[j]]) == 4 for j, _, _ in b.ties)
    # the restatements on the twin's lists: the same results (the twin's lists are the same arrays read through the table)
    T = pose_near(w, 4)
    kps, desc = w.track_query(T)
    r0 = track(w, kps, desc, perturbed_pose(T), radii=(15.0,), refine_pose=False)
    r1 = track(w, kps, desc, perturbed_pose(T), lists=(twin_xy, [w.slot_oct[s] for s in pos_slot], twin_desc, None), radii=(15.0,), refine_pose=False)
    assert np.array_equal(r0["passes"][0]["point"], r1["passes"][0]["point"]) and r0["passes"][0]["matches"] >= 100
    qk, qd = w.reloc_query(3, pose_near(w, 3))
    ra, rb = (restate(qd, d, w.obs_off, w.obs_kf, w.obs_kp) for d in (w.kf_desc, twin_desc))
    assert ra["candidates"] == rb["candidates"] and ra["candidates"][0] == 3
    assert ba_problem_edges(b) == ba_problem_edges(b, lists=([b.slot_xy[s] for s in b.survivors],))


def test_skipping_the_table_changes_every_read_path():
    """what a kernel reading slot = position would produce: the restatements fed the store's slots in place of the positions"""
    w = world("clean")
    lists = w.slot_order()
    pos = 3   # the keyframe at position 3 sits in slot 5
    qk, qd = w.reloc_query(pos, pose_near(w, pos))
    right, wrong = restate(qd, w.kf_desc, w.obs_off, w.obs_kf, w.obs_kp), restate(qd, lists[2], w.obs_off, w.obs_kf, w.obs_kp)
    assert right["candidates"][0] == pos
    c_r, c_w = right["C"][pos], wrong["C"][pos]
    n_c = len(set(zip(*[a.tolist() for a in c_r])) ^ set(zip(*[a.tolist() for a in c_w])))
    print("relocalization: candidates %s against %s; %d correspondences of keyframe %d differ" % (right["candidates"], wrong["candidates"], n_c, pos))
    assert right["candidates"] != wrong["candidates"] or n_c > 0
    assert n_c > 0
    T = pose_near(w, 4)
    kps, desc = w.track_query(T)
    for window in (3, 0):
        a = track(w, kps, desc, perturbed_pose(T), window=window, radii=(15.0,), refine_pose=False)["passes"][0]
        b = track(w, kps, desc, perturbed_pose(T), lists=lists, window=window, radii=(15.0,), refine_pose=False)["passes"][0]
        n_t = int((a["point"] != b["point"]).sum() + ((a["point"] == b["point"]) & (a["dist"] != b["dist"])).sum())
        print("track, window %d: %d of %d pass-1 entries differ (%d matches)" % (window, n_t, len(kps), a["matches"]))
        assert n_t > 0 and a["matches"] >= 20
    bw = world("ba")
    fr, fx, e_r = ba_problem_edges(bw)
    _, _, e_w = ba_problem_edges(bw, lists=bw.slot_order())
    n_e = len(set(e_r) ^ set(e_w))
    print("bundle adjustment: %d edges against %d, %d differ; free %s fixed %s" % (len(e_r), len(e_w), n_e, fr, fx))
    assert n_e > 0
    # a free and a fixed keyframe sit in a slot that is not their position
    assert any(bw.survivors[p] != p for p in fr) and any(bw.survivors[p] != p for p in fx)


def test_the_preselection_keeps_the_true_keyframe_on_the_clean_world():
    """the premise of test_relocalize_preselected_after_removal (tests/test_gpu_map_reads.py): with PRE_WORDS words the restated query
    ranks the true position among the first PRE_N for each of its queries, so relocalize(preselect=PRE_N) has the plain call's winner
    among the keyframes it matches; and the clean world's position -> slot table is not the identity at two of the three positions"""
    from tests import bow_restatement as B
    w = world("clean")
    words, weights, _ = clean_vocabulary()
    assert len(words) == PRE_WORDS and PRE_N < len(w.survivors)
    for pos in PRE_QUERIES:
        _, qd, _ = clean_reloc_query(pos)
        first, sc = B.query(qd, w.kf_desc, words, weights, len(w.survivors))
        print("query near position %d (slot %d): first %s scores %s" % (pos, w.survivors[pos], first[:PRE_N + 1], ["%.3f" % x for x in sc[:PRE_N + 1]]))
        assert pos in first[:PRE_N], (pos, first)
        assert len(set(sc[:PRE_N + 1])) == len(sc[:PRE_N + 1])   # no tie at the cut: the selection does not hang on a tie rule
    assert sum(w.survivors[p] != p for p in PRE_QUERIES) >= 2


def test_the_octave_world_tells_the_gate_the_scaling_and_the_weights():
    w = world("octave")
    T = pose_near(w, 4)
    for sf in (1.2, 1.5):
        kps, desc = w.track_query(T, octave_spread=2, seed=6)
        assert set(np.unique(kps["octave"] - 0).tolist()) >= set(range(0, 9))
        pose0 = perturbed_pose(T)
        kw = dict(radii=(6.0,), refine_pose=False, scale_factor=sf)   # (pose0 puts the projections up to 13 px off: the scaling decides)
        a = track(w, kps, desc, pose0, **kw)["passes"][0]
        g = track(w, kps, desc, pose0, octave_gate=False, **kw)["passes"][0]
        s = track(w, kps, desc, pose0, scale_radius=False, **kw)["passes"][0]
        n_g, n_s = int((a["point"] != g["point"]).sum()), int((a["point"] != s["point"]).sum())
        print("scale factor %.1f: %d matches; without the gate %d entries differ, with the radius unscaled %d" % (sf, a["matches"], n_g, n_s))
        assert n_g > 0 and n_s > 0 and a["matches"] >= 20
        q = np.flatnonzero(a["point"] >= 0)
        X, x = w.xyz[a["point"][q]].astype(np.float64), np.column_stack([kps["x"][q], kps["y"][q]]).astype(np.float64)
        Tr, inl, _ = TR.refine(w.K, pose0, X, x, kps["octave"][q], scale_factor=sf)
        Tu, inl_u, _ = TR.refine(w.K, pose0, X, x, kps["octave"][q], scale_factor=sf, unit_information=True)
        moved = not np.allclose(Tr, Tu, rtol=1e-9, atol=1e-9)
        print("scale factor %.1f: with unit weights %d inlier flags differ, pose moves by %.3g" % (sf, int((inl != inl_u).sum()), np.abs(Tr - Tu).max()))
        assert (inl != inl_u).any() or moved


def test_the_stale_world_holds_every_kind_of_key_and_the_calls_still_proceed():
    for name in ("stale", "ba_stale"):
        w = world(name)
        kinds = w.key_kinds()
        print("%s world: %s" % (name, kinds))
        assert all(kinds[k] > 0 for k in ("position_out_of_range", "row_out_of_range", "negative_position", "negative_row", "valid"))
    w = world("stale")
    T, (kps, desc), pos, (qk, qd) = stale_queries(w)
    r = track(w, kps, desc, perturbed_pose(T), radii=(15.0,), refine_pose=False)
    assert r["n_local"] >= 30 and r["passes"][0]["matches"] >= 20, (r["n_local"], r["passes"][0]["matches"])   # min_inliers, min_matches
    rr = restate(qd, w.kf_desc, w.obs_off, w.obs_kf, w.obs_kp)
    assert rr["candidates"] and rr["scores"][rr["candidates"][0]] >= 50, rr["scores"]
    b = world("ba_stale")
    fr, fx, e = ba_problem_edges(b)
    trace = []
    poses, xyz = perturbed(b, first_free=BA_FIRST_FREE)
    rb = ba_restated(b, poses, xyz, max_steps=STALE_BA_STEPS, trace=trace)
    decisions_are_clear(trace)
    assert rb["accepted"][0] > 0 and rb["steps"][0] > rb["accepted"][0]
    print("stale worlds: track %d local, %d matches; relocalization scores %s; bundle adjustment %d edges, free %s" %
          (r["n_local"], r["passes"][0]["matches"], rr["scores"], len(e), fr))
    assert fr and len(e) >= 50
    # the slot-order reading differs here too
    r2 = track(w, kps, desc, perturbed_pose(T), lists=w.slot_order(), radii=(15.0,), refine_pose=False)
    assert (r["passes"][0]["point"] != r2["passes"][0]["point"]).any()


def test_the_cull_after_bundle_adjustment_sees_the_write_back():
    c = ba_case()
    w, ref = c["w"], c["ref"]
    assert ref["ok"] and ref["free"] and ref["accepted"][0] > 0 and ref["accepted"][1] > 0
    decisions_are_clear(c["trace"])
    seen_free = np.array([any((k if k >= 0 else k + len(w.survivors)) in ref["free"] for k in o) for o in w.obs])
    keep_none, _ = cull_after_ba(w, c["poses"], ref, "none")
    keep_slot, near = cull_after_ba(w, c["poses"], ref, "slot")
    keep_pos, _ = cull_after_ba(w, c["poses"], ref, "position")
    n1, n2 = int((keep_none != keep_slot)[seen_free].sum()), int((keep_slot != keep_pos).sum())
    print("cull after BA: %d of %d points kept; %d decisions differ from the unrefined poses, %d from a write-back at kP[position]; %d within "
          "1e-9 px of the threshold" % (keep_slot.sum(), len(keep_slot), n1, n2, near.sum()))
    assert n1 > 0 and n2 > 0 and near.sum() < 10
