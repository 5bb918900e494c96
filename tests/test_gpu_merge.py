"""LocalMapper.merge_map on the GPU.  The loop world mapped in two sessions (tests/merge_worlds.split), the second in a frame of its own
(its side rescaled by 1.3): merge_map aligns the absorbed side onto the absorbing one, with the integer results of the one-session
world run through the same calls, and puts the absorbed keyframes and the surviving duplicates back at the unscaled world within
tests/correct_worlds.TRUTH_BOUND; the merged mapper round-trips through its file.  A map of random rows does not align and leaves
the absorbing map as it was.  The driver merges a run into a saved one."""
import numpy as np
import pytest

from tests import correct_worlds as CW
from tests import loop_worlds as LW
from tests import merge_worlds as MW

pytestmark = pytest.mark.gpu

FACTOR = 1.3
SEED = 11


def _ctx():
    import vslam_amd as V
    return V.Context(device=0, max_w=640, max_h=480, max_batch=1)


def _same(a, b, tag):
    from tests.test_gpu_scratch_poison import _flat, _same as same
    same(_flat(a), _flat(b), tag)


COUNTS = ("n_corrected", "n_moved", "n_loop_points", "n_direct_edges", "n_direct_gained", "n_pairs", "n_cand", "n_proposals", "n_gained", "n_edges",
          "n_absorbed", "n_points", "n_obs")


def test_merge_aligns_a_map_built_in_its_own_frame(tmp_path):
    import vslam_amd as V
    from tests.test_gpu_sim3 import _rescaled
    from vslam_amd.mapper import LocalMapper
    ctx = _ctx()
    base = LW.loop_world()
    wr = _rescaled(base, FACTOR)
    words, weights = LW.loop_vocabulary()
    voc = V.Vocabulary.from_arrays(words, weights, context=ctx)
    A, B = MW.split(wr)
    mA, mB = A.build(ctx), B.build(ctx)
    mA.set_vocabulary(voc)
    res = mA.merge_map(mB, sim3_kw=dict(seed=SEED))
    assert res["aligned"] and res["kept"] and res["kf_pos"] == 26 and 0 <= res["cand_pos"] < MW.SPLIT and res["tries"] == 1
    assert abs(res["scale"] - 1.0 / FACTOR) < 1e-3 or abs(res["scale"] - FACTOR) < 1e-3
    co = res["correct"]
    absorbed = list(range(MW.SPLIT, LW.N_KF))
    assert co["corrected"] == absorbed and not set(co["group"]) & set(absorbed) and all(k < MW.SPLIT for k in co["group"])
    # the one-session world through the same calls with the same explicit masks
    m1 = wr.build(ctx)
    m1.set_vocabulary(voc)
    own = np.arange(LW.N_KF) < MW.SPLIT
    info = m1.loop_candidates(26, among=own)
    ok1, al = m1.compute_sim3(info, seed=SEED)
    ok2, cf = m1.confirm_loop(info, al)
    assert ok1 and ok2
    ref = m1.correct_loop(cf, kf_position=26, corrected=absorbed, group=info["candidates"][int(cf["win"])]["group"])
    assert {k: co[k] for k in COUNTS} == {k: ref[k] for k in COUNTS}, ({k: co[k] for k in COUNTS}, {k: ref[k] for k in COUNTS})
    assert np.array_equal(co["into"], ref["into"]) and np.array_equal(co["moved"], ref["moved"])
    assert co["group"] == ref["group"] and res["cand_pos"] == int(cf["candidates"][int(cf["win"])]["pos"])
    assert co["n_absorbed"] >= 40 and co["n_corrected"] == len(absorbed)
    # against the unscaled world: the ids of the absorbed side back in the one-session numbering
    after = mA.arrays()
    id_off = res["offsets"]["id_offset"]
    ids = np.where(after["id"] >= id_off, after["id"] - id_off, after["id"])
    named, wrong, old_moved, e = CW.facts(wr, base, {"into": co["into"], "moved": co["moved"], "xyz": after["xyz"], "ids": ids, "poses": co["poses"],
                                                     "loop_point": cf["loop_point"]})
    print("merge: %s; %d named duplicates absorbed; error to the unscaled world %.3g (bound %.3g)" % ({k: co[k] for k in COUNTS}, named, e, CW.TRUTH_BOUND))
    assert named >= 40 and wrong == [] and old_moved == 0
    assert e <= CW.TRUTH_BOUND, e
    for k in LW.RETURN_POS:
        assert np.abs(np.asarray(mA.keyframes[k]["pose"], np.float64)[:3, :4] - np.asarray(base.kf_poses[k], np.float64)[:3, :4]).max() <= CW.TRUTH_BOUND
    for k in range(MW.SPLIT):
        assert np.asarray(mA.keyframes[k]["pose"], np.float64).tobytes() == np.asarray(A.kf_poses[k], np.float64).tobytes()
    # the merged mapper through its file
    path = str(tmp_path / "merged.npz")
    mA.save_state(path)
    back = LocalMapper.load_state(path, context=ctx)
    _same(back.export_state(), mA.export_state(), "file")
    assert [kf["id"] for kf in back.keyframes] == [kf["id"] for kf in mA.keyframes] == list(range(LW.N_KF))
    assert back._kf_serials == mA._kf_serials and back._next_serial == mA._next_serial == LW.N_KF
    assert {a: dict(b) for a, b in back.co_visibility_graph.items() if b} == {a: dict(b) for a, b in mA.co_visibility_graph.items() if b}
    _same(back.loop_candidates(24), mA.loop_candidates(24), "loaded answers")
    assert len(back.map_points) == len(mA.map_points) and back.map_points[5]["id"] == mA.map_points[5]["id"]
    assert ctx.dev_status() == 0
    for m in (mA, mB, m1, back):
        m.close()
    voc.close(); ctx.close()


def test_a_map_of_random_rows_does_not_align_and_is_taken_out_again():
    import vslam_amd as V
    from tests.map_worlds import kps_array
    from tests.test_gpu_snapshot import _rand_kf
    from vslam_amd.mapper import LocalMapper
    ctx = _ctx()
    w = LW.loop_world()
    words, weights = LW.loop_vocabulary()
    voc = V.Vocabulary.from_arrays(words, weights, context=ctx)
    A, _ = MW.split(w)
    mA = A.build(ctx)
    mA.set_vocabulary(voc)
    rng = np.random.default_rng(77)
    src = LocalMapper(w.K, save_every_keyframe=False, context=ctx, n_hyp=8, capacity=(4, 64, 64, 128))
    for _ in range(3):
        _rand_kf(src, rng, 120, size=w.image_size)
    src.update_map_points([{"id": i, "position": rng.normal(0, 2, 3), "color": np.zeros(3, np.uint8),
                            "observed_keyframes": {0: int(rng.integers(0, 120)), 2: int(rng.integers(0, 120))}} for i in range(30)])
    before = {k: v.copy() for k, v in mA.arrays().items()}
    kfs = [(kf["id"], kf["pose"].copy(), kf._rows) for kf in mA.keyframes]
    serials, graph = list(mA._kf_serials), {a: dict(b) for a, b in mA.co_visibility_graph.items() if b}
    with pytest.raises(ValueError, match="vocabulary"):
        src.merge_map(mA)
    res = mA.merge_map(src, max_tries=2)
    assert not res["aligned"] and not res["kept"] and res["correct"] is None and res["kf_pos"] == -1
    assert res["tries"] == 2   # the absorbed positions 2 and 0 hold the points; position 1 has none and is passed over
    _same(mA.arrays(), before, "arrays after a failed merge")
    assert [(kf["id"], kf["pose"].tobytes(), kf._rows) for kf in mA.keyframes] == [(i, p.tobytes(), r) for i, p, r in kfs]
    assert mA._kf_serials == serials and {a: dict(b) for a, b in mA.co_visibility_graph.items() if b} == graph
    assert mA._next_serial == MW.SPLIT + 3   # nothing is rewound: the serials of the absorbed keyframes are spent
    # the map goes on: a keyframe, a tracked frame
    n = 80
    xy = np.column_stack([rng.uniform(0, w.image_size[0], n), rng.uniform(0, w.image_size[1], n)])
    mA.add_keyframe(np.zeros((w.image_size[1], w.image_size[0]), np.uint8), kps_array(xy), rng.integers(0, 256, (n, 32)).astype(np.uint8), np.eye(4))
    assert len(mA.keyframes) == MW.SPLIT + 1 and mA._kf_serials[-1] == MW.SPLIT + 3
    ok, pose, info = mA.track_local_map(kps_array(w.kf_xy[3]), w.kf_desc[3], w.kf_poses[3], window=0)
    print("tracked behind the failed merge: ok %s, %d inliers of %d local points" % (ok, int(info["inlier"].sum()), info["n_local"]))
    assert ok and np.abs(pose - w.kf_poses[3]).max() < 1e-3 and int(info["inlier"].sum()) >= 50
    # keep_unaligned: the absorbed side stays, unaligned
    res = mA.merge_map(src, max_tries=1, keep_unaligned=True)
    assert not res["aligned"] and res["kept"] and len(mA.keyframes) == MW.SPLIT + 4 and len(mA.map_points) == res["offsets"]["point_offset"] + 30
    assert ctx.dev_status() == 0
    mA.close(); src.close(); voc.close(); ctx.close()


def test_the_driver_merges_a_run_into_a_saved_one(tmp_path, capsys):
    """examples/run_frames.py --map --save-state, then a second run over the same sequence with --merge-into: the saved mapper is the
    base, the vocabulary is trained on the run's keyframes, and --save-state writes a mapper that loads"""
    from tests.test_gpu_dropin import _run_frames_module
    from vslam_amd.mapper import LocalMapper
    mod = _run_frames_module()
    base_file, merged_file = str(tmp_path / "base.npz"), str(tmp_path / "merged.npz")
    mod.main(["--max-frames", "14", "--keyframe-every", "4", "--map", str(tmp_path / "a.ply"), "--save-state", base_file])
    capsys.readouterr()
    mod.main(["--max-frames", "14", "--keyframe-every", "4", "--map", str(tmp_path / "b.ply"), "--vocabulary", str(tmp_path / "voc.npz"),
              "--merge-into", base_file, "--save-state", merged_file])
    out = capsys.readouterr().out
    line = next(ln for ln in out.splitlines() if ln.startswith("merged into " + base_file))
    print(line)
    ctx = _ctx()
    base, merged = LocalMapper.load_state(base_file, context=ctx), LocalMapper.load_state(merged_file, context=ctx)
    assert merged.vocabulary is not None and "state saved to " + merged_file in out
    if "aligned True" in line:
        assert len(merged.keyframes) > len(base.keyframes) and len(merged.map_points) > 0
    else:
        assert "taken out again" in line and len(merged.keyframes) == len(base.keyframes) and len(merged.map_points) == len(base.map_points)
    base.close(); merged.close(); ctx.close()
