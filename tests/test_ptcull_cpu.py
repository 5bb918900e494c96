"""The map-point cull's restatement (tests/ptcull_restatement.py) and the constructed worlds (tests/ptcull_worlds.py), without a GPU:
every world decides what it was built to decide, the variant it is there to exclude decides differently, the erase leaves the map of the
survivors, the carry and merge rules do what the header says, and the new structs match the header."""
import os

import numpy as np
import pytest

from tests import ptcull_restatement as PR
from tests import ptcull_worlds as PW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(PW.CASES))
def test_world_decides_what_it_was_built_for(name):
    _, switch, want = PW.CASES[name]
    w = PW.case(name)
    r = PW.decide(w)
    assert len(w.counts) <= 6 and (w.counts <= 64).all() and (len(w.ids) <= 400 or name == "large")
    if want is not None:
        assert r["removed_indices"] == sorted(i for t in want for i in w.tagged(t))
    v = PW.decide(w, **{switch: False})
    assert v["removed_indices"] != r["removed_indices"], switch
    assert r["n_removed"] == len(r["removed_indices"]) and sum(r["n_reason"]) == len(w.ids)


def test_what_the_worlds_are_made_of():
    """the properties the cases' names promise"""
    w = PW.case("ratio_boundary")
    at, below, found = w.tagged("at"), w.tagged("below"), w.tagged("found")
    assert (w.life[at, :2] == [4, 1]).all() and (w.life[below, :2] == [5, 1]).all() and (w.life[found, :2] == [2, 2]).all()
    assert (w.life[:, 2] == 5).all() and w.now == 6
    r = PW.decide(w)
    assert (r["reason"][below] == 1).all() and not r["reason"][at].any()
    w = PW.case("age_window")
    r = PW.decide(w)
    for age in range(6):
        two, three = w.tagged("two@%d" % age), w.tagged("three@%d" % age)
        assert len(two) == len(three) == 15 and (w.now - w.life[two + three, 2] == age).all()
        n_obs = PR.observers(w.obs_off, w.obs_kf, w.obs_kp, w.counts)
        assert (n_obs[two] == 2).all() and (n_obs[three] == 3).all()
        assert (r["reason"][two] == (2 if age in (2, 3) else 0)).all() and not r["reason"][three].any()
    assert r["n_tested"] == 4 * 30 and len(w.ids) == 180   # (five doomed points left at the keyframes' own culls)
    w = PW.case("duplicate_position")
    d = w.tagged("dup")
    assert (np.diff(w.obs_off)[d] == 3).all() and (PR.observers(w.obs_off, w.obs_kf, w.obs_kp, w.counts)[d] == 2).all() and (w.obs_kf < 0).any()
    w = PW.case("invalid_entry")
    d = w.tagged("late")
    assert (np.diff(w.obs_off)[d] == 3).all() and (PR.observers(w.obs_off, w.obs_kf, w.obs_kp, w.counts)[d] == 2).all() and (w.obs_kf == 6).sum() >= 40
    w = PW.case("orphan")
    r = PW.decide(w)
    o4, o0 = w.tagged("orphan@4"), w.tagged("orphan@0")
    assert (r["reason"][o4 + o0] == 3).all() and (w.now - w.life[o4, 2] == 4).all() and (w.now - w.life[o0, 2] == 0).all() and len(w.counts) == 5
    w = PW.case("protect")
    r = PW.decide(w)
    prot = w.kw["protect"].astype(bool)
    assert (r["reason"][prot & (r["reason"] == 2)] == 2).sum() == 8 and not r["removed"][prot].any() and r["n_removed"] == 30 - 8
    assert r["n_reason"][2] == 30
    w = PW.case("max_age_off")
    assert PW.decide(w)["n_tested"] == len(w.ids)
    w = PW.case("large")
    assert len(w.ids) == 1500 > 1024 and len(w.obs_kf) == 3200 > 3 * 1024 and PW.decide(w)["removed_indices"] == list(range(0, 1500, 2))


@pytest.mark.parametrize("name", ["large", "age_window", "invalid_entry"])
def test_erase_leaves_the_map_of_the_survivors(name):
    w = PW.case(name)
    r = PW.decide(w)
    a = w.arrays()
    out, life, remap = PR.erase(a, w.life, r["removed"])
    keep = np.flatnonzero(~r["removed"])
    assert len(out["id"]) == len(keep) == len(life) and np.array_equal(out["id"], w.ids[keep]) and np.array_equal(life, w.life[keep])
    assert np.array_equal(remap[keep], np.arange(len(keep))) and (remap[r["removed"]] == -1).all()
    for new, old in enumerate(keep.tolist()):
        for f in ("obs_kf", "obs_kp"):
            assert np.array_equal(out[f][out["obs_off"][new]:out["obs_off"][new + 1]], a[f][a["obs_off"][old]:a["obs_off"][old + 1]])
    if name == "large":
        assert (out["obs_kf"] == 40).sum() == 200   # entries that name nothing travel with their points
    # nothing removed: nothing changes; what is left decides as before
    same, life2, remap2 = PR.erase(out, life, np.zeros(len(keep), bool))
    assert all(np.array_equal(same[f], out[f]) for f in out) and np.array_equal(remap2, np.arange(len(keep)))
    r2 = PR.decide(life, w.now, out["obs_off"], out["obs_kf"], out["obs_kp"], w.counts, **w.kw) if "protect" not in w.kw else None
    if r2 is not None:
        assert r2["n_removed"] == 0


def test_carry_and_merge_rules():
    life = np.array([[3, 2, 0], [5, 1, 1], [1, 1, 2], [2 ** 31 - 2, 7, 3], [9, 2 ** 31 - 1, 4]], np.int32)
    assert np.array_equal(PR.appended(life, 2, 6)[5:], [[1, 1, 6], [1, 1, 6]])
    assert np.array_equal(PR.compacted(life, [1, 0, 1, 0, 1])[:, 2], [0, 2, 4])
    # points 0 and 2 merge (2 has more observations and survives), 3 and 4 merge and saturate, 1 stays
    into = np.array([0, 1, 0, 2, 2])
    out = PR.merged(life, into, n_obs_valid=[2, 3, 4, 2, 2])
    assert out.tolist() == [[4, 3, 2], [5, 1, 1], [2 ** 31 - 1, 2 ** 31 - 1, 3]]
    assert PR.merged(life, into, survivors=[0, 1, 4])[:, 2].tolist() == [0, 1, 4]


def test_note_counts_a_point_once():
    w = PW.case("age_window")
    n = len(w.ids)
    life0 = PR.created(n, 6)
    pt = np.array([3, 3, 3, 5, -1, n, 7], np.int32)
    inl = np.array([0, 1, 0, 0, 1, 1, 1], bool)
    args = (w.xyz, w.obs_off, w.obs_kf, w.obs_kp, w.counts, PW.BASE_K, PW.POSE, 640, 480, pt, inl)
    life, cnt = PR.note(life0, *args, local_keyframes=[])
    assert cnt == dict(n_local=0, n_seen=0, n_matched=3, n_found=2)
    assert life[3].tolist() == [2, 2, 6] and life[5].tolist() == [2, 1, 6] and life[7].tolist() == [2, 2, 6] and (np.delete(life, [3, 5, 7], 0) == [1, 1, 6]).all()
    # with the whole map local every point is seen (they all stand in the image), matched or not: still once
    life, cnt = PR.note(life0, *args, window=0)
    assert cnt["n_local"] == cnt["n_seen"] == n and (life[:, 0] == 2).all() and life[:, 1].sum() == n + 2
    sat = life0.copy(); sat[:, 0] = 2 ** 31 - 1
    assert (PR.note(sat, *args, window=0)[0][:, 0] == 2 ** 31 - 1).all()


def test_new_structs_match_the_header(tmp_path):
    """the method of tests/test_cabi_cpu.py on the structs of the point-life calls"""
    import ctypes as C
    import subprocess
    import vslam_amd as V
    structs = [("mo_map_note_params", V.MapNoteParams), ("mo_map_note_out", V.MapNoteOut), ("mo_map_ptcull_params", V.MapPtCullParams),
               ("mo_map_ptcull_out", V.MapPtCullOut), ("mo_map_pterase_out", V.MapPtEraseOut)]
    body = ""
    for cname, cls in structs:
        body += '  printf("%%zu\\n", sizeof(%s));\n' % cname
        body += "".join('  printf("%%zu\\n", offsetof(%s, %s));\n' % (cname, f[0]) for f in cls._fields_)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vslam_amd.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    k = 0
    for cname, cls in structs:
        assert got[k] == C.sizeof(cls), cname
        offs = [getattr(cls, f[0]).offset for f in cls._fields_]
        assert got[k + 1:k + 1 + len(offs)] == offs, cname
        k += 1 + len(offs)


def test_abi_version_and_symbols():
    import vslam_amd as V
    lib = V.load_library()
    assert lib.mo_abi_version() == 7 == V.ABI_VERSION
    for name in ("mo_map_point_life", "mo_map_note_tracking", "mo_map_points_bad", "mo_map_erase_points", "mo_map_cull_points"):
        assert hasattr(lib, name) and name in V.SIGNATURES


def test_the_sequence_removes_the_wrong_points_only():
    """tests/ptcull_worlds.sequence() with the tracking restated (tests/view_restatement.track_frustum and the pose refinement): the true
    points stay at found >= 0.25 visible through the four keyframes, the wrong ones fall below it at the second and only they leave"""
    from tests import track_restatement as TR
    from tests import view_restatement as VR
    from tests import view_worlds as VW
    s = PW.sequence()
    w, wrong = s["w"], s["wrong"]
    a = w.arrays()
    n = len(w.obs)
    assert 150 <= n <= 400 and max(len(x) for x in w.kf_xy) <= 400
    kf_desc, kf_oct, kf_P = list(w.kf_desc), list(w.kf_oct), list(w.kf_P())
    life, ids = PR.created(n, VW.N_KF - 1), np.arange(n)
    arr = {"xyz": w.xyz.copy(), "id": ids.astype(np.int32), "obs_off": a["obs_off"], "obs_kf": a["obs_kf"], "obs_kp": a["obs_kp"]}
    removed_at = {}
    for j, (Tk, frames) in enumerate(s["steps"]):
        for T, kps, desc in frames:
            lv = VR.local_views(arr["xyz"], arr["obs_off"], arr["obs_kf"], arr["obs_kp"], kf_desc, kf_oct, kf_P, window=0)
            r = VR.track_frustum(VW.K, VW.perturbed(T), arr["xyz"], lv, kps, desc, VW.W_IMG, VW.H_IMG, refine_pose=True)
            ps = r["passes"][-1]
            q = np.flatnonzero(ps["point"] >= 0)
            pose, inl, n_inl = TR.refine(VW.K, ps["from"], arr["xyz"][ps["point"][q]].astype(np.float64),
                                         np.column_stack([kps["x"][q], kps["y"][q]]).astype(np.float64), kps["octave"][q])
            assert len(r["passes"]) == 2 and n_inl >= 30
            inlier = np.zeros(len(kps), bool)
            inlier[q] = inl
            life, cnt = PR.note(life, arr["xyz"], arr["obs_off"], arr["obs_kf"], arr["obs_kp"], [len(d) for d in kf_desc], VW.K, pose, VW.W_IMG,
                                VW.H_IMG, ps["point"], inlier, window=0, frustum=dict(kf_oct=kf_oct, kf_P=kf_P))
            assert not np.isin(arr["id"][ps["point"][q]], wrong).any()
        kp, d = PW.empty_keyframe(j)
        kf_desc.append(d); kf_oct.append(kp["octave"].astype(np.int32)); kf_P.append(TR.projection_matrix(VW.K, Tk))
        true = ~np.isin(arr["id"], wrong)
        assert (4 * life[true, 1] >= life[true, 0]).all(), (life[true, 1] / life[true, 0]).min()   # the true points stay at found >= 0.25 visible
        r = PR.decide(life, VW.N_KF + j, arr["obs_off"], arr["obs_kf"], arr["obs_kp"], [len(x) for x in kf_desc])
        removed_at[j] = arr["id"][r["removed"]].tolist()
        arr, life, _ = PR.erase(arr, life, r["removed"])
    assert removed_at == {0: [], 1: wrong, 2: [], 3: []} and len(arr["id"]) == n - PW.N_WRONG
