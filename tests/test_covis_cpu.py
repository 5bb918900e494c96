"""The covisibility restatement (tests/covis_restatement.py) against a brute-force set intersection, its tie rules on a hand-written
matrix, what the pan-back world (tests/covis_worlds.py) must show for tests/test_gpu_covis.py to mean anything, and the two new structs
of include/vslam_amd.h against their ctypes mirrors.  No GPU."""
import os

import numpy as np
import pytest

from tests import covis_restatement as CR
from tests import track_restatement as TR
from tests.covis_worlds import A_KF, pan_back
from tests.map_worlds import perturbed_pose, world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _brute(w):
    """W from the sets of points each position sees, read off the observation arrays key by key"""
    n = len(w.counts)
    sees = [set() for _ in range(n)]
    for i in range(len(w.obs_off) - 1):
        for o in range(int(w.obs_off[i]), int(w.obs_off[i + 1])):
            k, r = int(w.obs_kf[o]), int(w.obs_kp[o])
            k = k + n if k < 0 else k
            if not 0 <= k < n:
                continue
            r = r + int(w.counts[k]) if r < 0 else r
            if 0 <= r < w.counts[k]:
                sees[k].add(i)
    return np.array([[len(sees[p] & sees[q]) for q in range(n)] for p in range(n)], np.int32)


@pytest.mark.parametrize("name", ["clean", "stale", "ba", "ba_stale", "pan_back"])
def test_restatement_equals_set_intersection(name):
    w = pan_back() if name == "pan_back" else world(name)
    W = CR.covisibility(w.obs_off, w.obs_kf, w.obs_kp, w.counts)
    assert W.dtype == np.int32 and np.array_equal(W, _brute(w)) and np.array_equal(W, W.T)
    assert W.trace() > 0 and (W - np.diag(W.diagonal())).sum() > 0
    if name in ("stale", "ba_stale"):   # keys that name nothing were there to be skipped
        assert W.trace() < len(w.obs_kf)


def test_tie_rules_on_a_hand_written_matrix():
    W = np.array([[9, 5, 5, 0, 2],
                  [5, 9, 3, 3, 0],
                  [5, 3, 9, 5, 1],
                  [0, 3, 5, 9, 1],
                  [2, 0, 1, 1, 9]])
    # no votes: K1 = {ref}; row 0 holds 5, 5, 2: the later of the two fives first
    s = CR.local_keyframes(W, None, 0, n_best=1, min_weight=1)
    assert (s["k1"], s["k2"], s["ref"]) == ([0], [2], 0)
    s = CR.local_keyframes(W, None, 0, n_best=2, min_weight=1)
    assert (s["k1"], s["k2"]) == ([0], [1, 2])
    s = CR.local_keyframes(W, None, None, n_best=3, min_weight=1)   # ref None: the last keyframe; its row holds 2, 0, 1, 1
    assert (s["k1"], s["k2"], s["ref"]) == ([4], [0, 2, 3], 4)
    s = CR.local_keyframes(W, None, 4, n_best=2, min_weight=1)      # ... 2, then the later of the two ones
    assert s["k2"] == [0, 3]
    # votes: ref = the most votes, ties to the later position; a K1 keyframe that is also somebody's neighbour stays 1
    s = CR.local_keyframes(W, [0, 4, 0, 4, 1], None, n_best=1, min_weight=1)
    assert (s["k1"], s["ref"]) == ([1, 3, 4], 3) and s["k2"] == [0, 2] and s["mask"].tolist() == [2, 1, 2, 1, 1]
    # n_best = 0 and a floor above every weight: K1 alone; min_weight <= 0 still asks for one shared point
    assert CR.local_keyframes(W, [0, 4, 0, 4, 1], None, n_best=0, min_weight=1)["k2"] == []
    assert CR.local_keyframes(W, [0, 4, 0, 4, 1], None, n_best=4, min_weight=6)["k2"] == []
    assert CR.local_keyframes(W, None, 1, n_best=4, min_weight=0)["local"] == [0, 1, 2, 3]
    assert CR.local_keyframes(np.zeros((0, 0), np.int32))["ref"] == -1


def test_pan_back_world_tells_the_window_from_covisibility():
    w = pan_back()
    n_kf = len(w.counts)
    assert n_kf == 20 and len(w.obs) == 1500
    n_obs = np.array([len(p) for p in CR.positions(w.valid)])
    assert all((n_obs == c).sum() >= 20 for c in (1, 2, 3, 6)) and len(w.twice) >= 5
    assert all(len(w.valid[i]) == n_obs[i] + 1 for i in w.twice)   # seen twice in one keyframe: one position fewer than observations
    assert w.a_only.sum() >= 200 and all(k in A_KF for i in np.flatnonzero(w.a_only) for k, _ in w.valid[i])
    # the recency window of 10 holds no point of A ...
    local10 = TR.local_points(w.valid, n_kf, 10)
    assert local10.sum() > 500 and not (local10 & w.a_only).any()
    kps, desc = w.query()
    pose0 = perturbed_pose(w.query_pose)
    W_, H_ = w.image_size
    r10 = TR.track(w.K, pose0, w.xyz, w.obs_off, w.obs_kf, w.obs_kp, w.kf_desc, w.kf_oct, kps, desc, W_, H_, window=10)
    assert not r10["ok"] and r10["passes"][-1]["matches"] < 20
    # ... the covisible keyframes of what the frame before matched hold all of it
    seeds = w.seeds()
    assert (seeds < 0).sum() > 100 and not w.a_only[seeds[seeds >= 0]].any()
    res, sel = CR.track_covisible(w.K, pose0, w.xyz, w.obs_off, w.obs_kf, w.obs_kp, w.kf_desc, w.kf_oct, kps, desc, W_, H_, seed_points=seeds)
    assert all(k in sel["local"] for k in A_KF) and all(k in sel["k2"] for k in (0, 1, 2, 3)) and sel["ref"] >= 7
    W = CR.covisibility(w.obs_off, w.obs_kf, w.obs_kp, w.counts)
    assert min(W[4, 0], W[4, 2], W[5, 1], W[5, 3]) >= 2 * 15   # the links that bring A in, with margin over min_weight
    last = res["passes"][-1]
    assert res["ok"] and last["inliers"] >= 4 * 30 and int(w.a_only[last["point"][last["point"] >= 0]].sum()) >= 100
    assert np.abs(res["pose"] - w.query_pose).max() < 1e-6
    # a tighter selection is a proper subset: the world tells n_best and min_weight apart
    tight = CR.local_keyframes(W, CR.seed_votes(w.obs_off, w.obs_kf, w.obs_kp, w.counts, seeds), None, n_best=1, min_weight=100)
    assert set(tight["k2"]) < {0, 1, 2, 3} and tight["k2"] and len(tight["local"]) < n_kf


def test_new_structs_match_the_header(tmp_path):
    """the method of tests/test_cabi_cpu.py on mo_map_local_params / mo_map_local_out"""
    import ctypes as C
    import subprocess
    import vslam_amd as V
    structs = [("mo_map_local_params", V.MapLocalParams), ("mo_map_local_out", V.MapLocalOut)]
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
    for name in ("mo_map_covisibility", "mo_map_local_keyframes", "mo_map_track_covisible"):
        assert hasattr(lib, name) and name in V.SIGNATURES
