"""The restated chain of tests/rebuild_chain_world.py alone: the world has what tests/test_gpu_rebuild_chain.py is there for, so that the
device test cannot pass on an empty case."""
import numpy as np

from tests import rebuild_chain_world as RC
from tests.track_restatement import valid_observations


def test_the_chain_world_has_every_case():
    chain = RC.restated()
    assert [s for s, _ in chain] == ["start"] + list(RC.STEPS)
    st = dict(chain)
    a = st["start"]
    n = len(a["id"])
    assert 1024 < n < 1400 and len(a["counts"]) == RC.N_KF                      # more than a workgroup, more than one scan tile
    per = np.diff(a["obs_off"])
    assert per[0] == 0 and per[-1] == 0 and (per == 0).sum() >= RC.N_ZERO - 2   # points without observations, at both ends too
    valid = valid_observations(a["obs_off"], a["obs_kf"], a["obs_kp"], a["counts"])
    n_valid = sum(len(v) for v in valid)
    assert n_valid < len(a["obs_kf"]) and (a["obs_kf"] < 0).any() and (a["obs_kf"] >= RC.N_KF).any()   # stale and negative keys
    assert len(set(map(tuple, a["life"].tolist()))) >= 3 and len(set(map(tuple, a["color"].tolist()))) > n // 2
    # the add gives entries, but not one per given pair
    added = len(st["add_observations"]["obs_kf"]) - len(a["obs_kf"])
    assert 10 <= added < len(RC.world()["add"][1]) - 3
    # a mask that removes nothing: the identity
    assert np.array_equal(st["erase_map_points_none"]["remap"], np.arange(n))
    r = st["erase_map_points"]["remap"]
    assert r[0] == -1 and r[-1] == -1 and 100 < (r < 0).sum() < n // 2          # a point removed at each end
    k = st["erase_keyframes"]
    assert len(k["counts"]) == RC.N_KF - 1 and len(k["obs_kf"]) < len(st["erase_map_points"]["obs_kf"])   # a keyframe removed
    assert (k["obs_kf"] >= 0).all() and (k["obs_kf"] < RC.N_KF - 1).all() and (k["obs_kp"] >= 0).all()
    e = st["erase_observations"]["info"]
    assert st["erase_observations_none"]["info"]["n_erased"] == 0 and e["n_erased"] > 20 and e["n_under"] > 0
    f = st["fuse_map_points"]
    assert f["info"]["n_absorbed"] >= 50 and f["info"]["n_gained"] >= 0 and f["margin"] > 1e-9        # fused pairs, clear decisions
    assert (np.bincount(f["into"]) > 1).sum() >= 50
    assert (f["life"][:, 0] > a["life"][:, 0].max()).any()                                              # a merged record is a sum
    c = st["add_keyframe"]
    assert 50 <= len(c["id"]) < len(f["id"]) and (np.diff(c["obs_off"]) >= 2).all() and len(c["counts"]) == RC.N_KF
