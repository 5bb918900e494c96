"""The loop world of tests/loop_worlds.py as the loop correction reads it, for the end-to-end tests of
LocalMapper.detect_loop(sim3=True, confirm=True, correct=True): at the asking position the confirmation's restatement (the world's true
similarity, every match a seed: tests/confirm_worlds.py) gives loop_point, the covisibility counts give the default corrected set, and
tests/correct_restatement.py is run on them.  Plain numpy."""
import numpy as np

from tests import confirm_restatement as CFR
from tests import confirm_worlds as CW
from tests import correct_restatement as CR
from tests import loop_worlds as LW
from tests.track_restatement import valid_observations

ASK = 26
MIN_WEIGHT = 15
# The largest distance of a corrected pose or of a surviving moved duplicate from the unscaled world (w.X_world, the unscaled poses),
# measured on the restatement with the world's true similarity: 4.77e-7 on the world rescaled by 1.3 (one f32 rounding of a coordinate
# near 4), 6.9e-18 on the plain world (A is the identity to the last bits).  The points are f32, as for tests/sim3_cases.TRUTH_BOUND:
# the device, which corrects with the similarity it found itself, is held to ten times the measurement.
TRUTH_RESTATED = 4.8e-7
TRUTH_BOUND = 4.8e-6


def arrays_of(w):
    n = len(w.points)
    return {"xyz": np.array([np.asarray(q["position"], np.float64) for q in w.points], np.float32), "color": np.zeros((n, 3), np.uint8),
            "id": np.array([q["id"] for q in w.points], np.int32), "obs_off": w.obs_off, "obs_kf": w.obs_kf, "obs_kp": w.obs_kp,
            "dref_kf": np.zeros(n, np.int32), "dref_row": np.zeros(n, np.int32)}


def covisibility(w):
    counts = [len(d) for d in w.kf_desc]
    obs = valid_observations(w.obs_off, w.obs_kf, w.obs_kp, counts)
    W = np.zeros((len(counts), len(counts)), np.int64)
    for v in obs:
        pos = sorted({k for k, _ in v})
        for a in pos:
            for b in pos:
                W[a, b] += 1
    return W


def restated(w, factor=1.0):
    """dict: cand, group, corrected (position lists), loop_point, model and `res`: correct_restatement's result at position 26"""
    words, weights = LW.loop_vocabulary()
    lc = CW.candidates_at(w, ASK, words, weights)
    inp = CW.inputs_at(w, lc, 0, ASK, factor)
    fr = CFR.front(inp)
    m = fr["n_pairs"][0]
    bk = CFR.back(inp, fr, [np.ones(m, bool)], [m], inp.models)
    k = lc["cand"][0]
    group = sorted(set(lc["group"][0]) | {k})
    W = covisibility(w)
    corrected = sorted(({int(q) for q in np.flatnonzero(W[ASK] >= MIN_WEIGHT)} | {ASK}) - set(group))
    n_kf = len(w.kf_desc)
    cm, gm = np.zeros(n_kf, np.uint8), np.zeros(n_kf, np.uint8)
    cm[corrected] = 1; gm[group] = 1
    res = CR.correct(arrays_of(w), w.K, w.kf_poses, w.kf_xy, [np.zeros(len(a), np.int64) for a in w.kf_xy], w.kf_desc, ASK, k, inp.models[0], cm, gm,
                     bk["loop_point"], w.image_size[0], w.image_size[1])
    return {"cand": k, "group": group, "corrected": corrected, "loop_point": bk["loop_point"], "confirm_ok": bk["ok"], "model": inp.models[0], "res": res}


def facts(w, base, r):
    """what the end-to-end tests assert of a correction of world w (base: the unscaled world), from old-index arrays `into`, `moved`,
    the new xyz and ids, the corrected poses [n_kf][3][4] and loop_point: (absorbed duplicates named by loop_point, wrongly absorbed,
    old points moved, largest error of a corrected pose and of a surviving moved duplicate against the unscaled world)"""
    into, moved, xyz, ids, poses, lpt = r["into"], r["moved"], r["xyz"], r["ids"], r["poses"], r["loop_point"]
    old_ids = w.ids
    new_of_id = {int(i): j for j, i in enumerate(ids)}
    named, wrong = 0, []
    for L in sorted({int(x) for x in lpt if x >= 0}):
        j = int(old_ids[L])
        dup = np.flatnonzero(old_ids == LW.DUP_ID + j)
        if not len(dup):
            continue
        named += 1
        if not (j in new_of_id and LW.DUP_ID + j not in new_of_id and into[dup[0]] == into[L] == new_of_id[j]):
            wrong.append(j)
    e = 0.0
    for pos in LW.RETURN_POS:
        e = max(e, np.abs(poses[pos] - np.asarray(base.kf_poses[pos], np.float64)[:3, :4]).max())
    X_true = {int(q["id"]): np.asarray(q["position"], np.float64) for q in base.points}
    for i in np.flatnonzero(moved):
        if int(old_ids[i]) in new_of_id and ids[into[i]] == old_ids[i]:
            e = max(e, np.abs(xyz[into[i]].astype(np.float64) - X_true[int(old_ids[i])]).max())
    return named, wrong, int(moved[:w.n_old].sum()), e
