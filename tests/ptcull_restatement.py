"""numpy restatement of the life of a map point (mo_map_point_life, mo_map_note_tracking, mo_map_points_bad, mo_map_erase_points,
mo_map_cull_points in include/vslam_amd.h), operation for operation: the record {visible, found, born} and how every rebuild of the
store carries or merges it, note() for one tracked frame, decide() for ORB-SLAM2's MapPointCulling and erase() for the removal.
decide() takes switches, each the rule a kernel could get wrong; tests/test_ptcull_cpu.py shows that every constructed world of
tests/ptcull_worlds.py decides differently under the switch it is there for.  life is an int32 array [n][3]: visible, found, born."""
import numpy as np

from tests import view_restatement as VR
from tests.track_restatement import local_points, project, valid_observations

INT32_MAX = 2 ** 31 - 1
FIELDS = ("xyz", "color", "id", "dref_kf", "dref_row")


# ---- the record through the rebuilds ---------------------------------------------------------------------------------------------------
def created(n, now):
    """n new points made while the keyframe of ordinal `now` is the last stored one"""
    return np.tile(np.array([1, 1, now], np.int32), (n, 1))


def appended(life, n, now):
    """a creating call (the growth step of add_keyframe, create_new_map_points, update_map_points): the new records behind the old"""
    return np.vstack([np.asarray(life, np.int32).reshape(-1, 3), created(n, now)])


def compacted(life, keep):
    """a rebuild that keeps the points of the mask `keep` in their order (add_keyframe's cull, erase_map_points)"""
    return np.asarray(life, np.int32)[np.asarray(keep, bool)]


def carried(life):
    """a rebuild that keeps every point where it is (add_observations, erase_keyframes, capacity growth)"""
    return np.asarray(life, np.int32).copy()


def merged(life, into, n_obs_valid=None, survivors=None):
    """fuse_map_points / correct_loop: into[i] = the new index of the point old point i now is.  The survivor of a component (`survivors`
    [new index] -> old index; by default the member with the most valid observations - n_obs_valid - then the lowest index, the calls'
    rule) keeps its born; visible and found are the members' sums, formed beyond int32 and clamped"""
    life = np.asarray(life, np.int64)
    into = np.asarray(into, np.int64)
    n_new = int(into.max()) + 1 if len(into) else 0
    out = np.zeros((n_new, 3), np.int64)
    np.add.at(out[:, 0], into, life[:, 0])
    np.add.at(out[:, 1], into, life[:, 1])
    if survivors is None:
        survivors = np.full(n_new, -1, np.int64)
        best = {}
        for i, r in enumerate(into.tolist()):
            key = (-int(n_obs_valid[i]), i)
            if r not in best or key < best[r]:
                best[r] = key
                survivors[r] = i
    out[:, 2] = life[np.asarray(survivors, np.int64), 2]
    return np.minimum(out, INT32_MAX).astype(np.int32)


# ---- one tracked frame -----------------------------------------------------------------------------------------------------------------
def note(life, xyz, obs_off, obs_kf, obs_kp, counts, K, pose, w, h, point, inlier, window=10, local_keyframes=None, frustum=None):
    """(life after the call, counts).  frustum: None, or a dict of kf_oct and kf_P (by position) and optionally scale_factor, n_levels,
    view_range, min_cos: the frustum test of tests/view_restatement.py on views computed as a frustum call computes them"""
    life = np.asarray(life, np.int32).copy()
    n = len(life)
    cnt = dict(n_local=0, n_seen=0, n_matched=0, n_found=0)
    if n == 0 or len(counts) == 0:
        return life, cnt
    obs = valid_observations(obs_off, obs_kf, obs_kp, counts)
    if local_keyframes is None:
        local = local_points(obs, len(counts), window)
    else:
        pos = set(int(k) for k in local_keyframes)
        local = np.array([any(k in pos for k, _ in v) for v in obs], bool)
    u, v, z = project(K, pose, xyz)
    with np.errstate(invalid="ignore"):
        seen = local & (z > 0) & (u >= 0) & (u < w) & (v >= 0) & (v < h)
    if frustum is not None:
        sf, nl = frustum.get("scale_factor", 1.2), frustum.get("n_levels", 8)
        lo, hi = frustum.get("view_range", (0.8, 1.2))
        views = VR.point_views(xyz, obs, frustum["kf_oct"], VR.centres(frustum["kf_P"]), sf, nl, only=local)
        C = VR.camera_centre(pose)
        X = np.asarray(xyz, np.float32).astype(np.float64)
        for i in np.flatnonzero(seen).tolist():
            seen[i] = VR.frustum(X[i], views["normal"][i], views["max_dist"][i], C, sf, nl, lo, hi, frustum.get("min_cos", 0.5))[0]
    matched = np.zeros(n, bool)
    hit = np.zeros(n, bool)
    for p, ok in zip(np.asarray(point).reshape(-1).tolist(), np.asarray(inlier).reshape(-1).tolist()):
        if 0 <= p < n:
            matched[p] = True
            hit[p] |= bool(ok)
    vis = life[:, 0].astype(np.int64) + (seen | matched)
    fnd = life[:, 1].astype(np.int64) + hit
    life[:, 0] = np.minimum(vis, INT32_MAX)
    life[:, 1] = np.minimum(fnd, INT32_MAX)
    cnt.update(n_local=int(local.sum()), n_seen=int(seen.sum()), n_matched=int(matched.sum()), n_found=int(hit.sum()))
    return life, cnt


# ---- the decision ----------------------------------------------------------------------------------------------------------------------
def observers(obs_off, obs_kf, obs_kp, counts, once_per_position=True, skip_invalid=True):
    """per point: the positions at which it has a valid observation, each once.  once_per_position=False counts every valid entry,
    skip_invalid=False every entry: wrong on purpose"""
    if not skip_invalid:
        return np.diff(np.asarray(obs_off, np.int64))
    obs = valid_observations(obs_off, obs_kf, obs_kp, counts)
    return np.array([len(set(k for k, _ in v)) if once_per_position else len(v) for v in obs], np.int64)


def decide(life, now, obs_off, obs_kf, obs_kp, counts, ratio=0.25, min_age=2, max_age=3, max_obs=2, orphan_obs=1, protect=None,
           once_per_position=True, skip_invalid=True, strict_ratio=True, age_window=True, reason_2_needs_age=True, orphans=True,
           honour_protect=True, negative_max_age_tests_all=True):
    """dict of reason [n] u8, removed [n] bool, n_tested, n_removed, n_reason [4], removed_indices.  The switches after `protect` are the
    rules a kernel could get wrong, each True as the header states it."""
    life = np.asarray(life, np.int64).reshape(-1, 3)
    n = len(life)
    n_obs = observers(obs_off, obs_kf, obs_kp, counts, once_per_position, skip_invalid) if n else np.zeros(0, np.int64)
    reason = np.zeros(n, np.uint8)
    removed = np.zeros(n, bool)
    n_tested = 0
    for i in range(n):
        visible, found, born = (int(x) for x in life[i])
        age = int(now) - born
        tested = (max_age < 0 and negative_max_age_tests_all) or age <= max_age or not age_window
        n_tested += tested
        prod = np.float64(ratio) * np.float64(visible)
        low = np.float64(found) < prod if strict_ratio else np.float64(found) <= prod
        if tested and low:
            reason[i] = 1
        elif tested and (age >= min_age or not reason_2_needs_age) and n_obs[i] <= max_obs:
            reason[i] = 2
        elif orphans and n_obs[i] <= orphan_obs:
            reason[i] = 3
        removed[i] = reason[i] != 0 and not (honour_protect and protect is not None and protect[i])
    return {"reason": reason, "removed": removed, "n_tested": int(n_tested), "n_removed": int(removed.sum()),
            "n_reason": [int((reason == k).sum()) for k in range(4)], "removed_indices": np.flatnonzero(removed).tolist(), "now": int(now)}


# ---- the erase -------------------------------------------------------------------------------------------------------------------------
def erase(a, life, remove):
    """(arrays, life, remap) of the map without the points of the mask `remove`: the survivors in their order, every field and every
    observation entry as stored"""
    remove = np.asarray(remove, bool)
    keep = ~remove
    n = len(remove)
    off = np.asarray(a["obs_off"], np.int64)
    out = {f: np.asarray(a[f])[keep] for f in FIELDS if f in a}
    ent = np.concatenate([np.arange(off[i], off[i + 1]) for i in np.flatnonzero(keep)] + [np.zeros(0, np.int64)]).astype(np.int64)
    out["obs_kf"] = np.asarray(a["obs_kf"], np.int32)[ent]
    out["obs_kp"] = np.asarray(a["obs_kp"], np.int32)[ent]
    out["obs_off"] = np.concatenate([[0], np.cumsum(np.diff(off)[keep])]).astype(np.int32)
    remap = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    assert len(remap) == n
    return out, compacted(life, keep), remap
