"""One small map and a chain of every call that rebuilds its store, each step restated in numpy by the restatement the repository already
has for it (tests/test_rebuild_chain_cpu.py, tests/test_gpu_rebuild_chain.py).  What the chain is there for: one rebuild must leave the
store and the device's live counts right for a different rebuild behind it.

The map: tests/fuse_worlds.split_world at four keyframes - every point with two observations stands twice, each half with one of them, so
that fuse_map_points has pairs to merge - plus points without any observation (the first and the last point of the map among them) and
keys decorated with stale and negative values.  About 1100 points: more than the 256 threads of a rebuild's workgroup and more than
one 1024-element tile of the device-wide scan.  Every point has its own colour; note_tracking gives the life records different counts.

The chain (STEPS), on one LocalMapper:
  add_observations            true observations of the other half's keypoint, given twice, out of range, and to a point that has one there
  erase_map_points (nothing)  the store is not flipped, remap is the identity
  erase_map_points            point 0, the last point and every seventh
  erase_keyframes             position 1 (not the last: add_keyframe sizes its host buffers by the last stored keyframe): the stale
                              entries go with it, points are left without an observation
  erase_observations (none)   the store is not flipped
  erase_observations          every eleventh entry
  fuse_map_points             the halves merge
  add_keyframe                a keyframe nothing matches: the cull chain removes the points under two observations
Plain numpy; build() and apply() import the library when called."""
import numpy as np

from tests import ba_local_restatement as BLR
from tests import ba_restatement as BR
from tests import fuse_restatement as FR
from tests import fuse_worlds as FW
from tests import kfcull_restatement as KR
from tests import map_restatement as MR
from tests import ptcull_restatement as PR
from tests.map_worlds import kps_array
from tests.track_restatement import valid_observations

N_KF, ERASED_KF, N_ZERO = 4, 1, 6
STEPS = ("add_observations", "erase_map_points_none", "erase_map_points", "erase_keyframes", "erase_observations_none", "erase_observations",
         "fuse_map_points", "add_keyframe")
_W = {}


def _P(K, T):
    """the projection matrix as the mapper stores it"""
    from orbslam2.utils import compute_projection_matrix
    T = np.asarray(T, np.float64)
    return np.ascontiguousarray(compute_projection_matrix(T[:3, :3], T[:3, 3], K), np.float64)


def world():
    """dict: w (the FuseWorld), dicts (the injected points), notes [(points, inliers)], add (kf_pos, point, row), new_kf (kps, desc, pose)"""
    if _W:
        return _W
    w, _, n_split = FW.split_world(n_w=850, n_kf=N_KF, seed=47)
    assert n_split > 100
    zero_at = np.array([0.0, 0.0, 6.0], np.float32)
    for _ in range(N_ZERO - 2):
        w.add_point(zero_at, {})
    # a point without observations at either end of the map
    w.obs.insert(0, {}); w.xyz.insert(0, zero_at); w.ids.insert(0, max(w.ids) + 1); w.origin.insert(0, -1)
    w.add_point(zero_at, {})
    w.finish()
    FW.decorate(w, seed=9, share=0.1)
    n = len(w.obs)
    rng = np.random.default_rng(5)
    col = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    dicts = [{"id": int(w.ids[i]), "position": np.asarray(w.xyz[i], np.float32), "color": col[i], "observed_keyframes": w.obs[i]} for i in range(n)]
    # the other half's observation for every fifth split pair (neighbours with the same id: i holds the first observation, i + 1 the rest)
    valid = valid_observations(w.obs_off, w.obs_kf, w.obs_kp, w.counts)
    pairs = [i for i in range(n - 1) if w.ids[i] == w.ids[i + 1] and len(valid[i]) == 1 and len(valid[i + 1]) == 1 and valid[i + 1][0][0] == 2]
    assert len(pairs) > 50
    pt, row = [], []
    for i in pairs[::5]:
        pt.append(i); row.append(valid[i + 1][0][1])
    have = next(i for i in range(n) if any(k == 2 for k, _ in valid[i]))
    pt = [-1, n, pt[0]] + pt + [pt[1], have]              # out of range twice; the first pair again in front: the lowest entry wins
    row = [7, 7, row[0]] + row + [row[1] + 1, 0]          # (the repeated one behind with another row, which loses; a point that has one at 2)
    notes = [(np.arange(0, n, 3, dtype=np.int32), (np.arange(0, n, 3) % 2 == 0)), (np.arange(1, n, 4, dtype=np.int32), np.ones(len(range(1, n, 4)), bool))]
    rng = np.random.default_rng(200)
    xy = np.column_stack([rng.uniform(0, w.image_size[0], 120), rng.uniform(0, w.image_size[1], 120)]).astype(np.float32)
    new_desc = np.repeat(rng.integers(0, 256, (60, 32)).astype(np.uint8), 2, axis=0)   # every descriptor twice: no match passes the ratio test
    new_pose = np.asarray(w.kf_poses[N_KF - 1], np.float64).copy()
    new_pose[0, 3] += 0.05
    _W.update(w=w, dicts=dicts, color=col, notes=notes, add=(2, np.array(pt, np.int32), np.array(row, np.int32)), new_kf=(xy, new_desc, new_pose))
    return _W


def remove_mask(n):
    m = np.zeros(n, bool)
    m[0] = m[n - 1] = True
    m[3::7] = True
    return m


def entry_mask(n_obs):
    m = np.zeros(n_obs, bool)
    m[5::11] = True
    return m


def restated():
    """[(step, state)] with the start as step "start": state = dict of the map arrays (FR.FIELDS), life [n][3], counts (rows per
    position), and what the step returns (remap, into, info)"""
    W = world()
    w = W["w"]
    n = len(w.obs)
    a = FR.as_arrays(w.xyz_arr, [list(o.items()) for o in w.obs], ids=w.ids, color=W["color"])
    a["dref_kf"] = -(np.arange(n, dtype=np.int32) + 1)   # the mapper's reference to the injected dict
    counts = np.asarray(w.counts, np.int32)
    life = PR.created(n, N_KF - 1)
    for point, inlier in W["notes"]:
        life, _ = PR.note(life, a["xyz"], a["obs_off"], a["obs_kf"], a["obs_kp"], counts, w.K, np.eye(4), *w.image_size, point, inlier, local_keyframes=[])
    P = [_P(w.K, T) for T in w.kf_poses]
    xy, octv, desc = list(w.kf_xy), list(w.kf_oct), list(w.kf_desc)
    out = [("start", dict(a, life=life, counts=counts))]

    def push(step, a, life, counts, **extra):
        out.append((step, dict({f: np.asarray(a[f]) for f in FR.FIELDS}, life=np.asarray(life, np.int32), counts=np.asarray(counts, np.int32), **extra)))
    # 1
    kf_pos, pt, row = W["add"]
    off, okf, okp = BR.add_observations(a["obs_off"], a["obs_kf"], a["obs_kp"], counts, kf_pos, pt, row)
    a = dict(a, obs_off=off, obs_kf=okf, obs_kp=okp)
    life = PR.carried(life)
    push(STEPS[0], a, life, counts)
    # 2, 3
    n = len(a["id"])
    a2, life2, remap = PR.erase(a, life, np.zeros(n, bool))
    assert all(np.array_equal(a2[f], a[f]) for f in a2)
    push(STEPS[1], a, life, counts, remap=remap)
    a, life, remap = PR.erase(a, life, remove_mask(n))
    push(STEPS[2], a, life, counts, remap=remap)
    # 4
    off, okf, okp, counts = KR.erase(a["obs_off"], a["obs_kf"], a["obs_kp"], counts, [ERASED_KF])
    a = dict(a, obs_off=off, obs_kf=okf, obs_kp=okp)
    life = PR.carried(life)
    for lst in (P, xy, octv, desc):
        lst.pop(ERASED_KF)
    push(STEPS[3], a, life, counts)
    # 5, 6
    no = len(a["obs_kf"])
    off, okf, okp, n_erased, n_under = BLR.erase_entries(a["obs_off"], a["obs_kf"], a["obs_kp"], np.zeros(no, bool))
    assert n_erased == 0 and np.array_equal(off, a["obs_off"])
    push(STEPS[4], a, life, counts, info={"n_erased": 0, "n_under": 0, "n_obs": no})
    off, okf, okp, n_erased, n_under = BLR.erase_entries(a["obs_off"], a["obs_kf"], a["obs_kp"], entry_mask(no))
    a = dict(a, obs_off=off.astype(np.int32), obs_kf=okf.astype(np.int32), obs_kp=okp.astype(np.int32))
    push(STEPS[5], a, life, counts, info={"n_erased": n_erased, "n_under": n_under, "n_obs": len(okf)})
    # 7
    n_valid = [len(v) for v in valid_observations(a["obs_off"], a["obs_kf"], a["obs_kp"], counts)]
    fused, into, cnt, margins = FR.fuse(a, P, xy, octv, desc, w.image_size[0], w.image_size[1])
    life = PR.merged(life, into, n_obs_valid=n_valid)
    a = fused
    push(STEPS[6], a, life, counts, into=into, info=cnt, margin=margins["min"])
    # 8
    nxy, ndesc, npose = W["new_kf"]
    P.append(_P(w.K, npose)); xy.append(nxy)
    counts = np.append(counts, len(nxy)).astype(np.int32)
    keep, near = MR.cull_arrays(P, xy, a["xyz"], a["obs_off"], a["obs_kf"], a["obs_kp"])
    assert not near.any()
    a, life, remap = PR.erase(a, life, ~keep)
    push(STEPS[7], a, life, counts, remap=remap)
    return out


def build(ctx):
    """the start of the chain on a device map"""
    from vslam_amd.mapper import LocalMapper
    W = world()
    w = W["w"]
    m = LocalMapper(w.K, save_every_keyframe=False, context=ctx)
    img = np.zeros((w.image_size[1], w.image_size[0]), np.uint8)
    for k in range(N_KF):
        m.add_keyframe(img, kps_array(w.kf_xy[k], w.kf_oct[k]), w.kf_desc[k], w.kf_poses[k])
        assert m.last["n_new"] == 0 and len(m.map_points) == 0
    m.update_map_points(W["dicts"])
    for point, inlier in W["notes"]:
        m.note_tracking(np.eye(4), {"point": point, "inlier": inlier}, local_keyframes=[])
    return m


def apply(m, step, state):
    """one step of the chain on the mapper; state: the restated state in front of it.  Returns what the call returned."""
    W = world()
    n, no = len(state["id"]), len(state["obs_kf"])
    if step == "add_observations":
        return m.add_observations(*W["add"])
    if step == "erase_map_points_none":
        return m.erase_map_points(np.zeros(n, bool))
    if step == "erase_map_points":
        return m.erase_map_points(remove_mask(n))
    if step == "erase_keyframes":
        return m.erase_keyframes([ERASED_KF])
    if step == "erase_observations_none":
        return m.erase_observations(np.zeros(no, bool))
    if step == "erase_observations":
        return m.erase_observations(entry_mask(no))
    if step == "fuse_map_points":
        return m.fuse_map_points(image_size=W["w"].image_size)
    assert step == "add_keyframe"
    xy, desc, pose = W["new_kf"]
    img = np.zeros((W["w"].image_size[1], W["w"].image_size[0]), np.uint8)
    m.add_keyframe(img, kps_array(xy), desc, pose)
    assert m.last["n_new"] == 0
    return None
