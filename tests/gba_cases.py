"""Constructed scenes for the tests of the global bundle adjustment (mo_map_global_ba), as arrays: a long trajectory along x.  The scene of
the local solver's tests (tests/ba_scene.py) cannot supply one, because its points stop at x = 5.5.  Cameras every 0.35 along x with
the small rotations and the intrinsics of ba_scene; per_kf * n_kf points uniform in x over the path +- 3, y in +- 2, depth 3 .. 12; the
track of a point starts 0 .. 5 keyframes after the point first becomes visible and lasts `span` keyframes (where visible); exact f32
positions and f32 keypoints, rows shuffled among random extra rows.  No library, no GPU.

The cases are the smallest that reach new ground:
  A  24 keyframes x 40: 22 free keyframes with two fixed, more than the local solver's 16
  B  200 keyframes x 20: 6 n_free > 1024, every loop over the solve's vectors strides
  C  4 keyframes x 1500: a keyframe with more edges than a workgroup has threads
  D  4 keyframes x 1700: 4594 edges per free keyframe, past the 4096 from which pass (b) of the solve runs 1024 threads per keyframe
     (C, at 4056, stays below)
The module asserts, as a condition of the scenes, that consecutive keyframes share at least 20 problem points: one connected map."""
import numpy as np

from tests.ba_scene import H_IMG, K, W_IMG, Scene, pose, project, rot

CASES = {"A": dict(n_kf=24, per_kf=40), "B": dict(n_kf=200, per_kf=20), "C": dict(n_kf=4, per_kf=1500), "D": dict(n_kf=4, per_kf=1700)}
MIN_SHARED = 20


class LongScene(Scene):
    """tests.ba_scene.Scene's fields (and its perturbed / move_edges / pose_error) over a long trajectory"""

    def __init__(self, n_kf=24, per_kf=40, span=4, n_rand=30, seed=21, pixel_noise=0.0):
        rng = np.random.default_rng(seed)
        self.n_kf = n_kf
        n_w = per_kf * n_kf
        length = 0.35 * (n_kf - 1)
        X = np.column_stack([rng.uniform(-3.0, length + 3.0, n_w), rng.uniform(-2.0, 2.0, n_w), rng.uniform(3.0, 12.0, n_w)]).astype(np.float32)
        self.poses = [pose(rot([0.0, rng.uniform(-0.03, 0.03), rng.uniform(-0.02, 0.02)]), np.array([0.35 * k, 0.05 * np.sin(k), 0.0]))
                      for k in range(n_kf)]
        vis, xys = np.zeros((n_kf, n_w), bool), []
        for k, T in enumerate(self.poses):
            xy, z = project(T, X.astype(np.float64))
            vis[k] = (z > 0) & (xy[:, 0] > 5) & (xy[:, 0] < W_IMG - 5) & (xy[:, 1] > 5) & (xy[:, 1] < H_IMG - 5)
            xys.append(xy)
        first = np.where(vis.any(axis=0), vis.argmax(axis=0), n_kf)
        start = first + rng.integers(0, 6, n_w)
        obs = [dict() for _ in range(n_w)]
        self.kxy, self.octave = [], []
        for k in range(n_kf):
            seen = np.flatnonzero(vis[k] & (start <= k) & (k < start + span))
            n = len(seen) + n_rand
            perm = rng.permutation(n)
            kxy = np.zeros((n, 2), np.float32)
            kxy[perm[:len(seen)]] = xys[k][seen] + (rng.normal(0, pixel_noise, (len(seen), 2)) if pixel_noise else 0.0)
            kxy[perm[len(seen):]] = np.column_stack([rng.uniform(0, W_IMG, n_rand), rng.uniform(0, H_IMG, n_rand)])
            for j, r in zip(seen, perm[:len(seen)]):
                obs[j][k] = int(r)
            self.kxy.append(kxy)
            self.octave.append(rng.integers(0, 4, n).astype(np.int32))
        keep = [j for j in range(n_w) if obs[j]]
        self.obs = [obs[j] for j in keep]
        self.X = X[keep]
        self.counts = np.array([len(k) for k in self.kxy], np.int32)
        off, okf, okp = [0], [], []
        for o in self.obs:
            okf += list(o.keys()); okp += list(o.values())
            off.append(len(okf))
        self.obs_off, self.obs_kf, self.obs_kp = np.array(off, np.int32), np.array(okf, np.int32), np.array(okp, np.int32)
        # the conditions of the scene
        self.problem = np.diff(self.obs_off) >= 2
        self.kf_edges = np.bincount(self.obs_kf[np.repeat(self.problem, np.diff(self.obs_off))], minlength=n_kf)
        shared = [sum(1 for o in self.obs if len(o) >= 2 and k in o and k + 1 in o) for k in range(n_kf - 1)]
        self.min_shared = min(shared)
        assert self.min_shared >= MIN_SHARED, shared

    def restate(self, poses, xyz, **kw):
        from tests.gba_restatement import global_bundle_adjust
        return global_bundle_adjust(self.obs_off, self.obs_kf, self.obs_kp, self.counts, self.kxy, self.octave, xyz, K,
                                    np.array([T[:3, :4] for T in poses]), **kw)


def case(name, **kw):
    return LongScene(**dict(CASES[name], **kw))


def scale_normalised_errors(s, poses, points, mask):
    """(pose error, point error) to the truth after the map is rescaled about the first camera centre so that the distance between the
    first and the last camera centre is the truth's: what a solution with the scale held only by the damping is compared by.  Position
    0 is fixed at its true pose, so the rescaling leaves it in place."""
    def centre(T):
        T = np.asarray(T)[:3, :4]
        return -T[:, :3].T @ T[:, 3]
    c0 = centre(s.poses[0])
    g = np.linalg.norm(centre(s.poses[-1]) - c0) / np.linalg.norm(centre(poses[-1]) - centre(poses[0]))
    e_pose = 0.0
    for k in range(s.n_kf):
        R = np.asarray(poses[k])[:3, :3]
        c = c0 + g * (centre(poses[k]) - c0)
        T = np.hstack([R, (-R @ c).reshape(3, 1)])
        e_pose = max(e_pose, float(np.abs(T - s.poses[k][:3, :4]).max()))
    Xs = c0 + g * (np.asarray(points, np.float64)[mask] - c0)
    return e_pose, float(np.abs(Xs - s.X[mask]).max())
