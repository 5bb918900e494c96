"""Worlds of the local bundle adjustment over a keyframe set (LocalMapper.bundle_adjust(local="covisible" / free=...)) and of the
observation erase, as arrays.  No library, no GPU.

The revisit world is tests/ba_scene.Scene's construction with two more keyframes that come back to a place the camera left: keyframes
0 .. 9 move along x as in Scene (a point is seen by the keyframes win .. win + 2, win drawn from 0 .. 9), keyframes 10 and 11 stand
between keyframes 2 and 4 and see the points with win in {1, 2} and nothing else.  The keyframes sharing points with the last one are
therefore old ones: 1 .. 4 and 10, not the last six."""
import numpy as np

from tests.ba_scene import H_IMG, W_IMG, Scene, pose, project, rot

REVISIT_X = {10: 2.5, 11: 3.5}                       # centres of the two late keyframes, in units of the 0.35 baseline
REVISIT_W11 = [0, 135, 259, 263, 121, 0, 0, 0, 0, 0, 262, 264]
REVISIT_SET = [1, 2, 3, 4, 10, 11]                   # the covisible set of keyframe 11 at min_weight 15


class Revisit(Scene):
    """Scene's fields (see there); n_kf = 12"""

    def __init__(self, n_w=1500, n_rand=100, seed=21, pixel_noise=0.0):
        rng = np.random.default_rng(seed)
        n_kf = self.n_kf = 12
        X = np.column_stack([rng.uniform(-3.0, 5.5, n_w), rng.uniform(-2.0, 2.0, n_w), rng.uniform(3.0, 12.0, n_w)]).astype(np.float32)
        win = rng.integers(0, 10, n_w)
        self.poses = [pose(rot([0.0, rng.uniform(-0.03, 0.03), rng.uniform(-0.02, 0.02)]),
                           np.array([0.35 * REVISIT_X.get(k, k), 0.05 * np.sin(k), 0.0])) for k in range(n_kf)]
        obs = [dict() for _ in range(n_w)]
        self.kxy, self.octave = [], []
        for k, T in enumerate(self.poses):
            xy, z = project(T, X.astype(np.float64))
            seen = (win <= k) & (k <= win + 2) if k < 10 else (win == 1) | (win == 2)
            vis = np.flatnonzero(seen & (z > 0) & (xy[:, 0] > 5) & (xy[:, 0] < W_IMG - 5) & (xy[:, 1] > 5) & (xy[:, 1] < H_IMG - 5))
            n = len(vis) + n_rand
            perm = rng.permutation(n)
            kxy = np.zeros((n, 2), np.float32)
            kxy[perm[:len(vis)]] = xy[vis] + (rng.normal(0, pixel_noise, (len(vis), 2)) if pixel_noise else 0.0)
            kxy[perm[len(vis):]] = np.column_stack([rng.uniform(0, W_IMG, n_rand), rng.uniform(0, H_IMG, n_rand)])
            for j, r in zip(vis, perm[:len(vis)]):
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


def perturbed_set(s, positions, seed=3, angle=np.deg2rad(1.0), shift=0.03, depth=0.02):
    """Scene.perturbed with the keyframes of `positions` (and no others) turned and moved; every point moved along its ray"""
    rng = np.random.default_rng(seed)
    poses = [T.copy() for T in s.poses]
    for k in sorted(positions):
        d = rng.normal(size=3)
        c = rng.normal(size=3)
        P = np.eye(4)
        P[:3, :3] = rot(angle * d / np.linalg.norm(d))
        P[:3, 3] = shift * c / np.linalg.norm(c)
        poses[k] = P @ poses[k]
    X = s.X.astype(np.float64)
    X = X + rng.normal(0, depth / np.sqrt(3.0), X.shape) * np.linalg.norm(X, axis=1, keepdims=True)
    return poses, X.astype(np.float32)


def tiny_world(n_kf, n_pts, per_point, seed=5, rows=40):
    """a map of few points for the selection and erase tests: n_kf keyframes of `rows` keypoints at the identity pose, n_pts points each
    observed at `per_point` consecutive positions starting at a drawn one (wrapping), rows drawn.  Returns a Scene-like object."""
    rng = np.random.default_rng(seed)
    s = Scene.__new__(Scene)
    s.n_kf = n_kf
    s.poses = [pose(np.eye(3), np.array([0.01 * k, 0.0, 0.0])) for k in range(n_kf)]
    s.kxy = [np.column_stack([rng.uniform(0, W_IMG, rows), rng.uniform(0, H_IMG, rows)]).astype(np.float32) for _ in range(n_kf)]
    s.octave = [rng.integers(0, 4, rows).astype(np.int32) for _ in range(n_kf)]
    s.X = np.column_stack([rng.uniform(-1, 1, n_pts), rng.uniform(-1, 1, n_pts), rng.uniform(4, 8, n_pts)]).astype(np.float32)
    s.obs = []
    for j in range(n_pts):
        a = int(rng.integers(0, n_kf))
        s.obs.append({(a + d) % n_kf: int(rng.integers(0, rows)) for d in range(min(per_point, n_kf))})
    s.counts = np.array([rows] * n_kf, np.int32)
    off, okf, okp = [0], [], []
    for o in s.obs:
        okf += list(o.keys()); okp += list(o.values())
        off.append(len(okf))
    s.obs_off, s.obs_kf, s.obs_kp = np.array(off, np.int32), np.array(okf, np.int32), np.array(okp, np.int32)
    return s
