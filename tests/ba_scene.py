"""The constructed scene of the bundle-adjustment tests, as arrays: eight keyframes along x, points each seen from the keyframes a, a + 1,
a + 2 (where visible), exact f32 positions and f32 keypoints, rows shuffled among random extra rows.  No library, no GPU.
(The relocalization tests' world takes a, a + 2, a + 4: its even and odd keyframes share no point, two separate maps with one fixed
keyframe each, whose scales no bundle adjustment can tie together.  Consecutive keyframes make one connected map.)"""
import numpy as np

K = np.array([[500.0, 0, 320.0], [0, 500.0, 240.0], [0, 0, 1.0]])
W_IMG, H_IMG = 640, 480


def rot(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def pose(R, c):
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = -R @ c
    return T


def project(T, X):
    x = (K @ (T[:3, :3] @ X.T + T[:3, 3:4])).T
    return x[:, :2] / x[:, 2:3], x[:, 2]


class Scene:
    """truth: poses [n_kf] 4x4, X [n_w][3] f32; per keyframe kxy [rows][2] f32, octave [rows]; the map points (those with observations)
    in world order: xyz, obs_off / obs_kf / obs_kp (insertion order = keyframe order)"""

    def __init__(self, n_w=1500, n_kf=8, n_rand=100, seed=21, pixel_noise=0.0):
        rng = np.random.default_rng(seed)
        self.n_kf = n_kf
        X = np.column_stack([rng.uniform(-3.0, 5.5, n_w), rng.uniform(-2.0, 2.0, n_w), rng.uniform(3.0, 12.0, n_w)]).astype(np.float32)
        win = rng.integers(0, n_kf, n_w)
        self.poses = [pose(rot([0.0, rng.uniform(-0.03, 0.03), rng.uniform(-0.02, 0.02)]), np.array([0.35 * k, 0.05 * np.sin(k), 0.0]))
                      for k in range(n_kf)]
        obs = [dict() for _ in range(n_w)]
        self.kxy, self.octave = [], []
        for k, T in enumerate(self.poses):
            xy, z = project(T, X.astype(np.float64))
            vis = np.flatnonzero((win <= k) & (k <= win + 2) & (z > 0) & (xy[:, 0] > 5) & (xy[:, 0] < W_IMG - 5) & (xy[:, 1] > 5)
                                 & (xy[:, 1] < H_IMG - 5))
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

    def perturbed(self, seed=3, angle=np.deg2rad(1.0), shift=0.03, depth=0.02, first_free=2):
        """(poses [n_kf][4][4] with those from first_free on turned by about `angle` and moved by about `shift`, xyz f32 moved by about
        `depth` of the distance to the origin)"""
        rng = np.random.default_rng(seed)
        poses = [T.copy() for T in self.poses]
        for k in range(first_free, self.n_kf):
            d = rng.normal(size=3)
            c = rng.normal(size=3)
            P = np.eye(4)
            P[:3, :3] = rot(angle * d / np.linalg.norm(d))
            P[:3, 3] = shift * c / np.linalg.norm(c)
            poses[k] = P @ poses[k]
        X = self.X.astype(np.float64)
        X = X + rng.normal(0, depth / np.sqrt(3.0), X.shape) * np.linalg.norm(X, axis=1, keepdims=True)
        return poses, X.astype(np.float32)

    def move_edges(self, frac=0.05, lo=8.0, hi=15.0, seed=9):
        """moves the keypoint of `frac` of the observation entries by lo .. hi px up or down (in self.kxy); returns the mask over the
        observation entries.  The cameras move along x, so the epipolar lines are close to horizontal: a move along them is what a
        change of depth looks like and is partly absorbed by the point, a move across them is a wrong match in every reading.  Only tracks of three views are touched, one edge each: a two-view track has four residuals for
        three unknowns and cannot tell which of its two edges is the wrong one, nor can a three-view track with two wrong edges."""
        rng = np.random.default_rng(seed)
        n = len(self.obs_kf)
        three = np.flatnonzero(np.diff(self.obs_off) >= 3)
        pts = rng.choice(three, int(round(frac * n)), replace=False)
        moved = np.zeros(n, bool)
        for p in pts:
            moved[rng.integers(self.obs_off[p], self.obs_off[p + 1])] = True
        for o in np.flatnonzero(moved):
            r = rng.uniform(lo, hi) * rng.choice([-1.0, 1.0])
            self.kxy[self.obs_kf[o]][self.obs_kp[o]] += np.array([0.0, r], np.float32)
        return moved

    def restate(self, poses, xyz, **kw):
        from tests.ba_restatement import bundle_adjust
        return bundle_adjust(self.obs_off, self.obs_kf, self.obs_kp, self.counts, self.kxy, self.octave, xyz, K,
                             np.array([T[:3, :4] for T in poses]), **kw)

    def pose_error(self, poses, positions=None):
        """largest absolute difference of the [R | t] entries to the truth over the positions"""
        positions = range(self.n_kf) if positions is None else positions
        return max(float(np.abs(np.asarray(poses[k])[:3, :4] - self.poses[k][:3, :4]).max()) for k in positions)
