"""A numpy restatement of the reference LocalMapper's bookkeeping (local_mapper.py), written from what it does: map growth from a
given set of inliers, the map-point cull, the per-keyframe lists, the keyframe cull and the PLY text.  No GPU.

The growth step's geometry (matching, F-RANSAC, triangulation) comes from outside: a caller feeds either the oracle's results or the
device's, so the bookkeeping can be compared exactly."""
from collections import defaultdict

import numpy as np


def projection(K, pose):
    t = np.asarray(pose[:3, 3]).reshape(3, 1)
    return K @ np.hstack((pose[:3, :3], t))


def reproj_err(P, pos, pt):
    """err in the order numpy's P @ [x, y, z, 1] rounds without FMA: ((P0 x + P1 y) + P2 z) + P3"""
    x, y, z = (float(v) for v in np.asarray(pos, np.float32))
    r = [((P[i, 0] * x + P[i, 1] * y) + P[i, 2] * z) + P[i, 3] for i in range(3)]
    du = r[0] / r[2] - float(pt[0])
    dv = r[1] / r[2] - float(pt[1])
    return float(np.sqrt(du * du + dv * dv))


class RefMapper:
    def __init__(self, K):
        self.K = np.asarray(K, np.float64)
        self.keyframes = []
        self.map_points = []
        self.co_visibility_graph = defaultdict(lambda: defaultdict(int))
        self.near = []   # (point id, err) of observations within 1e-9 of the threshold

    def add_keyframe(self, image, xy, pose, growth=None):
        """xy [n][2] f32 keypoint positions; growth = (queryIdx, trainIdx, positions f32 [m][3]) of the F inliers in query order"""
        kf = {"id": len(self.keyframes), "image": image, "xy": np.asarray(xy, np.float32), "pose": pose,
              "P": projection(self.K, pose), "map_points": []}
        self.keyframes.append(kf)
        if len(self.keyframes) > 1 and growth is not None:
            prev = self.keyframes[-2]
            q, t, X = growth
            img = prev["image"]
            for qi, ti, p in zip(q, t, X):
                x, y = int(prev["xy"][qi][0]), int(prev["xy"][qi][1])
                if img is not None and 0 <= x < img.shape[1] and 0 <= y < img.shape[0]:
                    col = img[y, x, :] if img.ndim == 3 else np.array([img[y, x]] * 3)
                else:
                    col = np.array([0, 0, 255])
                mp = {"id": len(self.map_points), "position": np.asarray(p, np.float32), "color": np.asarray(col),
                      "observed_keyframes": {prev["id"]: int(qi), kf["id"]: int(ti)}}
                self.map_points.append(mp)
                prev["map_points"].append(mp["id"])
                kf["map_points"].append(mp["id"])
                self.co_visibility_graph[prev["id"]][kf["id"]] += 1
                self.co_visibility_graph[kf["id"]][prev["id"]] += 1
        if len(self.keyframes) >= 2:
            if self.map_points:
                self.cull_map_points()
            if len(self.keyframes) > 3:
                self.cull_keyframes()

    def cull_map_points(self):
        keep = []
        for mp in self.map_points:
            obs = mp.get("observed_keyframes", {})
            if len(obs) < 2:
                continue
            ok = True
            for kf_id, kp_id in obs.items():
                kf = self.keyframes[kf_id]           # by position, as the reference (IndexError included)
                pt = kf["xy"][kp_id]
                err = reproj_err(kf["P"], mp["position"], pt)
                if abs(err - 5.0) < 1e-9:
                    self.near.append((mp["id"], err))
                if err > 5.0:
                    ok = False
                    break
            if ok:
                keep.append(mp)
        self.map_points = keep
        for kf in self.keyframes:
            kf["map_points"] = [mp["id"] for mp in self.map_points if kf["id"] in mp.get("observed_keyframes", {})]

    def keyframe_counts(self):
        out = []
        for kf in self.keyframes:
            red = 0
            for mp_id in kf["map_points"]:
                mp = next((p for p in self.map_points if p["id"] == mp_id), None)
                if mp is None:
                    continue
                if sum(1 for k in mp["observed_keyframes"] if k != kf["id"]) >= 3:
                    red += 1
            out.append((len(kf["map_points"]), red))
        return out

    def cull_keyframes(self):
        counts = self.keyframe_counts()
        remove = [i for i in range(1, len(self.keyframes) - 2) if counts[i][0] >= 20 and counts[i][1] / counts[i][0] > 0.9]
        for idx in sorted(remove, reverse=True):
            kf_id = self.keyframes[idx]["id"]
            for other in self.co_visibility_graph[kf_id]:
                if other != kf_id:
                    del self.co_visibility_graph[other][kf_id]
            del self.co_visibility_graph[kf_id]
            self.keyframes.pop(idx)
        for i, kf in enumerate(self.keyframes):
            kf["id"] = i
        return remove

    def ply_text(self):
        pts = [mp for mp in self.map_points if len(mp["observed_keyframes"]) >= 2]
        s = ("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\n"
             "property uchar green\nproperty uchar blue\nend_header\n" % len(pts))
        lines = []
        for mp in pts:
            x, y, z = np.asarray(mp["position"], np.float32)
            r, g, b = mp["color"]
            lines.append(f"{x} {y} {z} {int(r)} {int(g)} {int(b)}\n")
        return s + "".join(lines)


def cull_arrays(P_by_pos, xy_by_pos, xyz, off, okf, okp, min_obs=2):
    """vectorised cull of an array map: keep mask [n] and the error of every point's deciding observation, with the reference's
    position indexing (negative ids count from the end); raises IndexError where the reference would"""
    n_kf = len(P_by_pos)
    n = len(xyz)
    cnt = np.diff(off)
    keep = cnt >= min_obs
    alive = keep.copy()
    near = np.zeros(n, bool)
    X = xyz.astype(np.float64)
    for j in range(int(cnt.max()) if n else 0):
        idx = np.flatnonzero(alive & (cnt > j))
        if not len(idx):
            break
        e = off[idx] + j
        kf = okf[e].copy()
        kf[kf < 0] += n_kf
        if ((kf < 0) | (kf >= n_kf)).any():
            raise IndexError("list index out of range")
        P = np.stack(P_by_pos)[kf]
        pt = np.stack([xy_by_pos[k][p] for k, p in zip(kf, okp[e])]) if len(idx) < 1000 else None
        if pt is None:
            pt = np.empty((len(idx), 2), np.float32)
            for k in np.unique(kf):
                s = kf == k
                pt[s] = xy_by_pos[k][okp[e][s]]
        r = [((P[:, i, 0] * X[idx, 0] + P[:, i, 1] * X[idx, 1]) + P[:, i, 2] * X[idx, 2]) + P[:, i, 3] for i in range(3)]
        du = r[0] / r[2] - pt[:, 0].astype(np.float64)
        dv = r[1] / r[2] - pt[:, 1].astype(np.float64)
        err = np.sqrt(du * du + dv * dv)
        near[idx[np.abs(err - 5.0) < 1e-9]] = True
        bad = idx[err > 5.0]
        keep[bad] = False
        alive[bad] = False
    return keep, near
