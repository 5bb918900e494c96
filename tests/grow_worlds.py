"""Constructed maps for the tests of LocalMapper.create_new_map_points (tests/test_grow_cpu.py, tests/test_gpu_grow.py), on the worlds of
tests/map_worlds.py and tests/fuse_worlds.py.  Plain numpy; build_map / hand_map make the device maps.

withheld_points_world: a skip world in which every map point observed at the last keyframe position is taken out of the map while its
keypoints stay in the keyframes: what the call should give back.
Hand maps: camera f = 100, centre (50, 50), image 100 x 100; keyframe k looks down z from x = k (poses()), so a point (a, b, 10) lands
at (50 + 10 a - 10 k, 50 + 10 b): the epipolar lines are the image rows, the epipoles lie at infinity, two neighbouring keyframes see a
point at depth 10 under 5.7 degrees."""
import numpy as np

from tests import fuse_worlds as FW
from tests import grow_restatement as GR
from tests.track_restatement import valid_observations

K = np.array([[100.0, 0, 50.0], [0, 100.0, 50.0], [0, 0, 1.0]])
SIZE = (100, 100)


def withheld_points_world(n_w=500, n_kf=10, removed=(), seed=41, decorated=False):
    """(world, held): held = [(xyz f32, {position: row})] of the map points taken out, their valid observations by position"""
    w = FW.FuseWorld(FW.skip_world(n_w=n_w, n_kf=n_kf, removed=removed, seed=seed))
    last = len(w.survivors) - 1
    gone = [i for i, o in enumerate(w.obs) if last in o]
    held = [(np.asarray(w.xyz[i], np.float32), dict(w.obs[i])) for i in gone]
    keep = [i for i in range(len(w.obs)) if last not in w.obs[i]]
    w.obs = [w.obs[i] for i in keep]; w.xyz = [w.xyz[i] for i in keep]; w.ids = [w.ids[i] for i in keep]; w.origin = [w.origin[i] for i in keep]
    w.finish()
    if decorated:
        FW.decorate(w)
    return w, held


def restate_world(w, lists=None, **kw):
    """GR.grow of the map build_map makes of a world, without a device.  lists = (xy, octave, descriptors, poses) per position in place
    of the world's own (what a reader without the position -> slot table would see)"""
    a = FW.world_inputs(w)[0]
    xy, octv, desc, poses = lists if lists is not None else (w.kf_xy, w.kf_oct, w.kf_desc, w.kf_poses)
    kw.setdefault("target_slot", w.survivors[-1])
    return GR.grow(a, w.K, poses, xy, octv, desc, **kw)


def restate(m, lists=None, **kw):
    """GR.grow of the device map as it stands"""
    a, _, xy, octv, desc = FW.map_inputs(m)
    poses = [np.asarray(kf["pose"], np.float64) for kf in m.keyframes]
    if lists is not None:
        xy, octv, desc, poses = lists
    if m.keyframes:
        kw.setdefault("target_slot", next(s for s, r in enumerate(m._records) if r is m.keyframes[-1]))
        kw.setdefault("image", m.keyframes[-1]["image"])
    return GR.grow(a, np.asarray(m.camera_matrix, np.float64), poses, xy, octv, desc, **kw)


def recovered(held, a, point, counts, lo=0):
    """per held point with >= 2 observations at positions >= lo: (index of the new point at its target row or -1, observation set wanted)"""
    obs = valid_observations(a["obs_off"], a["obs_kf"], a["obs_kp"], counts)
    T = len(counts) - 1
    out = []
    for xyz, o in held:
        want = {(k, r) for k, r in o.items() if k >= lo}
        if len(want) < 2:
            continue
        i = int(point[o[T]])
        out.append((i, want, set(obs[i]) if i >= 0 else set(), xyz))
    return out


# ---- hand maps ------------------------------------------------------------------------------------------------------------------------
def poses(xs=(0.0, 1.0, 2.0)):
    out = []
    for x in xs:
        T = np.eye(4)
        T[0, 3] = -float(x)
        out.append(T)
    return out


_CODE = (0x00, 0x0F, 0x33, 0x55, 0x3C, 0x5A, 0x66, 0x69, 0xFF, 0xF0, 0xCC, 0xAA, 0xC3, 0xA5, 0x99, 0x96)


def desc(code, flips=()):
    """32 bytes of one word of the first-order Reed-Muller code of length 8 (any two words 128 or 256 bits apart), the given bits flipped"""
    d = np.full(32, _CODE[code], np.uint8)
    for b in flips:
        d[b // 8] ^= np.uint8(1 << (b % 8))
    return d


def px(a, b, k, z=10.0, xs=(0.0, 1.0, 2.0, 3.0)):
    """where keyframe k sees the point (a, b, z)"""
    return (50.0 + 100.0 * (a - xs[k]) / z, 50.0 + 100.0 * b / z)


def run(kfs, obs=(), xyz=(), T=None, **kw):
    """GR.grow of a hand map: kfs per keyframe [(x, y, descriptor[, octave])], obs per existing point [(key, row)]"""
    kf_xy = [np.array([[p[0], p[1]] for p in kf], np.float32).reshape(-1, 2) for kf in kfs]
    kf_desc = [np.array([p[2] for p in kf], np.uint8).reshape(-1, 32) for kf in kfs]
    kf_oct = [np.array([p[3] if len(p) > 3 else 0 for p in kf], np.int32) for kf in kfs]
    a = FW.FR.as_arrays(np.asarray(xyz, np.float32).reshape(-1, 3), [list(o) for o in obs], ids=np.arange(len(obs)) + 100)
    kw.setdefault("window", 0)
    return GR.grow(a, K, poses() if T is None else T, kf_xy, kf_oct, kf_desc, **kw)


def cases():
    """the hand-made gate cases shared by the CPU and the GPU tests: name -> (kfs, obs, xyz, poses, keyword arguments, expectations).
    expectations: counts that must hold (a subset of GR.COUNTS), `point` = per target row whether it made a point, `lists` = the
    observation lists of the new points.  Every pixel value is derived in the comment next to it."""
    c = {}
    two = poses((0.0, 1.0))
    D = [desc(j) for j in range(16)]
    # epipolar distance, octave 0: sqrt(3.84) = 1.9596 px.  Rows of the neighbour 1.95 and 1.97 px off the target rows' lines (y = 30, 60)
    c["epi_octave0"] = ([[(60, 31.95, D[0]), (60, 61.97, D[1])], [(50, 30, D[0]), (50, 60, D[1])]], [], [], two, {},
                        dict(n_free=2, n_epi=1, n_accepted=1, n_matches=1, n_new=1, point=[True, False], lists=[[(0, 0), (1, 0)]]))
    # ... at octave 2 of the neighbour row: 1.9596 * 1.2^2 = 2.8218 px: 2.81 inside, 2.83 outside (1.97 is now inside as well)
    c["epi_octave2"] = ([[(60, 32.81, D[0], 2), (60, 62.83, D[1], 2)], [(50, 30, D[0], 2), (50, 60, D[1], 2)]], [], [], two, {},
                        dict(n_epi=1, n_new=1, point=[True, False]))
    # epipole zone: the target one unit ahead and 0.1 to the right of the neighbour: the epipole in the neighbour is (60, 50), the
    # radius at octave 0 10 px, at octave 2 sqrt(100 * 1.44) = 12 px.  The points (1.99, 0, 10), (2.01, 0, 10) land 9.9 and 10.1 px from
    # it and in the target at 50 + 100 * 1.89 / 9 = 71.0, 50 + 100 * 1.91 / 9 = 71.2222; (2.19, 2.21) at octave 2 land 11.9 and 12.1 px off
    ahead = poses((0.0, 0.0))
    ahead[1][0, 3], ahead[1][2, 3] = -0.1, -1.0
    zone = [[(69.9, 50, D[0]), (70.1, 50, D[1]), (71.9, 50, D[2], 2), (72.1, 50, D[3], 2)],
            [(50 + 189 / 9.0, 50, D[0]), (50 + 191 / 9.0, 50, D[1]), (50 + 209 / 9.0, 50, D[2]), (50 + 211 / 9.0, 50, D[3])]]
    # (every row lies on every line here - they all pass through the epipole along y = 50 -: 4 target rows x the 2 rows outside the zone)
    c["epipole_zone"] = (zone, [], [], ahead, {}, dict(n_free=4, n_epi=8, n_accepted=2))
    # max_dist: 50 bits off is accepted, 51 is not
    c["max_dist"] = ([[(60, 30, desc(0, range(50))), (60, 60, desc(1, range(51)))], [(50, 30, D[0]), (50, 60, D[1])]], [], [], two, {},
                     dict(n_epi=2, n_accepted=1, n_new=1, point=[True, False]))
    # parallax: cos_max 0.9998 is 1.146 degrees.  A baseline of 0.21 at depth 10 is 1.203 degrees (cos 0.99978), 0.19 is 1.089 (0.99982):
    # the second match is won and not usable; a baseline of 0.001 likewise
    for name, base, made in (("cos_inside", 0.21, True), ("cos_outside", 0.19, False), ("no_baseline", 0.001, False)):
        c[name] = ([[(50 + 10 * base, 50, D[0])], [(50, 50, D[0])]], [], [], poses((0.0, base)), {},
                   dict(n_epi=1, n_accepted=1, n_matches=1, n_new=int(made), point=[made]))
    # negative depth: the neighbour on the left must see the point further right; 10 px further left the rays meet behind the cameras
    c["negative_depth"] = ([[(40, 50, D[0])], [(50, 50, D[0])]], [], [], two, {}, dict(n_matches=1, n_new=0, point=[False]))
    # reprojection in the base pair: the neighbour row at octave 6 passes the epipolar gate up to 1.9596 * 1.2^6 = 5.85 px.  A row d px off
    # the line: the least-squares point lies half way between the two rows in y (d / 2 px from each) and gives way in depth,
    # Z = 0.1 / (0.01 + (d / 100)^2), which moves it d^2 / 20 px along the line in both views: the target (octave 0) sees
    # d^2 / 4 + d^4 / 400 against 5.991, that is d = 4.469: 4.45 gives 5.93, 4.49 gives 6.06.  ratio_factor 10 keeps the scale gate out
    # of the way (octaves 0 and 6)
    c["reprojection_base"] = ([[(60, 34.45, D[0], 6), (60, 64.49, D[1], 6)], [(50, 30, D[0]), (50, 60, D[1])]], [], [], two, {"ratio_factor": 10.0},
                              dict(n_epi=2, n_accepted=2, n_matches=2, n_new=1, point=[True, False]))
    # ... and in a further observation: three keyframes, base pair = position 0 (the wider baseline); the rows of position 1 lie on the
    # lines and 2.4 / 2.5 px along them from where the points project: 5.76 <= 5.991 < 6.25: both points stay, one observation goes
    three = poses((0.0, 1.0, 2.0))
    c["reprojection_further"] = ([[(70, 30, D[0]), (70, 60, D[1])], [(62.4, 30, D[0]), (62.5, 60, D[1])], [(50, 30, D[0]), (50, 60, D[1])]], [], [], three, {},
                                 dict(n_matches=4, n_new=2, n_obs_new=5, point=[True, True], lists=[[(0, 0), (1, 0), (2, 0)], [(0, 1), (2, 1)]]))
    # scale consistency: rd = d2 / d1 is 1 within 1 % here, ratio_factor 1.8: 1.2^3 = 1.728 passes, 1.2^4 = 2.0736 does not, on either side
    c["scale_ratio"] = ([[(60, 20, D[0], 0), (60, 40, D[1], 0), (60, 60, D[2], 3), (60, 80, D[3], 4)],
                         [(50, 20, D[0], 3), (50, 40, D[1], 4), (50, 60, D[2], 0), (50, 80, D[3], 0)]], [], [], two, {},
                        dict(n_matches=4, n_new=2, point=[True, False, True, False]))
    # claims: target rows 0 and 1 on one line, one neighbour row: 3 bits against 5 - the lower distance; rows 2 and 3 likewise at equal
    # distance - the lower row
    c["claims"] = ([[(60, 30, D[0]), (60, 60, D[1])],
                    [(50, 30, desc(0, range(5))), (50.5, 30, desc(0, range(100, 103))), (50, 60, D[1]), (50.5, 60, D[1])]], [], [], two, {},
                   dict(n_accepted=4, n_matches=2, n_new=2, point=[False, True, True, False], lists=[[(0, 0), (1, 1)], [(0, 1), (1, 2)]]))
    # occupied rows: a map point holds the neighbour's row 0 and the target's row 1; rows 1 / 0 of the same two features are free
    c["occupied"] = ([[(60, 30, D[0]), (60, 60, D[1]), (60, 80, D[2])], [(50, 30, D[0]), (50, 60, D[1]), (50, 80, D[2])]],
                     [[(0, 0)], [(1, 1)]], [[0, -2, 10], [0, 1, 10]], two, {},
                     dict(n_free=2, n_epi=1, n_new=1, point=[False, False, True], lists=[[(0, 0)], [(1, 1)], [(0, 2), (1, 2)]]))
    return c


def base_pair_case():
    """four keyframes, the point (2, 0, 10) exact in positions 0 and 3, half a pixel along the line off in 1 and 2: the point is exact
    only when position 0 - the lowest cosine of the three - is the base pair"""
    D = desc(0)
    four = poses((0.0, 1.0, 2.0, 3.0))
    return [[(70, 50, D)], [(60.5, 50, D)], [(50.5, 50, D)], [(40, 50, D)]], four


def hand(ctx, kfs, obs, xyz, T, image=None, capacity=None):
    """FW.hand_map of a case (with `image` stored for every keyframe in place of the black one)"""
    if image is None:
        return FW.hand_map(ctx, K, T, kfs, xyz, obs, size=SIZE, capacity=capacity)
    from vslam_amd.mapper import LocalMapper
    from tests.map_worlds import kps_array
    m = LocalMapper(K, save_every_keyframe=False, context=ctx)
    for kf, P in zip(kfs, T):
        m.add_keyframe(image, kps_array([[p[0], p[1]] for p in kf], [p[3] if len(p) > 3 else 0 for p in kf]),
                       np.array([p[2] for p in kf], np.uint8).reshape(-1, 32), P)
        assert m.last["n_new"] == 0
    return m
