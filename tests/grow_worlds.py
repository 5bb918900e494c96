"""Constructed maps for the tests of LocalMapper.create_new_map_points (tests/test_grow_cpu.py, tests/test_gpu_grow.py), on the worlds of
tests/map_worlds.py and tests/fuse_worlds.py.  Plain numpy; build_map / hand_map make the device maps.

withheld_points_world: a skip world in which every map point observed at the last keyframe position is taken out of the map while its
keypoints stay in the keyframes: what the call should give back.
Hand maps: camera f = 100, centre (50, 50), image 100 x 100; keyframe k looks down z from x = k (poses()), so a point (a, b, 10) lands
at (50 + 10 a - 10 k, 50 + 10 b): the epipolar lines are the image rows, the epipoles lie at infinity, two neighbouring keyframes see a
point at depth 10 under 5.7 degrees.
large_world: the withheld world at the mapper's keyframe size (about 2000 rows); row_cases: hand maps of up to 2049 rows at the row
edges of k_grow_free and k_grow_search (csrc/map_grow.hip)."""
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


# ---- worlds at the keyframe size the mapper runs at -------------------------------------------------------------------------------------
LARGE = dict(n_w=4000, n_kf=4)
LARGE_STALE = dict(n_w=3400, n_kf=6, removed=(1,), seed=43, decorated=True)
_LARGE = {}


def large_world(stale=False):
    """withheld_points_world at about 2000 rows per keyframe, built once.  Checked on the CPU (tests/test_grow_cpu.py):
    LARGE:       rows [921, 1117, 1924, 1830]; window 0: 1830 free target rows, 847 new points, margins["min"] 2.3e-4
    LARGE_STALE: slots [548, 765, 693, 1087, 1785, 1656], position 1 removed: rows [548, 693, 1087, 1785, 1656], slot != position from
                 position 1 on, keys decorated; window 0: 1656 free target rows, 953 new points, margins["min"] 2.6e-4
    In both no pair of consecutive keyframes (in slot order, as build_map adds them) has a descriptor match that survives the ratio
    test at 0.8, so no growth step of build_map finds a model.  The target and at least one neighbour exceed 1024 rows: k_grow_free
    takes a second trip, k_grow_search a second tile; nothing exceeds 2100 rows, to keep the tests at a few seconds."""
    if stale not in _LARGE:
        w, held = withheld_points_world(**(LARGE_STALE if stale else LARGE))
        free = GR.free_rows(FW.world_inputs(w)[0], w.counts)
        assert free[-1].sum() > 1024 and max(len(f) for f in free[:-1]) > 1024 and 4 <= len(w.counts) <= 6 and w.counts.max() <= 2100, w.counts
        _LARGE[stale] = (w, held)
    return _LARGE[stale]


# ---- hand maps at the row edges of the search ---------------------------------------------------------------------------------------------
# The camera and poses of cases(): a neighbour at x = 0, the target at x = 1; a feature is (60, y, d) in the neighbour and (50, y, d) in
# the target (the point (1, (y - 50) / 10, 10)); other x on the same image row are the same line at another depth (disparity 6 .. 14 px:
# depth 16.7 .. 7.1, parallax 3.4 .. 8 degrees, exact reprojection: every gate behind the search is passed by far).
TILE = 1024                  # GR_TILE of csrc/map_grow.hip, and the rows k_grow_free takes per trip
Y_FILL = (90.0, 10.0)        # the image rows of the fillers: neighbours, target.  The lines used are y = 30, 40, 60: 20 px or more away
FILL = 15                    # the code word of the plain fillers


def padded(n, rows, y_fill):
    """a keyframe of n rows: `rows` = {row: (x, y, descriptor[, octave])}, every other row a filler on the image row y_fill, where no
    epipolar line of the case comes within the gate (2 px at octave 0).  Fillers carry the code word FILL, except one for each
    descriptor of `rows` that stands once: it carries a copy.  Every descriptor then stands at least twice in the keyframe: for any
    query the best two distances are equal, the ratio test of add_keyframe's own growth step keeps nothing and hand_map's n_new == 0
    holds (the device of tests/map_worlds.py)."""
    once = {}
    for p in rows.values():
        once.setdefault(bytes(p[2]), []).append(p[2])
    copies = [v[0] for v in once.values() if len(v) == 1]
    n_fill = n - len(rows)
    assert n_fill >= len(copies) and n_fill - len(copies) != 1 and all(0 <= r < n for r in rows), (n, len(rows), len(copies))
    out = []
    for r in range(n):
        if r in rows:
            out.append(tuple(rows[r]))
        else:
            out.append((5.0 + r % 91, y_fill, copies.pop() if copies else desc(FILL)))
    return out


def owned(key, rows):
    """(obs, xyz) of one single-observation map point per row of keyframe `key`, as in the `occupied` case"""
    rows = list(rows)
    return [[(key, r)] for r in rows], [[0.0, -2.0, 10.0]] * len(rows)


def row_cases():
    """hand maps that put the search of csrc/map_grow.hip at its row edges: name -> (kfs, obs, xyz, poses, keyword arguments,
    expectations), as cases().  expectations: counts (a subset of GR.COUNTS), `point_rows` = the target rows that made a point, `new_lists`
    = the observation lists of the new points (in the order they are appended: by target row), `dref_row` of the new points.  A name's
    part before the first ":" is its family; tests/test_grow_cpu.py shows for every family a wrong reading of the rows it fails under."""
    c = {}
    two = poses((0.0, 1.0))
    D = [desc(j) for j in range(16)]
    tgt1 = padded(2, {0: (50, 30, D[0])}, Y_FILL[1])          # one feature on the line y = 30 and its copy among the fillers: n_free = 2
    one = dict(n_free=2, n_accepted=1, n_matches=1, n_new=1, n_obs_new=2, point_rows=[0])
    # tile_counts: the only row of the neighbour on the line is its last, n2 - 1: the last row of a full tile (1024, 2048), of a tile one
    # short (1023), the single row of a further tile (1025, 2049).  One row passes the gate, one point observing it
    for n2 in (TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1):
        c["tile_counts:%d" % n2] = ([padded(n2, {n2 - 1: (60, 30, D[0])}, Y_FILL[0]), tgt1], [], [], two, {},
                                    dict(one, n_epi=1, new_lists=[[(0, n2 - 1), (1, 0)]]))
    # first_tile_owned: rows 0 .. 1023 of the neighbour all owned, among them row 5 on the line with the target's very descriptor; the
    # free row 1030 on the line is 3 bits off.  Only free rows are staged: the first tile stages none (n = 0), n_epi = 1, row 1030
    ob, X = owned(0, range(TILE))
    c["first_tile_owned:second_tile_free"] = ([padded(TILE + 16, {5: (60, 30, D[0]), 1030: (61, 30, desc(0, (0, 1, 2)))}, Y_FILL[0]), tgt1], ob, X, two, {},
                                              dict(one, n_epi=1, n_points=TILE + 1, new_lists=[[(0, 1030), (1, 0)]]))
    # ... and the whole second tile owned (the decoy in row 1029), the match in row 5 of the first
    ob, X = owned(0, range(TILE, 2 * TILE))
    c["first_tile_owned:second_tile_owned"] = ([padded(2 * TILE, {1029: (60, 30, D[0]), 5: (61, 30, desc(0, (0, 1, 2)))}, Y_FILL[0]), tgt1], ob, X, two, {},
                                               dict(one, n_epi=1, n_points=TILE + 1, new_lists=[[(0, 5), (1, 0)]]))
    # tie_across_tiles: rows 5 and 1029 on the line, both 2 bits off (other bits): the best of the first tile is carried into the
    # second and keeps the tie, row 5.  With row 1029 only 1 bit off it is taken
    for name, far, row in (("equal", (100, 101), 5), ("second_closer", (100,), 1029)):
        c["tie_across_tiles:" + name] = ([padded(TILE + 16, {5: (60, 30, desc(0, (0, 1))), 1029: (61, 30, desc(0, far))}, Y_FILL[0]), tgt1], [], [], two, {},
                                         dict(one, n_epi=2, new_lists=[[(0, row), (1, 0)]]))
    # tie_inside_a_tile: rows 7, 15, .. 1023 (128 rows over the whole tile) on the line at x = 56 + j / 16, row 7 + 8 j 2 bits off the
    # target's descriptor at bits 2 j, 2 j + 1: 128 rows pass the gate at distance 2, each with another descriptor and another depth.
    # The staging order is that of an LDS atomic; the lowest row, 7, whatever it was
    c["tie_inside_a_tile"] = ([padded(TILE, {7 + 8 * j: (56 + j / 16.0, 30, desc(0, (2 * j, 2 * j + 1))) for j in range(128)}, Y_FILL[0]), tgt1], [], [], two, {},
                              dict(one, n_epi=128, new_lists=[[(0, 7), (1, 0)]]))
    # two_waves_one_row: 72 free target rows are two waves of the search (free indices 0 .. 63, 64 .. 71; every row is free, so a row is its
    # own free index).  Rows 3 and 70 lie on the line y = 30, both 3 bits (other bits) off the neighbour's row 0: they meet in the atomicMin
    # on row 0's key only, the lower target row wins, row 70 makes no point.  Rows 4 and 69 on y = 60 against the neighbour's row 1: 3 bits
    # against 2, row 69 wins.  4 gate passes, 4 accepted, 2 matches won
    tgt = padded(72, {3: (50, 30, desc(0, (0, 1, 2))), 70: (50.5, 30, desc(0, (100, 101, 102))),
                      4: (50, 60, desc(1, (0, 1, 2))), 69: (50.5, 60, desc(1, (100, 101)))}, Y_FILL[1])
    c["two_waves_one_row"] = ([[(60, 30, D[0]), (60, 60, D[1])], tgt], [], [], two, {},
                              dict(n_free=72, n_epi=4, n_accepted=4, n_matches=2, n_new=2, n_obs_new=4, point_rows=[3, 69],
                                   new_lists=[[(0, 0), (1, 3)], [(0, 1), (1, 69)]], dref_row=[3, 69]))
    # free_rows_past_1024: a target of 1100 rows, its three features in rows 1030, 1060, 1099 (lines y = 30, 40, 60; the neighbour's rows 0, 1,
    # 2).  n_free = 1024 and 1025: 76 and 75 owned rows sprinkled below 1024 (rows 1, 14, 27, ..): the second trip of k_grow_free writes
    # behind the 948 / 949 free rows of the first.  n_free = 63, 64, 65: every row owned but the three and 60, 61, 62 others (rows 2, 19, 36,
    # .. 1022, 1039): one wave short of a lane, one full wave and no second, a second wave with one live lane - row 1099, the last free
    # row, which has a match.  Three gate passes, three points, appended in row order
    nb = [(60, 30, D[0]), (60, 40, D[1]), (60, 60, D[2])]
    feats = {1030: (50, 30, D[0]), 1060: (50, 40, D[1]), 1099: (50, 60, D[2])}
    tgt = padded(1100, feats, Y_FILL[1])
    n_frees = (63, 64, 65, TILE, TILE + 1)
    for nf in n_frees:
        if nf >= TILE:
            taken = [1 + 13 * i for i in range(1100 - nf)]
            assert max(taken) < TILE
        else:
            free = sorted(set(feats) | {2 + 17 * i for i in range(nf - 3)})
            assert len(free) == nf and min(free) < TILE
            taken = [r for r in range(1100) if r not in free]
        assert 1100 - len(taken) == nf and not set(taken) & set(feats)
        ob, X = owned(1, taken)
        c["free_rows_past_1024:%d" % nf] = ([nb, tgt], ob, X, two, {},
                                            dict(n_free=nf, n_epi=3, n_accepted=3, n_matches=3, n_new=3, n_obs_new=6, point_rows=sorted(feats),
                                                 new_lists=[[(0, j), (1, r)] for j, r in enumerate(sorted(feats))], dref_row=sorted(feats)))
    # empty_and_full_neighbours: four keyframes at x = 0 .. 3, the feature is the point (3, -2, 10): (50, 30) in the target, (60, 30) at
    # position 2, (80, 30) at position 0.  Position 0: two rows on the line with the target's descriptor, both owned.  Position 1: no row.
    # Position 2: rows 0 and 1 on the line, both 2 bits off: row 0.  Counts as for position 2 alone: 2 gate passes, one accepted
    four = poses((0.0, 1.0, 2.0, 3.0))
    ob, X = owned(0, range(2))
    kfs = [[(80, 30, D[0]), (80.5, 30, D[0])], [], [(60, 30, desc(0, (0, 1))), (60.5, 30, desc(0, (100, 101)))], tgt1]
    c["empty_and_full_neighbours"] = (kfs, ob, X, four, {}, dict(one, n_neighbours=3, n_epi=2, n_points=3, new_lists=[[(2, 0), (3, 0)]]))
    # what the cases must cover, whatever is edited above
    assert {int(k.split(":")[1]) for k in c if k.startswith("tile_counts:")} == {1023, 1024, 1025, 2048, 2049}
    assert {v[5]["n_free"] for k, v in c.items() if k.startswith("free_rows_past_1024:")} == {63, 64, 65, 1024, 1025}
    assert all(len(kf) <= 2 * TILE + 1 for v in c.values() for kf in v[0]) and all(len(v[0]) <= 4 for v in c.values())
    return c


def families(c):
    return sorted({k.split(":")[0] for k in c})


def missed(want, a, point, cnt, n_old):
    """the expectations of a case (cases() / row_cases()) that a result does not meet: [] when it holds"""
    bad = [k for k in want if k in GR.COUNTS and cnt[k] != want[k]]
    lists = FW.FR.lists_of(a)
    if "point" in want and (point >= 0).tolist() != want["point"]:
        bad.append("point")
    if "point_rows" in want and np.flatnonzero(point >= 0).tolist() != want["point_rows"]:
        bad.append("point_rows")
    if "lists" in want and lists != want["lists"]:
        bad.append("lists")
    if "new_lists" in want and lists[n_old:] != want["new_lists"]:
        bad.append("new_lists")
    if "dref_row" in want and a["dref_row"][n_old:].tolist() != want["dref_row"]:
        bad.append("dref_row")
    return bad


# the wrong readings of the rows that a row case must notice (tests/test_grow_cpu.py): what a kernel would compute that
MUTATIONS = ("neighbours_cut", "target_cut", "ties_high")   # stopped after a neighbour's first tile / after k_grow_free's first trip / took ties upward


def run_mutated(kfs, obs, xyz, T, kw, mutation):
    """run() of a case under one wrong reading.  The cuts are made on the inputs: a keyframe cut to its first TILE rows (an observation
    of a row behind the cut names no row and is skipped, as any stale key); `point` is filled up to the target's rows again"""
    n_t = len(kfs[-1])
    if mutation == "neighbours_cut":
        kfs = [kf[:TILE] for kf in kfs[:-1]] + [kfs[-1]]
    elif mutation == "target_cut":
        kfs = list(kfs[:-1]) + [kfs[-1][:TILE]]
    else:
        assert mutation == "ties_high"
        kw = dict(kw, ties=-1)
    a, point, points, cnt, margins = run(kfs, obs, xyz, T, **kw)
    return a, np.concatenate([point, np.full(n_t - len(point), -1, np.int32)]), points, cnt, margins
