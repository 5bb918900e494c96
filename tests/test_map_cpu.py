"""CPU checks of the LocalMapper pieces that need no GPU: the numpy restatement of the reference's bookkeeping on hand-built maps,
and the native PLY float formatter against Python's own formatting."""
import ctypes as C

import numpy as np
import pytest

from tests.map_restatement import RefMapper, cull_arrays, reproj_err

K = np.array([[320.0, 0, 320.0], [0, 320.0, 240.0], [0, 0, 1.0]])


def _pose(tx):
    T = np.eye(4)
    T[0, 3] = tx
    return T


def _mapper(n_kf, xy):
    m = RefMapper(K)
    for k in range(n_kf):
        m.keyframes.append({"id": k, "image": None, "xy": np.asarray(xy, np.float32), "pose": _pose(-0.1 * k),
                            "P": K @ np.hstack((np.eye(3), np.array([[-0.1 * k], [0], [0]]))), "map_points": []})
    return m


def test_point_exactly_at_the_threshold_is_kept():
    # a point at depth 1 on the optical axis projects to (320, 240); a keypoint 5 px to the right is exactly at the threshold
    m = _mapper(2, [[325.0, 240.0], [320.0, 240.0], [326.0, 240.0]])
    assert reproj_err(m.keyframes[0]["P"], [0, 0, 1], [325.0, 240.0]) == 5.0
    m.map_points = [{"id": 0, "position": np.float32([0, 0, 1]), "color": np.zeros(3), "observed_keyframes": {0: 0, 0 - 2: 1}},
                    {"id": 1, "position": np.float32([0, 0, 1]), "color": np.zeros(3), "observed_keyframes": {0: 2, 1: 1}}]
    m.cull_map_points()
    assert [p["id"] for p in m.map_points] == [0]   # 5.0 is not > 5.0; 6 px is


def test_index_error_like_the_reference():
    m = _mapper(2, [[320.0, 240.0]])
    m.map_points = [{"id": 0, "position": np.float32([0, 0, 1]), "color": np.zeros(3), "observed_keyframes": {0: 0, 5: 0}}]
    with pytest.raises(IndexError):
        m.cull_map_points()
    m.map_points = [{"id": 0, "position": np.float32([0, 0, 1]), "color": np.zeros(3), "observed_keyframes": {0: 0, 1: 3}}]
    with pytest.raises(IndexError):
        m.cull_map_points()
    # an earlier failing observation ends the test before the bad index is reached
    m.map_points = [{"id": 0, "position": np.float32([0, 0, 1]), "color": np.zeros(3), "observed_keyframes": {0: 0, 1: 0, 9: 0}}]
    m.keyframes[1]["xy"] = np.float32([[400.0, 240.0]])
    m.cull_map_points()
    assert m.map_points == []


def test_duplicate_ids_and_first_point_lookup():
    xy = [[320.0, 240.0]] * 4
    m = _mapper(6, xy)
    for k in range(6):
        m.keyframes[k]["P"] = K @ np.hstack((np.eye(3), np.zeros((3, 1))))
    few = {"id": 7, "position": np.float32([0, 0, 1]), "color": np.zeros(3), "observed_keyframes": {1: 0, 2: 0}}
    many = {"id": 7, "position": np.float32([0, 0, 1]), "color": np.zeros(3), "observed_keyframes": {1: 0, 2: 0, 3: 0, 4: 0}}
    m.map_points = [few, many]
    m.cull_map_points()
    assert m.keyframes[1]["map_points"] == [7, 7]
    # the FIRST point with id 7 has 1 other observation: not redundant, although the second one would be
    assert m.keyframe_counts()[1] == (2, 0)


def test_stale_ids_after_renumbering():
    m = _mapper(6, [[320.0, 240.0]] * 30)
    for k in range(6):
        m.keyframes[k]["P"] = K @ np.hstack((np.eye(3), np.zeros((3, 1))))
    m.map_points = [{"id": i, "position": np.float32([0, 0, 1]), "color": np.zeros(3),
                     "observed_keyframes": {1: i, 2: i, 3: i, 4: i, 0: i}} for i in range(25)]
    m.co_visibility_graph[1][2] += 25; m.co_visibility_graph[2][1] += 25
    m.cull_map_points()
    removed = m.cull_keyframes()
    assert removed == [1, 2, 3]
    assert [k["id"] for k in m.keyframes] == [0, 1, 2]
    assert 1 not in m.co_visibility_graph and 2 not in m.co_visibility_graph[1]
    # observations keep the old ids: keyframe 4 no longer exists, the next cull raises IndexError as the reference would
    assert m.map_points[0]["observed_keyframes"] == {1: 0, 2: 0, 3: 0, 4: 0, 0: 0}
    with pytest.raises(IndexError):
        m.cull_map_points()


def test_vectorised_cull_equals_the_loop():
    rng = np.random.default_rng(3)
    m = _mapper(4, rng.uniform(0, 640, (50, 2)))
    n = 400
    xyz = np.column_stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(2, 4, n)]).astype(np.float32)
    cnt = rng.integers(1, 5, n)
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    # distinct keyframe positions per point, some written as negative positions (Python indexing from the end)
    okf = np.concatenate([rng.permutation(4)[:c] - 4 * rng.integers(0, 2, c) for c in cnt]).astype(np.int32)
    for k in range(4):   # one camera for all four keyframes: a point's observations of the same keypoint agree
        m.keyframes[k]["P"] = K @ np.hstack((np.eye(3), np.zeros((3, 1))))
    # every observation of a point names the same keypoint, a third of them another one; points placed within ~6 px of it
    okp = np.repeat(rng.integers(0, 50, n), cnt).astype(np.int32)
    other = rng.random(off[-1]) < 0.3
    okp[other] = rng.integers(0, 50, other.sum())
    for i in range(n):
        u, v = m.keyframes[0]["xy"][okp[off[i]]] + rng.normal(0, 4.0, 2)
        z = xyz[i, 2]
        xyz[i, 0] = (u - 320) * z / 320
        xyz[i, 1] = (v - 240) * z / 320
    keep, near = cull_arrays([k["P"] for k in m.keyframes], [k["xy"] for k in m.keyframes], xyz, off, okf, okp)
    m.map_points = [{"id": i, "position": xyz[i], "color": np.zeros(3),
                     "observed_keyframes": dict(zip(okf[off[i]:off[i + 1]].tolist(), okp[off[i]:off[i + 1]].tolist()))} for i in range(n)]
    m.cull_map_points()
    assert [p["id"] for p in m.map_points] == np.flatnonzero(keep).tolist()
    assert 0 < keep.sum() < n


def _fmt(lib, v):
    v = np.ascontiguousarray(v, np.float32)
    ln = C.c_size_t(0)
    assert lib.mo_format_floats(v.ctypes.data_as(C.c_void_p), len(v), None, 0, C.byref(ln)) == 0
    buf = C.create_string_buffer(ln.value)
    assert lib.mo_format_floats(v.ctypes.data_as(C.c_void_p), len(v), buf, ln.value, C.byref(ln)) == 0
    return buf.raw[:ln.value].decode()


def test_native_float_format_equals_python():
    """the PLY writer's floats are f"{np.float32}" = the repr of the double value: 10^7 random f32 bit patterns (subnormals, +-0,
    inf and nan among them) formatted natively equal Python's text"""
    import vslam_amd as V
    lib = V.load_library()
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e16, 1e15, 9.999999e15, 1e-4, 1e-5, 0.0001234, 123456789.0, 1.5,
                        np.float32(0.1257302165031433), 1.4e-45, -3.4028235e38, 16777216.0], np.float32)
    assert _fmt(lib, special) == "".join(f"{x}\n" for x in special)
    rng = np.random.default_rng(20251016)
    for _ in range(10):
        v = rng.integers(0, 2 ** 32, 10 ** 6, dtype=np.uint64).astype(np.uint32).view(np.float32)
        got = _fmt(lib, v)
        want = "\n".join(map(repr, v.astype(np.float64).tolist())) + "\n"
        assert got == want
