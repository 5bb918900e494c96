"""Every call that rebuilds the map store, one behind the other on one LocalMapper (tests/rebuild_chain_world.py has the map and the
chain): after each step the map's arrays, the life records, the sizes the library reports and what the call returned equal the numpy
restatement of that step applied to the restated state in front of it.  Integers and copies only: everything must be equal.  What no
single feature's test asserts is that one rebuild leaves the store, the choice of the live copy and the device's live counts right for
a different rebuild behind it.  tests/test_rebuild_chain_cpu.py shows that the world holds the cases."""
import ctypes as C

import numpy as np
import pytest

from tests import fuse_restatement as FR
from tests import rebuild_chain_world as RC

pytestmark = pytest.mark.gpu


def _state(m):
    """(arrays, life [n][3], sizes) as the library holds them now"""
    s = (C.c_int64 * 6)()
    assert m.lib.mo_map_sizes(m._h, s) == 0   # (the library's own answer, not the mapper's cached sizes)
    m._cache = None
    a = {k: v.copy() for k, v in m.arrays().items()}
    p = m.point_life()
    return a, np.column_stack([p["visible"], p["found"], p["born"]]).astype(np.int32).reshape(-1, 3), (int(s[1]), int(s[2]))


def _equal(m, step, want):
    a, life, sizes = _state(m)
    for f in FR.FIELDS:
        assert a[f].dtype == want[f].dtype and a[f].shape == want[f].shape and a[f].tobytes() == want[f].tobytes(), (step, f)
    assert np.array_equal(life, want["life"]), step
    assert sizes == (len(want["id"]), len(want["obs_kf"])), (step, sizes)
    assert [kf._rows for kf in m.keyframes] == want["counts"].tolist(), step


def test_every_rebuild_behind_every_other():
    import vslam_amd as V
    ctx = V.Context(device=0, max_w=640, max_h=480, max_batch=1)
    chain = RC.restated()
    m = RC.build(ctx)
    try:
        _equal(m, "start", chain[0][1])
        for (_, before), (step, want) in zip(chain, chain[1:]):
            got = RC.apply(m, step, before)
            _equal(m, step, want)
            if "remap" in want and step != "add_keyframe":
                assert got.dtype == np.int32 and np.array_equal(got, want["remap"]), step
            if step.startswith("erase_observations"):
                assert got == want["info"], (step, got)
            if step == "fuse_map_points":
                assert np.array_equal(got["into"], want["into"]) and {k: got[k] for k in FR.COUNTS} == want["info"], step
        assert ctx.dev_status() == 0
    finally:
        m.close(); ctx.close()
