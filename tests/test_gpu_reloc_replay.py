"""LocalMapper.relocalize (mo_map_relocalize) on the device against the host replay of its geometry (tests/native/reloc_replay.cpp) on
the constructed cases of tests/reloc_cases.py.  What the call downloaded is read back through mo_dbg_map_reloc_last: the winning key
of every candidate, the final counts and the refined poses.  Keys, counts, flags and the winner are integers and must be equal; the
poses are held to REFINE_TOL, the project's bound for a device refinement against its restatement (libm's sin / cos differ)."""
import ctypes as C
import shutil
import time

import numpy as np
import pytest

from tests import reloc_cases as RC
from tests.test_gpu_map_reads import REFINE_TOL

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("g++") is None, reason="needs a host C++ compiler")]

CASES = {c.name: c for c in RC.all_cases()}


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    d = tmp_path_factory.mktemp("reloc_replay")
    exe = RC.build_replay(d)
    done = {}

    def get(case):
        if case.name not in done:
            done[case.name] = RC.run_replay(exe, case, d)
        return done[case.name]
    return get


@pytest.fixture(scope="module")
def ctx():
    import vslam_amd as V
    c = V.Context(device=0, max_w=640, max_h=480, max_batch=1)
    yield c
    c.close()


def _probe(m):
    """(rc, dict) of mo_dbg_map_reloc_last"""
    import vslam_amd as V
    n = C.c_int32(-7)
    cand, ncorr, ninl = (np.full(64, -7, np.int32) for _ in range(3))
    best = np.full(64, 7, np.uint64)
    pose = np.full((64, 12), 7.0)
    rc = m.lib.mo_dbg_map_reloc_last(m._h, C.byref(n), V._ptr(cand), V._ptr(best), V._ptr(ncorr), V._ptr(ninl), V._ptr(pose))
    return rc, {"n_cand": int(n.value), "cand": cand, "best": [int(b) for b in best], "ncorr": ncorr, "ninl": ninl, "pose": pose}


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_the_replay(name, replay, ctx):
    case = CASES[name]
    rp = replay(case)
    RC.check(case, rp)   # the case's conditions, before any device is asked
    f, prm = case.front(), case.prm
    t0 = time.perf_counter()
    m = case.build_map(ctx)
    kps, desc = case.query()
    t1 = time.perf_counter()
    ok, pose, info = m.relocalize(kps, desc, threshold=prm["thr_px"], min_inliers=prm["min_inliers"], max_candidates=prm["max_candidates"],
                                  n_hyp=prm["n_hyp"], seed=prm["seed"])
    t2 = time.perf_counter()
    rc, dbg = _probe(m)
    assert rc == 0
    m.close()
    cands, nc, win = f["candidates"], len(f["candidates"]), rp["winner"]
    # integer front: the restatement's candidates, scores and the winner's correspondences
    assert [c[0] for c in info["candidates"]] == cands and dbg["n_cand"] == nc and dbg["cand"][:nc].tolist() == cands
    assert [c[1] for c in info["candidates"]] == [f["scores"][k] for k in cands] == dbg["ncorr"][:nc].tolist()
    assert (dbg["cand"][nc:] == -1).all() and not any(dbg["best"][nc:]) and not dbg["ninl"][nc:].any() and np.isnan(dbg["pose"][nc:]).all()
    assert info["kf_pos"] >= 0
    qi, pi = f["C"][info["kf_pos"]]
    assert np.array_equal(np.flatnonzero(info["point"] >= 0), qi) and np.array_equal(info["point"][qi], pi)
    assert info["n_corr"] == len(qi) >= case.floor
    # keys: 64-bit integers, equal
    for c in range(nc):
        assert dbg["best"][c] == rp["best"][c], (name, c, RC.key_parts(dbg["best"][c]), RC.key_parts(rp["best"][c]))
    # counts and flags
    assert dbg["ninl"][:nc].tolist() == rp["ninl"]
    assert [c[2] for c in info["candidates"]] == rp["ninl"]
    assert info["kf_pos"] == cands[win] and info["n_inliers"] == rp["ninl"][win]
    assert ok == (rp["ninl"][win] >= prm["min_inliers"] and rp["best"][win] != 0)
    if "ok" in case.expect:
        assert ok == case.expect["ok"]
    want = np.zeros(len(case.q_words), bool)
    want[qi[rp["flags"][win]]] = True
    assert np.array_equal(info["inlier"], want)
    # poses
    worst = 0.0
    for c in range(nc):
        if rp["best"][c]:
            assert np.allclose(dbg["pose"][c], rp["pose"][c], **REFINE_TOL), (name, c, dbg["pose"][c] - rp["pose"][c])
            worst = max(worst, np.abs(dbg["pose"][c] - rp["pose"][c]).max())
        else:
            assert np.isnan(dbg["pose"][c]).all()
    assert np.array_equal(pose[:3].reshape(12), dbg["pose"][win], equal_nan=True)
    if case.empty:   # no pose: not ok, 0 inliers, an all-NaN pose, no inlier set
        assert not ok and info["n_inliers"] == 0 and np.isnan(pose[:3]).all() and not info["inlier"].any() and dbg["best"][win] == 0
    else:
        assert dbg["best"][win] >> 32 > 0 and info["inlier"].sum() == info["n_inliers"] > 0
    print("%s: largest pose difference to the replay %.3g; map %.3f s, relocalize %.3f s" % (name, worst, t1 - t0, t2 - t1))


def test_probe_before_the_first_relocalization(ctx):
    import vslam_amd as V
    case = CASES["all_inliers_tie"]
    m = case.build_map(ctx)
    rc, _ = _probe(m)
    assert rc == V.MO_ERR_ARG
    m.relocalize(np.zeros(0, V.KP_DTYPE), np.zeros((0, 32), np.uint8))   # nothing to match: no chain runs
    rc, _ = _probe(m)
    assert rc == V.MO_ERR_ARG
    m.relocalize(*case.query(), n_hyp=4)
    rc, dbg = _probe(m)
    assert rc == V.MO_OK and dbg["n_cand"] == 1 and dbg["cand"][0] == 1
    m.close()
