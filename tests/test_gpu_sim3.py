"""LocalMapper.compute_sim3 (mo_map_loop_sim3) on the device against the host replay of its geometry (tests/native/sim3_replay.cpp) on
the constructed cases of tests/sim3_cases.py, and detect_loop(sim3=True) on a loop world whose return side is rescaled.  What the call
downloaded is read back through mo_dbg_map_sim3_last.  Keys, counts, flags, the winner and ok are integers and must be equal; the
models are held to REFINE_TOL, the project's bound for a device refinement against its restatement (libm's exp / sin / cos differ)."""
import copy
import ctypes as C
import shutil
import time

import numpy as np
import pytest

from tests import sim3_cases as SC
from tests.test_gpu_map_reads import POSE_TRUTH, REFINE_TOL

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("g++") is None, reason="needs a host C++ compiler")]

CASES = {c.name: c for c in SC.all_cases()}
STAGES = ["sim3_gather", "sim3_hyp", "sim3_refine", "sim3_finish"]


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    d = tmp_path_factory.mktemp("sim3_replay")
    exe = SC.build_replay(d)
    done = {}

    def get(case):
        if case.name not in done:
            done[case.name] = SC.run_replay(exe, case, d)
        return done[case.name]
    return get


@pytest.fixture(scope="module")
def ctx():
    import vslam_amd as V
    c = V.Context(device=0, max_w=640, max_h=480, max_batch=1)
    yield c
    c.close()


def _probe(m):
    """(rc, dict) of mo_dbg_map_sim3_last"""
    import vslam_amd as V
    n, win = C.c_int32(-7), C.c_int32(-7)
    cand, ncorr, ninl = (np.full(16, -7, np.int32) for _ in range(3))
    best = np.full(16, 7, np.uint64)
    model = np.full((16, 13), 7.0)
    rc = m.lib.mo_dbg_map_sim3_last(m._h, C.byref(n), C.byref(win), V._ptr(cand), V._ptr(best), V._ptr(ncorr), V._ptr(ninl), V._ptr(model))
    return rc, {"n_cand": int(n.value), "win": int(win.value), "cand": cand, "best": [int(b) for b in best], "ncorr": ncorr, "ninl": ninl, "model": model}


def _align(m, case, **over):
    return m.compute_sim3(case.candidates(), kf_position=case.p, **dict(case.prm, **over))


def _model(c):
    return np.concatenate([[c["scale"]], c["R"].reshape(9), c["t"]])


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_the_replay(name, replay, ctx):
    """Noise-free cases also against the constructed truth.  The replay misses POSE_TRUTH with a factor of ten to spare on them (map
    points and keypoints are f32; tests/sim3_cases.py lists its errors, 1.58e-6 at most), so the bound is SC.TRUTH_BOUND = 1.6e-5, ten
    times the replay's largest measured error."""
    case = CASES[name]
    rp = replay(case)
    SC.check(case, rp)   # the case's conditions, before any device is asked
    t0 = time.perf_counter()
    m = case.build_map(ctx)
    t1 = time.perf_counter()
    ok, info = _align(m, case)
    t2 = time.perf_counter()
    rc, dbg = _probe(m)
    assert rc == 0
    nc, n_p, pairs = len(case.cand), len(case.cur_point), case.pairs()
    res = info["candidates"]
    # the probe and the call tell the same
    assert dbg["n_cand"] == nc == len(res) and dbg["cand"][:nc].tolist() == case.cand == [c["pos"] for c in res]
    assert (dbg["cand"][nc:] == -1).all() and not any(dbg["best"][nc:]) and not dbg["ninl"][nc:].any() and not dbg["ncorr"][nc:].any()
    assert np.isnan(dbg["model"][nc:]).all()
    assert [c["n_corr"] for c in res] == dbg["ncorr"][:nc].tolist() and [c["n_inliers"] for c in res] == dbg["ninl"][:nc].tolist()
    assert all(np.array_equal(_model(c), dbg["model"][i], equal_nan=True) for i, c in enumerate(res))
    # integers: equal to the replay
    assert dbg["ncorr"][:nc].tolist() == rp["m"]
    for c in range(nc):
        assert dbg["best"][c] == rp["best"][c], (name, c, SC.key_parts(dbg["best"][c]), SC.key_parts(rp["best"][c]))
    assert dbg["ninl"][:nc].tolist() == rp["ninl"]
    for c in range(nc):
        want = np.zeros(n_p, bool)
        want[pairs[c][0][rp["flags"][c]]] = True
        assert res[c]["inlier"].shape == (n_p,) and np.array_equal(res[c]["inlier"], want), (name, c)
    assert info["win"] == dbg["win"] == rp["winner"] and ok == rp["ok"]
    assert info["n_inliers"] == (rp["ninl"][rp["winner"]] if rp["winner"] >= 0 else 0)
    if "ok" in case.expect:
        assert ok == case.expect["ok"]
    # models
    worst, worst_truth = 0.0, 0.0
    for c in range(nc):
        if rp["best"][c]:
            assert np.allclose(dbg["model"][c], rp["model"][c], **REFINE_TOL), (name, c, dbg["model"][c] - rp["model"][c])
            worst = max(worst, np.abs(dbg["model"][c] - rp["model"][c]).max())
            if case.truth[c] is not None:
                e = np.abs(dbg["model"][c] - SC.model_of(case.truth[c])).max()
                assert e < SC.TRUTH_BOUND, (name, c, e)
                worst_truth = max(worst_truth, e)
        else:
            assert np.isnan(dbg["model"][c]).all() and not res[c]["inlier"].any() and res[c]["n_inliers"] == 0
    if info["win"] >= 0:
        w = res[info["win"]]
        S = np.eye(4)
        S[:3, :3], S[:3, 3] = w["scale"] * w["R"], w["t"]
        assert np.allclose(info["world"], np.linalg.inv(case.poses[case.p]) @ S @ case.poses[w["pos"]], rtol=1e-12, atol=1e-12)
    else:
        assert info["world"] is None
    m.close()
    print("%s: largest model difference to the replay %.3g, to the truth %.3g (POSE_TRUTH %.3g, bound %.3g); map %.3f s, call %.3f s"
          % (name, worst, worst_truth, POSE_TRUTH, SC.TRUTH_BOUND, t1 - t0, t2 - t1))


def test_two_calls_give_equal_bytes(ctx):
    from tests.test_gpu_scratch_poison import _flat
    for name in ("pair_counts:129", "sixteen_candidates"):
        case = CASES[name]
        m = case.build_map(ctx)
        a = _flat(_align(m, case))
        other = _flat(_align(m, case, seed=case.prm["seed"] + 1))   # another call in between leaves its own scratch behind
        assert _flat(_align(m, case)) == a and [p for p, _ in other] == [p for p, _ in a]
        m.close()


def test_stage_names(ctx):
    case = CASES["geometry:s1.7"]
    m = case.build_map(ctx)
    ctx.set_host_timing(True)
    ok, _ = _align(m, case)
    names = [n for n, _ in ctx.stage_times()]
    ctx.set_host_timing(False)
    m.close()
    assert ok and names == STAGES


def _raw(m, case, K="case", poses="case", prm=True, out=True, **over):
    """mo_map_loop_sim3 called directly: (rc, MapSim3Out)"""
    import vslam_amd as V
    n_kf, nc, n_p = len(case.poses), len(case.cand), len(case.cur_point)
    Ka = np.ascontiguousarray(case.K, np.float64).reshape(9) if isinstance(K, str) else K
    Pa = np.ascontiguousarray(np.stack([T[:3, :4] for T in case.poses]), np.float64).reshape(n_kf, 12) if isinstance(poses, str) else poses
    cand = np.array(over.pop("cand", case.cand), np.int32)
    f = dict(kf_pos=case.p, n_cand=nc, n_hyp=case.prm["n_hyp"], min_inliers=case.prm["min_inliers"], seed=case.prm["seed"], chi2=case.prm["chi2"],
             scale_factor=case.prm["scale_factor"])
    f.update(over)
    cur, mpt, mrow = (np.ascontiguousarray(a, np.int32) for a in (case.cur_point, case.match_point, case.match_row))
    p = V.MapSim3Params(f["kf_pos"], f["n_cand"], cand.ctypes.data, cur.ctypes.data, mpt.ctypes.data, mrow.ctypes.data, f["n_hyp"], f["min_inliers"],
                        f["seed"], f["chi2"], f["scale_factor"])
    o = V.MapSim3Out()   # every output array NULL
    o.win, o.ok, o.win_inliers = 5, 5, 5
    rc = m.lib.mo_map_loop_sim3(m._h, V._ptr(Ka), V._ptr(Pa), C.byref(p) if prm else None, C.byref(o) if out else None)
    return rc, o


def test_errors_and_the_probe_before_the_first_call(ctx):
    import vslam_amd as V
    from vslam_amd.mapper import LocalMapper
    case = CASES["geometry:s1.0"]
    m = case.build_map(ctx)
    n_kf = len(case.poses)
    assert _probe(m)[0] == V.MO_ERR_ARG                                          # no alignment has run
    rc, o = _raw(m, case, n_cand=0)
    assert rc == V.MO_OK and (o.win, o.ok, o.win_inliers) == (-1, 0, 0)
    assert _probe(m)[0] == V.MO_ERR_ARG                                          # n_cand = 0 runs no chain
    nan_K = np.ascontiguousarray(case.K, np.float64).reshape(9).copy(); nan_K[4] = np.nan
    inf_P = np.stack([T[:3, :4] for T in case.poses]).reshape(n_kf, 12).copy(); inf_P[1, 3] = np.inf
    for bad in (dict(K=None), dict(poses=None), dict(prm=False), dict(out=False), dict(K=nan_K), dict(poses=inf_P), dict(kf_pos=n_kf), dict(kf_pos=-1),
                dict(cand=[n_kf]), dict(cand=[-1]), dict(n_cand=17), dict(n_cand=-1), dict(n_hyp=0), dict(n_hyp=(1 << 20) + 1),
                dict(chi2=float("nan")), dict(scale_factor=0.0)):
        assert _raw(m, case, **bad)[0] == V.MO_ERR_ARG, bad
    assert _raw(m, case, kf_pos=n_kf, n_cand=0)[0] == V.MO_ERR_ARG              # kf_pos is checked before the empty list returns
    assert _probe(m)[0] == V.MO_ERR_ARG
    rc, o = _raw(m, case)                        # every output array NULL: legal
    assert rc == V.MO_OK and o.win == 0 and o.ok == 1 and o.win_inliers == 30
    rc, dbg = _probe(m)
    assert rc == V.MO_OK and dbg["n_cand"] == 1 and dbg["cand"][0] == case.cand[0] and dbg["win"] == 0
    empty = LocalMapper(case.K, save_every_keyframe=False, context=ctx)
    rc, o = _raw(empty, case, poses=np.zeros((1, 12)))
    assert rc == V.MO_OK and (o.win, o.ok, o.win_inliers) == (-1, 0, 0)
    ok, info = empty.compute_sim3([])
    assert not ok and info["win"] == -1 and info["candidates"] == [] and info["world"] is None
    m.close(); empty.close()


def test_poison():
    """the call under the poison bytes 255, 0 and 90 returns the bytes it returns without, the fill totals grow, the maps keep theirs"""
    from tests.test_gpu_scratch_poison import _ctx, _read_sweep
    ctx = _ctx()
    cases = [CASES[n] for n in ("sixteen_candidates", "pair_counts:129", "collinear_sample", "missing_entries")]
    maps = [c.build_map(ctx) for c in cases]
    calls = [(c.name, lambda c=c, m=m: _align(m, c)) for c, m in zip(cases, maps)]
    assert calls[0][1]()[0] and calls[1][1]()[0]   # the reads find what they look for: nothing below compares empty results
    _read_sweep(ctx, maps, calls)
    for m in maps:
        m.close()
    ctx.close()


# ---- end to end: a loop world whose return side drifted in scale ---------------------------------------------------------------------
FACTOR = 1.3


def _rescaled(w, factor, scramble=None):
    """tests/loop_worlds.LoopWorld with its return side - the return keyframes and the duplicate points they observe - rescaled about the
    map's origin: positions times factor, the translation of the poses times factor, every projection unchanged.  scramble: a
    generator; each duplicate is moved by up to 2 units in every axis instead: the same descriptors and observations, so the same
    candidates and matches, but no similarity aligns the points."""
    from tests import loop_worlds as LW
    v = copy.copy(w)
    v.kf_poses = [T.copy() for T in w.kf_poses]
    for pos in LW.RETURN_POS:
        v.kf_poses[pos][:3, 3] *= factor
    v.points = [dict(q) for q in w.points]
    for q in v.points[w.n_old:]:
        q["position"] = np.asarray(q["position"], np.float64) * factor
        if scramble is not None:
            q["position"] = q["position"] + scramble.uniform(-2.0, 2.0, 3)
    return v


def _detect(m, **kw):
    from tests import loop_worlds as LW
    m._loop_consistency = None
    return [m.detect_loop(p, **kw) for p in LW.RETURN_POS]


def test_detect_loop_with_sim3_on_a_rescaled_loop_world():
    """The true candidate is accepted with the scale the return side was rescaled by; a look-alike - the same rows and matches over
    points that do not align - is rejected; without the flag both worlds answer as before.  Bound on the scale: the points and
    keypoints are f32 like those of the constructed cases, whose bound SC.TRUTH_BOUND is."""
    import vslam_amd as V
    from tests import loop_worlds as LW
    from tests.test_gpu_scratch_poison import _flat
    c = V.Context(device=0, max_w=640, max_h=480, max_batch=1)
    base = LW.loop_world()
    words, weights = LW.loop_vocabulary()
    voc = V.Vocabulary.from_arrays(words, weights, context=c)
    worlds = {"plain": base, "rescaled": _rescaled(base, FACTOR), "scrambled": _rescaled(base, FACTOR, np.random.default_rng(3))}
    plain = {}
    for tag, w in worlds.items():
        m = w.build(c)
        m.set_vocabulary(voc)
        before = {f: x.copy() for f, x in m.arrays().items()}
        plain[tag] = _detect(m)
        assert [f for f, _ in plain[tag]] == [p == 26 for p in LW.RETURN_POS], tag
        assert all("sim3" not in (x or {}) for _, i in plain[tag] for x in [i["accepted"]])
        got = _detect(m, sim3=True, seed=11)
        found, info = got[-1]
        acc = plain[tag][-1][1]["accepted"]
        if tag == "scrambled":
            assert [f for f, _ in got] == [False] * 4 and info["accepted"] is None
            tried = [x for x in info["candidates"] if "sim3_ok" in x]
            assert tried and not any(x["sim3_ok"] for x in tried) and tried[0]["pos"] == acc["pos"]
        else:
            assert [f for f, _ in got] == [p == 26 for p in LW.RETURN_POS]
            a = info["accepted"]
            assert a["pos"] == acc["pos"] and a["sim3_ok"] and a["sim3"]["n_inliers"] >= 20 and a["sim3"]["n_corr"] == a["n_match"]
            want = FACTOR if tag == "rescaled" else 1.0
            T1, T2 = w.kf_poses[26], w.kf_poses[a["pos"]]
            # the same physical point: X1 = want (R1 X + t1 / want ...): s = want, R = R1 R2^T, t = t1 - want R t2 (t1 is already rescaled)
            R = T1[:3, :3] @ T2[:3, :3].T
            t = T1[:3, 3] - want * R @ T2[:3, 3]
            print("%s: scale %.9g (want %g), %d inliers of %d" % (tag, a["sim3"]["scale"], want, a["sim3"]["n_inliers"], a["sim3"]["n_corr"]))
            assert abs(a["sim3"]["scale"] - want) < SC.TRUTH_BOUND
            assert np.abs(a["sim3"]["R"] - R).max() < SC.TRUTH_BOUND and np.abs(a["sim3"]["t"] - t).max() < SC.TRUTH_BOUND
            # world: takes a point of the old side onto the return side
            X = np.array([1.0, 0.5, 8.0, 1.0])
            assert np.abs(a["sim3"]["world"] @ X - np.append(want * X[:3], 1.0)).max() < 1e-3
        # without the flag: what it returned before, the bookkeeping restarted
        again = _detect(m)
        assert _flat([(f, {k: v for k, v in i.items()}) for f, i in again]) == _flat([(f, i) for f, i in plain[tag]])
        m._cache = None
        assert all(np.array_equal(before[f], x) for f, x in m.arrays().items())   # the map is read, not changed
        m.close()
    # the descriptors, observations and so the candidates and matches of the three worlds are the same: only the geometry tells them apart
    assert _flat([i["accepted"]["match_point"] for _, i in plain["plain"][-1:]]) == _flat([i["accepted"]["match_point"] for _, i in plain["scrambled"][-1:]])
    voc.close(); c.close()
