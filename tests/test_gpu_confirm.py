"""LocalMapper.confirm_loop (mo_map_loop_confirm) on the device against its numpy restatement (tests/confirm_restatement.py) and the host
replay of its refit (tests/native/confirm_replay.cpp) on the constructed cases of tests/confirm_cases.py, and
detect_loop(sim3=True, confirm=True) on the loop worlds.  Every integer the call returns must be equal; the models are held to REFINE_TOL,
the project's bound for a device refinement against its restatement (libm's exp / sin / cos differ)."""
import ctypes as C
import shutil
import time

import numpy as np
import pytest

from tests import confirm_cases as CC
from tests import confirm_worlds as CW
from tests import sim3_cases as SC
from tests.test_gpu_map_reads import REFINE_TOL

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("g++") is None, reason="needs a host C++ compiler")]

CASES = {c.name: c for c in CC.all_cases()}
STAGES = ["confirm_prep", "confirm_seed", "confirm_guided", "confirm_pairs", "confirm_refit", "confirm_win", "confirm_proj", "confirm_claim"]


@pytest.fixture(scope="module")
def evaluate(tmp_path_factory):
    d = tmp_path_factory.mktemp("confirm_replay")
    exe = CC.build_replay(d)
    done = {}

    def get(case):
        if case.name not in done:
            done[case.name] = CC.evaluate(exe, case, d)
        return done[case.name]
    return get


@pytest.fixture(scope="module")
def ctx():
    import vslam_amd as V
    c = V.Context(device=0, max_w=640, max_h=480, max_batch=1)
    yield c
    c.close()


def _model(c):
    return np.concatenate([[c["scale"]], c["R"].reshape(9), c["t"]])


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_the_restatement_and_the_replay(name, evaluate, ctx):
    """Noise-free refits also against the constructed truth, within CC.TRUTH_BOUND: ten times the replay's largest measured error
    (tests/confirm_cases.py lists the measurements)."""
    case = CASES[name]
    fr, rp, bk = ev = evaluate(case)
    CC.check(case, ev)   # the case's conditions, before any device is asked
    t0 = time.perf_counter()
    m = case.build_map(ctx)
    t1 = time.perf_counter()
    ok, info = case.call(m)
    t2 = time.perf_counter()
    nc, n_p = len(case.cand), len(case.kf[case.p]["xy"])
    res = info["candidates"]
    assert len(res) == nc and [c["pos"] for c in res] == case.cand and info["kf_pos"] == case.p
    worst, worst_truth = 0.0, 0.0
    for c in range(nc):
        n2 = len(case.kf[case.cand[c]]["xy"])
        assert res[c]["fwd"].shape == (n_p,) and np.array_equal(res[c]["fwd"], fr["fwd"][c]), (name, c, np.flatnonzero(res[c]["fwd"] != fr["fwd"][c]))
        assert res[c]["bwd"].shape == (n2,) and np.array_equal(res[c]["bwd"], fr["bwd"][c][:n2]), (name, c)
        assert (res[c]["n_pairs"], res[c]["n_guided"], res[c]["n_inliers"]) == (fr["n_pairs"][c], fr["n_guided"][c], rp["ninl"][c]), (name, c)
        assert res[c]["inlier"].shape == (n_p,) and np.array_equal(res[c]["inlier"], bk["pair_inlier"][c]), (name, c)
        got = _model(res[c])
        if not fr["part"][c]:
            assert np.isnan(got).all()
        elif fr["n_pairs"][c] < 3:
            assert np.array_equal(got, rp["model"][c])   # the model as given
        else:
            assert np.allclose(got, rp["model"][c], **REFINE_TOL), (name, c, got - rp["model"][c])
            worst = max(worst, np.abs(got - rp["model"][c]).max())
        if case.truth[c] is not None:
            e = np.abs(got - SC.model_of(case.truth[c])).max()
            assert e < CC.TRUTH_BOUND, (name, c, e)
            worst_truth = max(worst_truth, e)
    assert info["win"] == bk["win"] and ok == bk["ok"]
    assert info["n_inliers"] == (rp["ninl"][bk["win"]] if bk["win"] >= 0 else 0)
    assert np.array_equal(info["loop_point"], bk["loop_point"]) and np.array_equal(info["source"], bk["source"]), name
    assert (info["n_loop_points"], info["n_proj_cand"], info["n_proj"], info["n_total"]) == (bk["n_loop_points"], bk["n_proj_cand"], bk["n_proj"], bk["n_total"])
    if info["win"] >= 0:
        w = res[info["win"]]
        S = np.eye(4)
        S[:3, :3], S[:3, 3] = w["scale"] * w["R"], w["t"]
        assert np.allclose(info["world"], np.linalg.inv(case.kf[case.p]["pose"]) @ S @ case.kf[w["pos"]]["pose"], rtol=1e-12, atol=1e-12)
    else:
        assert info["world"] is None
    m.close()
    print("%s: largest model difference to the replay %.3g, to the truth %.3g (bound %.3g); map %.3f s, call %.3f s"
          % (name, worst, worst_truth, CC.TRUTH_BOUND, t1 - t0, t2 - t1))


def test_two_calls_give_equal_bytes(ctx):
    from tests.test_gpu_scratch_poison import _flat
    for name in ("candidates:16", "projection_rules", "loop_points:1100"):
        case = CASES[name]
        m = case.build_map(ctx)
        a = _flat(case.call(m))
        other = _flat(case.call(m, radius_guided=3.0, radius_proj=4.0, max_dist=20))   # another call in between leaves its own scratch behind
        assert _flat(case.call(m)) == a and [p for p, _ in other] == [p for p, _ in a]
        m.close()


def test_stage_names(ctx):
    case = CASES["total:40"]
    m = case.build_map(ctx)
    ctx.set_host_timing(True)
    ok, _ = case.call(m)
    names = [n for n, _ in ctx.stage_times()]
    ctx.set_host_timing(False)
    m.close()
    assert ok and names == STAGES


def _raw(m, case, K="case", poses="case", prm=True, out=True, null=(), **over):
    """mo_map_loop_confirm called directly with every output array NULL: (rc, MapConfirmOut)"""
    import vslam_amd as V
    case.inputs()
    n_kf = case.n_kf()
    Ka = np.ascontiguousarray(CC.K, np.float64).reshape(9) if isinstance(K, str) else K
    Pa = np.ascontiguousarray(np.stack([k["pose"][:3, :4] for k in case.kf]), np.float64).reshape(n_kf, 12) if isinstance(poses, str) else poses
    cur, mpt, mrow, fl = case.lists()
    cand = np.array(over.pop("cand", case.cand), np.int32)
    s = np.array([mm[0] for mm in case.models], np.float64)
    R = np.ascontiguousarray([mm[1].reshape(9) for mm in case.models], np.float64)
    t = np.ascontiguousarray([mm[2] for mm in case.models], np.float64)
    g = case.group_mask()
    f = dict(kf_pos=case.p, n_cand=len(case.cand), w=CC.W_IMG, h=CC.H_IMG, max_dist=50, min_inliers=3, min_matches=40, radius_guided=7.5, radius_proj=10.0,
             chi2=SC.CHI2, scale_factor=SC.SF)
    f.update(over)
    ptr = {"cand": cand, "cur_point": cur, "match_point": mpt, "match_row": mrow, "inlier": fl, "scale": s, "R": R, "t": t, "group": g}
    a = {k: (None if k in null or v is None else v.ctypes.data) for k, v in ptr.items()}
    p = V.MapConfirmParams(f["kf_pos"], f["n_cand"], a["cand"], a["cur_point"], a["match_point"], a["match_row"], a["inlier"], a["scale"], a["R"], a["t"],
                           a["group"], f["w"], f["h"], f["max_dist"], f["min_inliers"], f["min_matches"], f["radius_guided"], f["radius_proj"], f["chi2"],
                           f["scale_factor"])
    o = V.MapConfirmOut()   # every output array NULL
    o.win, o.ok, o.win_inliers, o.n_loop_points, o.n_proj_cand, o.n_proj, o.n_total = 5, 5, 5, 5, 5, 5, 5
    rc = m.lib.mo_map_loop_confirm(m._h, V._ptr(Ka) if Ka is not None else None, V._ptr(Pa) if Pa is not None else None, C.byref(p) if prm else None,
                                   C.byref(o) if out else None)
    return rc, o


def _scalars(o):
    return (o.win, o.ok, o.win_inliers, o.n_loop_points, o.n_proj_cand, o.n_proj, o.n_total)


def test_errors_and_empties(ctx):
    import vslam_amd as V
    from vslam_amd.mapper import LocalMapper
    case = CASES["total:40"]
    m = case.build_map(ctx)
    n_kf = case.n_kf()
    nan_K = np.ascontiguousarray(CC.K, np.float64).reshape(9).copy(); nan_K[4] = np.nan
    inf_P = np.stack([k["pose"][:3, :4] for k in case.kf]).reshape(n_kf, 12).copy(); inf_P[1, 3] = np.inf
    nan, inf = float("nan"), float("inf")
    for bad in (dict(K=None), dict(poses=None), dict(prm=False), dict(out=False), dict(K=nan_K), dict(poses=inf_P), dict(kf_pos=n_kf), dict(kf_pos=-1),
                dict(cand=[n_kf]), dict(cand=[-1]), dict(n_cand=17), dict(n_cand=-1), dict(chi2=nan), dict(chi2=-1.0), dict(chi2=inf), dict(scale_factor=0.0),
                dict(scale_factor=nan), dict(w=0), dict(h=0), dict(radius_guided=0.0), dict(radius_guided=inf), dict(radius_proj=-1.0), dict(radius_proj=nan),
                dict(max_dist=-1), dict(max_dist=257), dict(min_inliers=-1), dict(min_matches=-1), dict(null=("cand",)), dict(null=("cur_point",)),
                dict(null=("match_point",)), dict(null=("match_row",)), dict(null=("scale",)), dict(null=("R",)), dict(null=("t",))):
        assert _raw(m, case, **bad)[0] == V.MO_ERR_ARG, bad
    assert _raw(m, case, kf_pos=n_kf, n_cand=0)[0] == V.MO_ERR_ARG              # kf_pos is checked before the empty list returns
    rc, o = _raw(m, case, n_cand=0, null=("cand", "cur_point", "match_point", "match_row", "scale", "R", "t", "inlier", "group"))
    assert rc == V.MO_OK and _scalars(o) == (-1, 0, 0, 0, 0, 0, 0)
    rc, o = _raw(m, case, max_dist=0, chi2=0.0)                                  # the ends of the ranges are legal: nothing is an inlier
    assert rc == V.MO_OK and _scalars(o) == (-1, 0, 0, 0, 0, 0, 0)
    rc, o = _raw(m, case, max_dist=256)
    assert rc == V.MO_OK and o.win == 0
    rc, o = _raw(m, case)                                                        # every output array NULL: legal
    assert rc == V.MO_OK and _scalars(o) == (0, 1, 30, 40, 10, 10, 40)
    rc, o = _raw(m, case, null=("inlier",))                                      # NULL flags: every listed row a seed, as the flags say here
    assert rc == V.MO_OK and _scalars(o) == (0, 1, 30, 40, 10, 10, 40)
    rc, o = _raw(m, case, null=("group",))                                       # NULL group: the candidate alone, the neighbour's ten points are no loop points
    assert rc == V.MO_OK and _scalars(o) == (0, 0, 30, 30, 0, 0, 30)
    rc, o = _raw(m, case, min_matches=41)
    assert rc == V.MO_OK and _scalars(o) == (0, 0, 30, 40, 10, 10, 40)
    empty = LocalMapper(CC.K, save_every_keyframe=False, context=ctx)
    rc, o = _raw(empty, case, poses=np.zeros((1, 12)))
    assert rc == V.MO_OK and _scalars(o) == (-1, 0, 0, 0, 0, 0, 0)
    ok, info = empty.confirm_loop([], [])
    assert not ok and info["win"] == -1 and info["candidates"] == [] and info["world"] is None and info["n_total"] == 0
    with pytest.raises(ValueError):
        m.detect_loop(confirm=True)
    with pytest.raises(ValueError):
        m.confirm_loop(case.candidates(), [])
    m.close(); empty.close()


def test_poison():
    """the call under the poison bytes 255, 0 and 90 returns the bytes it returns without, the fill totals grow, the maps keep theirs"""
    from tests.test_gpu_scratch_poison import _ctx, _read_sweep
    ctx = _ctx()
    cases = [CASES[n] for n in ("candidates:16", "projection_rules", "stale_observations", "takes_no_part")]
    maps = [c.build_map(ctx) for c in cases]
    calls = [(c.name, lambda c=c, m=m: c.call(m)) for c, m in zip(cases, maps)]
    assert calls[0][1]()[1]["win"] == 5 and calls[1][1]()[1]["n_proj"] == 3   # the reads find what they look for: nothing below compares empty results
    _read_sweep(ctx, maps, calls)
    for m in maps:
        m.close()
    ctx.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
FACTOR = 1.3


def _detect(m, **kw):
    from tests import loop_worlds as LW
    m._loop_consistency = None
    return [m.detect_loop(p, **kw) for p in LW.RETURN_POS]


def test_detect_loop_with_confirmation_on_the_loop_worlds():
    """The loop world plain, with its return side rescaled by 1.3, and scrambled (tests/test_gpu_sim3.py's worlds), and the look-alike world
    of tests/confirm_worlds.py plain and rescaled.  At position 26 the loop is confirmed on all but the scrambled one with at least 40 loop
    points, more than the alignment had inliers, every one of them true; some are projected.  The plain loop world has no guided match to
    find - its ratio test refuses no true match, tests/test_confirm_cpu.py states the restatement's counts (75 seeds, 0 guided, 12
    projected) - so n_guided > 0 is asked of the look-alike world (57, 18, 12).  Bound on the scale: SC.TRUTH_BOUND, the alignment test's."""
    import vslam_amd as V
    from tests import loop_worlds as LW
    from tests.test_gpu_scratch_poison import _flat
    from tests.test_gpu_sim3 import _rescaled
    c = V.Context(device=0, max_w=640, max_h=480, max_batch=1)
    base, alike = LW.loop_world(), CW.look_alike_world()
    words, weights = LW.loop_vocabulary()
    voc = V.Vocabulary.from_arrays(words, weights, context=c)
    worlds = {"plain": (base, 1.0), "rescaled": (_rescaled(base, FACTOR), FACTOR), "scrambled": (_rescaled(base, FACTOR, np.random.default_rng(3)), None),
              "alike": (alike, 1.0), "alike rescaled": (_rescaled(alike, FACTOR), FACTOR)}
    for tag, (w, want) in worlds.items():
        m = w.build(c)
        m.set_vocabulary(voc)
        before = {f: x.copy() for f, x in m.arrays().items()}
        plain = _detect(m)
        aligned = _detect(m, sim3=True, seed=11)
        got = _detect(m, sim3=True, confirm=True, seed=11)
        found, info = got[-1]
        if want is None:
            assert [f for f, _ in got] == [False] * 4 and info["accepted"] is None
            assert not any("confirm_ok" in x for x in info["candidates"])   # nothing aligned: nothing to confirm
        else:
            assert [f for f, _ in got] == [p == 26 for p in LW.RETURN_POS], tag
            a, al = info["accepted"], aligned[-1][1]["accepted"]
            cf = a["confirm"]
            assert a["pos"] == al["pos"] == 3 and a["sim3_ok"] and a["confirm_ok"] and cf["win"] == 0
            r = cf["candidates"][0]
            by = [int((cf["source"] == k).sum()) for k in (1, 2, 3)]
            print("%s: %d loop points (%d seeds, %d guided, %d projected of %d candidates, %d loop points in the group); alignment %d inliers of %d; "
                  "scale %.9g -> %.9g (want %g)" % (tag, cf["n_total"], by[0], by[1], by[2], cf["n_proj_cand"], cf["n_loop_points"], a["sim3"]["n_inliers"],
                                                    a["sim3"]["n_corr"], a["sim3"]["scale"], r["scale"], want))
            assert cf["n_total"] >= 40 and cf["n_total"] > a["sim3"]["n_inliers"] and cf["n_proj"] > 0 and cf["n_total"] == sum(by)
            assert by[1] == int(r["inlier"].sum()) - by[0] <= r["n_guided"] and by[2] == cf["n_proj"]
            if tag.startswith("alike"):
                assert r["n_guided"] > 0 and by[1] > 0
            assert CW.true_loop_point(w, 26, a["cur_point"], w.kf_xy[26], cf["loop_point"], factor=want) == []
            assert abs(r["scale"] - want) < SC.TRUTH_BOUND
            X = np.array([1.0, 0.5, 8.0, 1.0])
            assert np.abs(cf["world"] @ X - np.append(want * X[:3], 1.0)).max() < 1e-3
        # without the keyword: what the calls returned before
        assert _flat([(f, i) for f, i in _detect(m)]) == _flat([(f, i) for f, i in plain])
        assert _flat([(f, i) for f, i in _detect(m, sim3=True, seed=11)]) == _flat([(f, i) for f, i in aligned])
        m._cache = None
        assert all(np.array_equal(before[f], x) for f, x in m.arrays().items())   # the map is read, not changed
        m.close()
    voc.close(); c.close()
