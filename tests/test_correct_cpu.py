"""The loop correction without a device: every constructed case of tests/correct_cases.py on the numpy restatement
(tests/correct_restatement.py), the loop worlds the device tests run end to end, and the boundary (mo_map_loop_correct, its structs)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import correct_cases as CC
from tests import correct_restatement as CR
from tests import correct_worlds as CW
from tests import loop_worlds as LW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {c.name: c for c in CC.all_cases()}
# corrected poses (f64) and surviving moved points (f32) of the constructed cases against their true worlds, on the restatement: 1.7e-7
# (empty_group, the one case whose duplicates survive; the poses alone: 4.8e-16)
TRUTH_CASES = 2e-7


@pytest.mark.parametrize("name", list(CASES))
def test_case_meets_its_conditions_on_the_restatement(name):
    case = CASES[name]
    res = CC.check(case)
    err = CC.truth_error(case, res)
    print("%s: %s; margin %.3g; error to the true world %.3g" % (name, res["counts"], res["margins"]["min"], err))
    assert err < TRUTH_CASES
    # the transform is the drift undone: scale 1 / f, and the corrected poses are rigid
    assert abs(res["A_scale"] * case.f - 1.0) < 1e-15
    for k in np.flatnonzero(case.masks()[0]):
        R = res["poses_out"][k][:, :3]
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14


def test_the_cases_cover_every_family():
    assert CC.FAMILIES - {"errors"} <= {c.family for c in CASES.values()} and len(CC.error_calls(8)) >= 10
    assert {len(CASES["points:%d" % n].xyz) for n in (255, 256, 257)} == {255, 256, 257}
    assert {len(CASES["rows:%d" % n].finish().kf[CASES["rows:%d" % n].p]["xy"]) for n in (63, 64, 65, 1025)} == {63, 64, 65, 1025}
    for n in (63, 64, 65, 1025):
        c = CASES["rows:%d" % n]
        assert c.loop_point()[n - 1] >= 0   # the last row is listed
    assert CASES["corrected:alone"].masks()[0].sum() == 1
    sc = np.flatnonzero(CASES["corrected:scattered"].masks()[0])
    assert len(sc) == 4 and (np.diff(sc) >= 2).all() and sc[-1] == CASES["corrected:scattered"].p
    assert CASES["corrected:with_zero"].masks()[0][0] == 1
    assert CASES["empty_group"].masks()[1].sum() == 0
    assert CASES["loop_point:null"].loop_point() is None
    o = CASES["loop_point:out_of_range"]
    lp = o.loop_point()
    assert (lp >= len(o.xyz)).sum() >= 2 and (lp < -1).any() and (lp == 2 ** 31 - 1).any()
    t = CASES["loop_point:two_rows_one_L"].loop_point()
    assert max(np.bincount(t[t >= 0])) == 2
    s = CASES["stale_observations"]
    n_kf = len(s.kf)
    assert any(k >= n_kf for ob in s.obs for k, _ in ob) and any(k < -n_kf for ob in s.obs for k, _ in ob) and any(r < 0 for ob in s.obs for _, r in ob)
    assert any(-n_kf <= k < 0 for ob in s.obs for k, _ in ob)
    assert {CASES["scale:rigid"].f, CASES["scale:1.3"].f, CASES["scale:0.5"].f} == {1.0, 1.3, 0.5}
    assert np.array_equal(CASES["scale:rigid"].R_D, np.eye(3))


def test_the_survivor_and_gain_cases_tell_the_rules_apart():
    """the inputs decide otherwise under the neighbouring rule: by observations alone the duplicates would survive their loop points; a
    gain per naming row would put the loop point at p twice"""
    from tests.fuse_restatement import lists_of
    case = CASES["direct:edge_fewer_obs"]
    res = CC.check(case)
    # (by observations alone the duplicates, with four observations against one, would survive)
    assert all(len(case.obs[fe["o"]]) > len(case.obs[fe["L"]]) and res["survivor"][fe["o"]] == fe["L"] for fe in case.f_dup)
    case = CASES["loop_point:two_rows_one_L"]
    res = CC.check(case)
    fe = case.f_free[0]
    assert sum(1 for k, _ in lists_of(res["arrays"])[res["into"][fe["L"]]] if k == case.p) == 1


def test_transform_on_hand_values():
    """rule 1 and rule 2 on a model whose answer is known: candidate and p at the same true pose, drift = a scale of 2 about the origin"""
    T = np.eye(4)
    T[:3, 3] = [1.0, 2.0, 3.0]
    Tp = T.copy()
    Tp[:3, 3] *= 2.0
    A, inv, RA, tA = CR.transform([T, Tp], 1, 0, 2.0, np.eye(3), np.zeros(3))
    assert inv == 0.5 and np.array_equal(A, np.hstack([0.5 * np.eye(3), np.zeros((3, 1))])) and np.array_equal(RA, np.eye(3))
    P = CR.corrected_poses([T, Tp], [1], 2.0, RA, tA)
    assert np.array_equal(P[1], T[:3, :4]) and np.array_equal(P[0], T[:3, :4])
    assert np.array_equal(CR.move(np.float32([[2.0, 4.0, -6.0]]), A), np.float32([[1.0, 2.0, -3.0]]))


def test_loop_worlds_on_the_restatement():
    """What tests/test_gpu_correct.py asks of detect_loop(..., correct=True) at position 26, on the host with the world's true similarity:
    the corrected set is exactly the return keyframes, at least 40 loop points are named, every named duplicate is absorbed into its old
    point, no old point moves, and the return side is back at the unscaled world within CW.TRUTH_RESTATED."""
    from tests.test_gpu_sim3 import _rescaled
    base = LW.loop_world()
    worst = {}
    for tag, factor in (("plain", 1.0), ("rescaled", 1.3)):
        w = base if factor == 1.0 else _rescaled(base, factor)
        r = CW.restated(w, factor)
        res = r["res"]
        assert r["confirm_ok"] and r["corrected"] == list(LW.RETURN_POS) and r["cand"] == 3 and not set(r["group"]) & set(r["corrected"])
        assert int((r["loop_point"] >= 0).sum()) >= 40 and res["fused"]
        # (no margin condition here: the device corrects with the similarity it found itself, and is asked for these facts, not for
        # this restatement's integers)
        named, wrong, old_moved, e = CW.facts(w, base, {"into": res["into"], "moved": res["moved"], "xyz": res["arrays"]["xyz"], "ids": res["arrays"]["id"],
                                                          "poses": res["poses_out"], "loop_point": r["loop_point"]})
        print(tag, res["counts"], "named duplicates", named, "error to the unscaled world %.3g" % e)
        assert named >= 40 and wrong == [] and old_moved == 0
        assert res["counts"]["n_absorbed"] >= named and res["counts"]["n_moved"] > 0
        worst[tag] = e
        assert e <= CW.TRUTH_RESTATED
    print(worst)


def test_loop_connections_read_observations_as_the_library_does():
    """vslam_amd.mapper.positions_sharing_points (correct_loop's loop_connections) against the restatement's observation reader, on the
    stale-observation case before and after its correction"""
    from tests.track_restatement import valid_observations
    from vslam_amd.mapper import positions_sharing_points
    case = CASES["stale_observations"]
    res = CC.check(case)
    counts = [len(k["xy"]) for k in case.kf]
    cpos = np.flatnonzero(case.masks()[0]).tolist()
    for a in (case.arrays(), res["arrays"]):
        obs = valid_observations(a["obs_off"], a["obs_kf"], a["obs_kp"], counts)
        want = {i: set() for i in cpos}
        for v in obs:
            pos = {k for k, _ in v}
            for i in pos & set(cpos):
                want[i] |= pos
        assert positions_sharing_points(a, counts, cpos) == want
    # the correction connected every corrected keyframe with the old side
    after = positions_sharing_points(res["arrays"], counts, cpos)
    before = positions_sharing_points(case.arrays(), counts, cpos)
    assert all(set(case.old) <= after[i] and not set(case.old) & before[i] for i in cpos)
    assert positions_sharing_points({"obs_off": np.zeros(1, np.int32), "obs_kf": np.zeros(0, np.int32), "obs_kp": np.zeros(0, np.int32)}, counts, cpos) == {i: set() for i in cpos}


def test_symbols_signatures_and_abi_version():
    import vslam_amd as V
    lib = V.load_library()
    hdr = open(os.path.join(ROOT, "include", "vslam_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert hasattr(lib, "mo_map_loop_correct") and "mo_map_loop_correct" in V.SIGNATURES and re.search(r"\bmo_map_loop_correct\s*\(", hdr)
    assert len(V.SIGNATURES["mo_map_loop_correct"][1]) == 5
    assert lib.mo_abi_version() == 7 == V.ABI_VERSION


def test_struct_layouts_match_the_header(tmp_path):
    """sizeof / offsetof of the two new structs as a C compiler sees include/vslam_amd.h == the ctypes mirror"""
    import vslam_amd as V
    structs = [("mo_map_correct_params", V.MapCorrectParams), ("mo_map_correct_out", V.MapCorrectOut)]
    body = ""
    for cname, cls in structs:
        body += '  printf("%%zu\\n", sizeof(%s));\n' % cname
        body += "".join('  printf("%%zu\\n", offsetof(%s, %s));\n' % (cname, f[0]) for f in cls._fields_)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vslam_amd.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    k = 0
    for cname, cls in structs:
        assert got[k] == C.sizeof(cls), cname
        offs = [getattr(cls, f[0]).offset for f in cls._fields_]
        assert got[k + 1:k + 1 + len(offs)] == offs, cname
        k += 1 + len(offs)
    assert [f[0] for f in V.MapCorrectParams._fields_][:8] == ["kf_pos", "cand_pos", "scale", "R", "t", "corrected", "group", "loop_point"]


def test_detect_loop_refuses_correct_without_confirm():
    """the keyword is checked before anything is asked of the map"""
    from vslam_amd.mapper import LocalMapper
    for kw in (dict(correct=True), dict(correct=True, sim3=True)):
        m = LocalMapper.__new__(LocalMapper)   # (no context, no map: the call must not get as far as needing one)
        with pytest.raises(ValueError):
            m.detect_loop(**kw)
