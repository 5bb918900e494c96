"""The loop confirmation without a device: every constructed case of tests/confirm_cases.py on the numpy restatement
(tests/confirm_restatement.py) and the host replay of the refit (tests/native/confirm_replay.cpp), the loop worlds the device tests run
end to end, and the boundary (mo_map_loop_confirm, its structs)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import confirm_cases as CC
from tests import confirm_restatement as CR
from tests import confirm_worlds as CW
from tests import loop_worlds as LW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs a host C++ compiler")
CASES = {c.name: c for c in CC.all_cases()}


@pytest.fixture(scope="module")
def evaluate(tmp_path_factory):
    d = tmp_path_factory.mktemp("confirm_replay")
    exe = CC.build_replay(d)
    return lambda case: CC.evaluate(exe, case, d)


@needs_gxx
@pytest.mark.parametrize("name", list(CASES))
def test_case_meets_its_conditions_on_the_restatement_and_the_replay(name, evaluate):
    case = CASES[name]
    fr, rp, bk = ev = evaluate(case)
    print("%s: pairs %s, guided %s, inliers %s, win %d, loop points %d, projected %d of %d, total %d; margins %.3g (guided) %.3g (refit) %.3g "
          "(projection); error to the truth %s" % (name, fr["n_pairs"], fr["n_guided"], rp["ninl"], bk["win"], bk["n_loop_points"], bk["n_proj"],
                                                   bk["n_proj_cand"], bk["n_total"], fr["margin"], rp["margin"], bk["margin"], CC.truth_error(case, rp)))
    CC.check(case, ev)
    err = CC.truth_error(case, rp)
    if err is not None:
        assert err < CC.TRUTH_REPLAY, (name, err)


def test_the_cases_cover_what_the_issue_lists():
    assert CC.FAMILIES <= {c.family for c in CASES.values()}
    rows_p = {len(c.kf[c.p]["xy"]) for c in CASES.values() if c.family == "rows"}
    assert {4, 63, 64, 65, 1025} <= rows_p
    assert len(CASES["rows:70/1025"].kf[CASES["rows:70/1025"].cand[0]]["xy"]) == 1025
    assert len(CASES["candidates:1"].cand) == 1 and len(CASES["candidates:16"].cand) == 16
    assert not np.isfinite(CASES["takes_no_part"].models[0][1]).all() and CASES["takes_no_part"].models[2][0] == 0.0
    assert CASES["null:inlier"].lists()[3] is None and CASES["null:group"].group_mask() is None
    o = CASES["guided_octaves"]
    assert {0, 3} <= set(o.kf[o.p]["oct"]) and {1, 2, 4, 5} <= set(o.kf[o.cand[0]]["oct"])
    assert {len(CASES["loop_points:%d" % n].kf[CASES["loop_points:%d" % n].nb[0][0]]["xy"]) >= max(n, 4) for n in (0, 1, 65, 1100)} == {True}
    assert CASES["total:39"].prm["min_matches"] == CASES["total:40"].prm["min_matches"] == 40
    s = CASES["stale_observations"]
    n_kf = s.n_kf()
    assert any(k >= n_kf for o in s.obs for k, _ in o) and any(k < -n_kf for o in s.obs for k, _ in o) and any(r < 0 for o in s.obs for _, r in o)
    # a descriptor flipped by k bits is k bits away, past the 32 bits of loop_worlds.near too
    from tests.reloc_cases import CODE
    from tests.reloc_restatement import hamming
    assert [int(hamming(CODE[7:8], CC.flipped(CODE[7], k)[None])[0, 0]) for k in (0, 3, 32, 50, 51)] == [0, 3, 32, 50, 51]
    assert int(hamming(CODE[7:8], CODE[8:9])[0, 0]) == 128


def test_restatement_window_and_projection_rules():
    """the searches on hand values: the box is strict, the octave gate is +-1, ties go to the lower row, forbidden rows are not visited"""
    kx, ky, ko = np.array([10.0, 17.5, 12.0, 12.0]), np.array([10.0, 10.0, 11.0, 11.0]), np.array([0, 0, 2, 1])
    desc = np.zeros((4, 32), np.uint8)
    desc[0, 0] = 3; desc[3, 0] = 3
    d = np.zeros(32, np.uint8)
    allow = np.ones(4, bool)
    assert CR.window(10.0, 10.0, 7.5, 0, kx, ky, ko, desc, d, allow)[:2] == (0, 2)          # row 1: |dx| = r is outside; row 2: octave 2; rows 0, 3 tie
    assert CR.window(10.0, 10.0, 7.5, 0, kx, ky, ko, desc, d, np.array([0, 1, 1, 1], bool))[:2] == (3, 2)
    assert CR.window(10.0, 10.0, 7.6, 0, kx, ky, ko, desc, d, allow)[:2] == (1, 0)
    assert CR.window(10.0, 10.0, 7.5, 1, kx, ky, ko, desc, d, allow)[:2] == (2, 0)
    assert CR.window(100.0, 10.0, 7.5, 0, kx, ky, ko, desc, d, allow)[0] == -1
    K = CC.K
    assert CR.project(K, np.array([0.0, 0.0, 1.0]), 640, 480)[:3] == (320.0, 240.0, True)
    assert not CR.project(K, np.array([0.0, 0.0, -1.0]), 640, 480)[2] and not CR.project(K, np.array([0.0, 0.0, 0.0]), 640, 480)[2]
    assert not CR.project(K, np.array([0.64, 0.0, 1.0]), 640, 480)[2] and CR.project(K, np.array([-0.64, 0.0, 1.0]), 640, 480)[2]   # u = 640 is outside, u = 0 inside
    s, R, t = CR.inverse((2.0, np.eye(3), np.array([1.0, 2.0, 3.0])))
    assert s == 0.5 and np.array_equal(t, [-0.5, -1.0, -1.5])


@needs_gxx
def test_loop_worlds_reach_the_counts_on_the_restatement(evaluate):
    """What tests/test_gpu_confirm.py asks of detect_loop(sim3=True, confirm=True) at position 26, on the host with the world's true
    similarity and every match a seed.  The plain loop world: 75 seeds, no guided match (the ratio test refused no true match), 12
    projected, 87 loop points.  The look-alike world: 57 seeds, 18 guided, 12 projected, 87 loop points.  Every loop point true."""
    words, weights = LW.loop_vocabulary()
    for w, want in ((LW.loop_world(), (75, 0, 12, 87)), (CW.look_alike_world(), (57, 18, 12, 87))):
        res = CW.candidates_at(w, 26, words, weights)
        assert res["cand"] == [3]
        inp = CW.inputs_at(w, res, 0, 26)
        fr = CR.front(inp)
        m = fr["n_pairs"][0]
        bk = CR.back(inp, fr, [np.ones(m, bool)], [m], inp.models)
        got = (m - fr["n_guided"][0], fr["n_guided"][0], bk["n_proj"], bk["n_total"])
        print(got, fr["margin"], bk["margin"])
        assert got == want and bk["ok"] and bk["win"] == 0
        assert fr["margin"] >= CC.MARGIN and bk["margin"] >= CC.MARGIN
        assert CW.true_loop_point(w, 26, inp.cur_point, inp.kf_xy[26], bk["loop_point"]) == []


def test_symbols_signatures_and_abi_version():
    import vslam_amd as V
    lib = V.load_library()
    hdr = open(os.path.join(ROOT, "include", "vslam_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert hasattr(lib, "mo_map_loop_confirm") and "mo_map_loop_confirm" in V.SIGNATURES and re.search(r"\bmo_map_loop_confirm\s*\(", hdr)
    assert len(V.SIGNATURES["mo_map_loop_confirm"][1]) == 5
    assert lib.mo_abi_version() == 7 == V.ABI_VERSION


def test_struct_layouts_match_the_header(tmp_path):
    """sizeof / offsetof of the two new structs as a C compiler sees include/vslam_amd.h == the ctypes mirror"""
    import vslam_amd as V
    structs = [("mo_map_confirm_params", V.MapConfirmParams), ("mo_map_confirm_out", V.MapConfirmOut)]
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
    assert [f[0] for f in V.MapConfirmParams._fields_][:11] == ["kf_pos", "n_cand", "cand", "cur_point", "match_point", "match_row", "inlier", "scale",
                                                                "R", "t", "group"]


def test_detect_loop_refuses_confirm_without_sim3():
    """the keyword is checked before anything is asked of the map"""
    from vslam_amd.mapper import LocalMapper
    m = LocalMapper.__new__(LocalMapper)   # (no context, no map: the call must not get as far as needing one)
    with pytest.raises(ValueError):
        m.detect_loop(confirm=True)
