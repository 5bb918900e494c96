"""The essential-graph optimisation without a device: the geometry of visual-slam_amd/csrc/posegraph.h as a host build
(tests/native/posegraph_check.cpp), the edge rules in numpy (tests/posegraph_restatement.py) on constructed weights, the cases of
tests/posegraph_cases.py on the host replay of the whole call (tests/native/posegraph_replay.cpp, plain and with its libm results
nudged), and the boundary (mo_map_pose_graph, its structs, detect_loop's keyword)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import posegraph_cases as PC
from tests import posegraph_restatement as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = {c.name: c for c in PC.exact_cases()}
DRIFT = {c.name: c for c in PC.drift_cases()}
EDGES = {c.name: c for c in PC.edge_cases()}


@pytest.fixture(scope="module")
def replays(tmp_path_factory):
    d = tmp_path_factory.mktemp("posegraph_replay")
    return PC.build_replays(d) + (d,)


# ---- posegraph.h ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [(), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "sanitized"])
def test_residual_jacobians_and_blocks_on_the_host(flags, tmp_path):
    exe = PC.build_native(tmp_path, "posegraph_check", flags=flags)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    assert "3.14159165" in out.stdout and "rotation 1e-09" in out.stdout and "rotation 0:" in out.stdout   # the three angles that are asked for


# ---- rule 1 ---------------------------------------------------------------------------------------------------------------------------------
def _pairs(case):
    a, b, k = case.edges()
    return list(zip(a.tolist(), b.tolist(), k.tolist()))


def test_edge_rules_on_constructed_weights():
    E, T, V = PR.EXTRA, PR.TREE, PR.COVIS
    # all-zero weights: a pure chain
    c = EDGES["edges:chain"]
    assert not c.weights().any() and _pairs(c) == [(i, i + 1, T) for i in range(8)]
    # a weight exactly at min_weight is an edge, one below is not; a pair with any weight is the parent's
    c = EDGES["edges:thresholds"]
    W = c.weights()
    assert (W[0, 4], W[1, 5], W[2, 7], W[3, 9]) == (3, 2, 4, 1) and c.min_weight == 3
    par = PR.parents(W)
    assert par.tolist() == [-1, 0, 1, 2, 0, 1, 5, 2, 7, 3]
    got = _pairs(c)
    assert (0, 4, T) in got and (1, 5, T) in got and (2, 7, T) in got and (3, 9, T) in got and (3, 4, T) not in got
    assert len(got) == 9 and all(k == T for _, _, k in got)   # (every weighted pair is its upper end's parent here: no covisibility edge is left)
    # ties: the lowest position of the largest weight
    c = EDGES["edges:ties"]
    par = PR.parents(c.weights())
    assert par[6] == 1 and par[7] == 0 and par[3] == 2
    got = _pairs(c)
    assert (3, 6, T) not in got and (3, 6, V) not in got and (2, 3, T) in got   # (weight 2 < 4: the tie's loser is no edge)
    # a pair that is both extra and heavy appears once, as an extra edge; given twice and reversed
    c = EDGES["edges:extra_and_heavy"]
    got = _pairs(c)
    assert [g for g in got if g[:2] == (1, 6)] == [(1, 6, E)] and (2, 7, E) in got and (2, 5, T) in got
    assert (5, 6, T) not in got   # (6's parent is 1: that pair is the extra one)
    assert got == sorted(got) and len({g[:2] for g in got}) == len(got)
    # pairs of two fixed positions are dropped, extra or not; an extra edge with one free end stays
    c = EDGES["edges:extra_between_fixed"]
    got = _pairs(c)
    assert not [g for g in got if g[:2] in ((0, 5), (0, 1))] and (1, 7, E) in got and (1, 3, T) in got
    # stale and repeated observations count as the library reads them
    c = EDGES["edges:stale_observations"]
    assert c.weights()[1, 5] == 3 and c.weights()[1, 1] == 3 and PR.parents(c.weights())[5] == 1
    # a weight matrix by hand, no map: min_weight below 1 counts as 1
    W = np.zeros((4, 4), np.int32)
    W[0, 3] = W[3, 0] = 1
    a, b, k = PR.edges(W, [], [1, 0, 0, 0], 0)
    assert list(zip(a.tolist(), b.tolist(), k.tolist())) == [(0, 1, T), (0, 3, T), (1, 2, T)]


def test_the_cases_cover_the_shapes():
    assert [c.n_kf for c in EXACT.values()] == [2, 3, 12, 70, 150] and [c.n_kf for c in DRIFT.values()] == [12, 70]
    assert EXACT["exact:12"].extra == [(0, 11)] and (0, 11, PR.EXTRA) in _pairs(EXACT["exact:12"])
    assert 7 * 149 > 1024 and PR.COVIS in EXACT["exact:150"].edges()[2]
    assert len(_pairs(EXACT["exact:2"])) == 1
    for c in DRIFT.values():
        assert PR.EXTRA in c.edges()[2] and PR.COVIS in c.edges()[2]


# ---- the replay -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(EXACT))
def test_exact_cases_reach_the_truth_on_the_replay(name, replays):
    plain, _, d = replays
    case = EXACT[name]
    r = PC.run_replay(plain, case, d)
    e0, e1 = PC.truth_error(case, case.init), PC.truth_error(case, r["sim3"])
    print("%s: %d edges, %d steps (%d accepted), %d cg iterations, cost %.3g -> %.3g, error to the truth %.3g -> %.3g (TRUTH_REPLAY %.3g)"
          % (name, len(case.edges()[0]), r["steps"], r["accepted"], r["cg_iters"], r["cost"][0], r["cost"][1], e0, e1, PC.TRUTH_REPLAY))
    assert e0 > 1e-3 and e1 <= PC.TRUTH_REPLAY and r["cost"][1] < 1e-20 * r["cost"][0] and r["accepted"] >= 3
    assert r["sim3"][0].tobytes() == case.init[0].tobytes()


@pytest.mark.parametrize("name", list(DRIFT))
def test_drift_cases_on_the_replay(name, replays):
    plain, nudged, d = replays
    case = DRIFT[name]
    a, b = PC.run_replay(plain, case, d), PC.run_replay(nudged, case, d)
    sp = PC.spread(case, a["sim3"], b["sim3"])
    r0, r1 = PC.consecutive_residual(case, case.init), PC.consecutive_residual(case, a["sim3"])
    print("%s: %d steps (%d accepted), cost %.6g -> %.6g, largest consecutive residual %.3g -> %.3g, spread of the two builds %.3g (recorded %.3g), decisive %s"
          % (name, a["steps"], a["accepted"], a["cost"][0], a["cost"][1], r0, r1, sp, PC.LIBM_SPREAD[name], PC.decisive(a, b)))
    assert a["cost"][1] < a["cost"][0] and a["accepted"] > 0
    assert a["sim3"][0].tobytes() == case.init[0].tobytes()
    assert r1 < r0
    assert 0 < sp <= PC.LIBM_SPREAD[name]
    assert PC.decisive(a, b)   # (the device's steps and accepted are compared on decisive cases only: these two must be)


def test_no_free_vertex_and_no_step_on_the_replay(replays):
    plain, _, d = replays
    case = PC.drift(12, 21, max_steps=0)
    r = PC.run_replay(plain, case, d)
    assert r["steps"] == 0 and r["sim3"].tobytes() == case.init.tobytes()


# ---- the boundary -----------------------------------------------------------------------------------------------------------------------------
def test_symbols_signatures_and_abi_version():
    import vslam_amd as V
    lib = V.load_library()
    hdr = open(os.path.join(ROOT, "include", "vslam_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert hasattr(lib, "mo_map_pose_graph") and "mo_map_pose_graph" in V.SIGNATURES and re.search(r"\bmo_map_pose_graph\s*\(", hdr)
    assert len(V.SIGNATURES["mo_map_pose_graph"][1]) == 5
    assert lib.mo_abi_version() == 7 == V.ABI_VERSION


def test_struct_layouts_match_the_header(tmp_path):
    """sizeof / offsetof of the two new structs as a C compiler sees include/vslam_amd.h == the ctypes mirror"""
    import vslam_amd as V
    structs = [("mo_map_pg_params", V.MapPgParams), ("mo_map_pg_out", V.MapPgOut)]
    body = ""
    for cname, cls in structs:
        body += '  printf("%%zu\\n", sizeof(%s));\n' % cname
        body += "".join('  printf("%%zu\\n", offsetof(%s, %s));\n' % (cname, f[0].rstrip("_")) for f in cls._fields_)
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
    assert [f[0] for f in V.MapPgParams._fields_][:4] == ["fixed", "extra_a", "extra_b", "n_extra"]


def test_detect_loop_refuses_optimize_without_correct():
    """the keyword is checked before anything is asked of the map"""
    from vslam_amd.mapper import LocalMapper
    for kw in (dict(optimize=True), dict(optimize=True, sim3=True, confirm=True)):
        m = LocalMapper.__new__(LocalMapper)   # (no context, no map: the call must not get as far as needing one)
        with pytest.raises(ValueError):
            m.detect_loop(**kw)
