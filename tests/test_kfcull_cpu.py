"""The keyframe cull's restatement (tests/kfcull_restatement.py) and the constructed worlds (tests/kfcull_worlds.py), without a GPU: every
world decides what it was built to decide, the variant it is there to exclude decides differently, the restatement gives the numbers of
an independent prototype on the existing worlds, and the erase leaves the map that never had the keyframes."""
import os

import numpy as np
import pytest

from tests import kfcull_restatement as KR
from tests import kfcull_worlds as KW
from tests.covis_restatement import covisibility as covis_restated
from tests.map_worlds import world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(KW.CASES))
def test_world_decides_what_it_was_built_for(name):
    _, _, switch, want = KW.CASES[name]
    w, kw = KW.case(name)
    r = KW.decide(w, **kw)
    assert len(w.counts) <= 12 or name == "many"
    assert len(w.obs) <= 2000
    if want is not None:
        assert r["removed_positions"] == want
    if switch:
        v = KW.decide(w, **kw, **KW.SWITCH[switch])
        assert v["removed_positions"] != r["removed_positions"], switch
    p = (len(w.counts) - 1) if kw.get("kf_pos", -1) < 0 else kw["kf_pos"]
    assert p not in r["pos"] and len(set(r["pos"])) == len(r["pos"])
    assert all(a >= b for a, b in zip(r["weight"], r["weight"][1:]))


def test_what_the_worlds_are_made_of():
    """the properties the cases' names promise"""
    w, kw = KW.case("mutual")
    r = KW.decide(w, **kw)
    assert r["weight"][1] == r["weight"][2] and r["pos"][1:] == [3, 2]           # equal weights, the later position first
    assert KW.decide(w, one_pass=True)["removed_positions"] == [2, 3]             # a one-pass evaluation removes both
    for n, n_red in (("threshold_15", 15), ("threshold_16", 16)):
        w, kw = KW.case(n)
        r = KW.decide(w, **kw)
        k = r["pos"].index(2)
        assert (r["n_points"][k], r["n_redundant"][k]) == (20, n_red) and kw["ratio"] == 0.75
    w, kw = KW.case("position_0")
    r = KW.decide(w, **kw)
    k = r["pos"].index(0)
    assert r["n_redundant"][k] == r["n_points"][k] == 40 and not r["removed"][k]
    w, kw = KW.case("protect")
    r = KW.decide(w, **kw)
    k = r["pos"].index(2)
    assert r["n_redundant"][k] == r["n_points"][k] and not r["removed"][k] and KW.decide(w)["removed_positions"] == [2]
    w, _ = KW.case("duplicate")
    assert any(k < 0 for o in w.obs for k in o) and max(np.bincount([k % 6 for k in w.obs[0]])) == 2
    w, _ = KW.case("negative_keys")
    assert (w.obs_kf < 0).sum() > 50 and (w.obs_kp < 0).sum() > 50
    w, _ = KW.case("nothing_named")
    valid = KR.valid_observations(w.obs_off, w.obs_kf, w.obs_kp, w.counts)
    assert len(valid[0]) == 3 and len(w.obs[0]) == 7
    w, _ = KW.case("negative_octaves")
    assert min(int(o.min()) for o in w.kf_oct) == -3
    w, _ = KW.case("earlier_removals")
    assert w.survivors != list(range(len(w.survivors)))
    w, _ = KW.case("tall")
    assert w.counts.max() > 1024 and len(w.counts) == 12
    w, kw = KW.case("many")
    r = KW.decide(w, **kw)
    assert len(w.counts) == 130 and (w.counts == 8).all() and len(r["pos"]) > 64 and 0 < len(r["removed_positions"]) < len(r["pos"])
    assert len(set(r["weight"])) < len(r["weight"])


@pytest.mark.parametrize("name", KW.EXISTING)
def test_restatement_on_the_existing_worlds(name):
    """the numbers of a prototype written apart from this restatement (first valid observation per keyframe, negative octaves as 0)"""
    w = world(name)
    pos, weight, n_points, n_red, n_red_noscale = KW.EXISTING_NUMBERS[name]
    r = KW.decide(w)
    assert (r["pos"], r["weight"], r["n_points"], r["n_redundant"]) == (pos, weight, n_points, n_red)
    assert r["removed_positions"] == []
    if n_red_noscale is not None:
        assert KW.decide(w, scale_test=False)["n_redundant"] == n_red_noscale
    # the weights are the device matrix's (its restatement), n_points its diagonal
    W = covis_restated(w.obs_off, w.obs_kf, w.obs_kp, w.counts)
    assert [int(W[-1, q]) for q in pos] == weight and [int(W[q, q]) for q in pos] == n_points


@pytest.mark.parametrize("name", ["ba_stale", "ba", "negative_keys", "duplicate", "nothing_named"])
def test_erase_leaves_the_map_without_the_keyframes(name):
    w, _ = KW.any_world(name)
    n_kf = len(w.counts)
    gone = [2, n_kf - 2]
    off, okf, okp, counts = KR.erase(w.obs_off, w.obs_kf, w.obs_kp, w.counts, gone)
    assert len(off) == len(w.obs_off) and len(counts) == n_kf - 2
    assert (okf >= 0).all() and (okf < n_kf - 2).all() and (okp >= 0).all() and (okp < counts[okf]).all()
    keep = [q for q in range(n_kf) if q not in gone]
    W0 = covis_restated(w.obs_off, w.obs_kf, w.obs_kp, w.counts)
    assert np.array_equal(covis_restated(off, okf, okp, counts), W0[np.ix_(keep, keep)])
    # erasing nothing normalises the keys and drops what names nothing; doing it twice changes nothing more
    o1 = KR.erase(w.obs_off, w.obs_kf, w.obs_kp, w.counts, [])
    o2 = KR.erase(*o1, [])
    assert all(np.array_equal(a, b) for a, b in zip(o1, o2))
    # the decision on the erased map only loses the erased keyframes' votes: every surviving point keeps its other observers
    oct2 = [w.kf_oct[q] for q in keep]
    r = KR.decide(off, okf, okp, counts, oct2)
    assert set(r["pos"]) <= set(range(n_kf - 2))


def test_new_structs_match_the_header(tmp_path):
    """the method of tests/test_cabi_cpu.py on mo_map_kfcull_params / mo_map_kfcull_out"""
    import ctypes as C
    import subprocess
    import vslam_amd as V
    structs = [("mo_map_kfcull_params", V.MapKfCullParams), ("mo_map_kfcull_out", V.MapKfCullOut)]
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


def test_abi_version_and_symbols():
    import vslam_amd as V
    lib = V.load_library()
    assert lib.mo_abi_version() == 7 == V.ABI_VERSION
    for name in ("mo_map_kf_redundancy", "mo_map_erase_keyframes", "mo_map_cull_keyframes"):
        assert hasattr(lib, name) and name in V.SIGNATURES
