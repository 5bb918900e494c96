"""mo_map_absorb and mo_map_loop_candidates_among without a GPU: the restatement of the absorb rules on snapshot dicts
(tests/absorb_restatement.py) puts a map built in two sessions back together, visual-slam_amd/csrc/absorb.h holds under
AddressSanitizer and UBSan (tests/native/absorb_check.cpp), the masked selection restated, and the layouts of the two new structs."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import absorb_restatement as AR
from tests import correct_worlds as CW
from tests import loop_restatement as LR
from tests import loop_worlds as LW
from tests import merge_worlds as MW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs a host C++ compiler")


# ---- the restatement on the loop world mapped in two sessions ------------------------------------------------------------------------------
def test_dim_names_are_the_snapshot_module_s():
    from vslam_amd import snapshot as S
    assert AR.DIM_NAMES == S.DIM_NAMES


def test_the_restated_absorb_of_the_split_loop_world_is_the_one_session_world():
    w = LW.loop_world()
    A, B = MW.split(w)
    assert len(A.kf_desc) == 20 and len(B.kf_desc) == 8 and min(B.obs_kf) >= 0 and max(B.obs_kf) < 8
    a, b = MW.snapshot_of(A), MW.snapshot_of(B)
    da, db = AR.dims_of(a), AR.dims_of(b)
    r = AR.absorb(a, b, dref_injected_shift=len(A.points))
    one = CW.arrays_of(w)
    assert np.array_equal(r["xyz"], one["xyz"]) and np.array_equal(r["obs_off"], one["obs_off"])
    assert np.array_equal(r["obs_kf"], one["obs_kf"]) and np.array_equal(r["obs_kp"], one["obs_kp"])
    shift = np.where(np.arange(len(w.points)) < w.n_old, 0, da["id_bound"])
    assert np.array_equal(r["id"], one["id"] + shift) and da["id_bound"] == int(A.ids.max()) + 1
    d = AR.dims_of(r)
    assert (d["n_kf"], d["n_pts"], d["n_obs"], d["kf_stored"]) == (28, len(w.points), len(w.obs_kf), 28)
    assert d["id_bound"] == da["id_bound"] + db["id_bound"] and d["st_live0"] == d["n_pts"] and d["st_live1"] == d["n_obs"]
    assert r["kf_cnt"].tolist() == w.counts.tolist() and r["kf_ord"].tolist() == list(range(28)) and d["kf_rows"] == int(w.counts.sum())
    assert np.array_equal(r["kf_desc"], np.concatenate(w.kf_desc)) and len(r["kf_kps"]) == d["kf_rows"] and r["kf_P"].shape == (28, 12)
    # injected references move behind A's dicts, the life records behind A's history
    assert r["dref_kf"].tolist() == [-(j + 1) for j in range(len(w.points))]
    assert r["life"][:w.n_old].tolist() == a["life"].tolist() and (r["life"][w.n_old:] == [1, 1, 20 + 7, 0]).all()
    # the inputs are not edited
    assert np.array_equal(a["obs_kf"], A.obs_kf) and AR.dims_of(a) == da


def test_restated_keys_of_stale_entries_and_the_no_op():
    cnt = [8, 0, 5]
    okf = np.array([0, 2, -1, -3, 0, 3, -4, -2 ** 31, 2, 2, 1, 1], np.int32)
    okp = np.array([0, 4, 1, 7, -1, 0, 1, 6, 5, -6, 0, -1], np.int32)
    kf, kp = AR.entry_keys(okf, okp, cnt, 7)
    m = AR.INT32_MIN
    assert kf.tolist() == [7, 9, 9, 7, 7, m, m, m, m, m, m, m]
    assert kp.tolist() == [0, 4, 1, 7, 7, 0, 1, 6, 5, -6, 0, -1]
    kf, kp = AR.entry_keys(okf, okp, [], 7)   # no keyframes: nothing is named
    assert (kf == m).all() and kp.tolist() == okp.tolist()
    a = MW.snapshot_of(MW.split(LW.loop_world())[0])
    empty = MW.snapshot_of(MW.Half(LW.loop_world(), slice(0, 0), [], 0))
    empty["dims"][list(AR.DIM_NAMES).index("kf_stored")] = 5   # a history, nothing live: still a no-op, the ordinals do not move
    r = AR.absorb(a, empty)
    assert all(np.array_equal(r[k], a[k]) for k in a) and set(r) == set(a)
    r = AR.absorb(empty, a)   # into an empty map: the ordinals move behind its history
    assert r["kf_ord"].tolist() == list(range(5, 25)) and AR.dims_of(r)["kf_stored"] == 25 and np.array_equal(r["obs_kf"], a["obs_kf"])


# ---- absorb.h natively ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def native_lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("absorb") / "absorb_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "absorb_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and lines and lines[-1] == "mismatches 0", out.stdout + out.stderr
    return [tuple(part.strip() for part in ln.split("|")) for ln in lines[:-1]]


@needs_gxx
def test_native_every_refusal_has_its_text_and_the_bounds_pass(native_lines):
    hdr = open(os.path.join(ROOT, "visual-slam_amd", "csrc", "absorb.h")).read()
    texts = dict(re.findall(r'#define (ABSORB_[A-Z0-9_]+) "([^"]+)"', hdr))
    assert len(texts) == 6
    broken = [ln for ln in native_lines if ln[0].startswith("broken ")]
    for kind, want, got in broken:
        assert want == got and want != "ok", (kind, want, got)
    assert {ln[1] for ln in broken} == set(texts.values())
    valid = [ln for ln in native_lines if ln[0].startswith("valid ")]
    assert len(valid) >= 8 and all(ln[2] == "ok" for ln in valid)


@needs_gxx
def test_native_key_rule_on_valid_negative_out_of_range_and_int32_min_entries(native_lines):
    rules = {ln[0].split()[1]: (ln[1], ln[2]) for ln in native_lines if ln[0].startswith("rule ")}
    for name in ("valid_first", "negative_key", "negative_row", "key_past_end", "key_before_start", "key_int32_min", "row_past_end", "row_int32_min",
                 "keyframe_of_0_rows", "no_keyframes", "dref_injected", "dref_ordinal", "life_born", "id"):
        assert name in rules
    assert all(want == got for want, got in rules.values()), rules
    # the native rule and the numpy restatement agree on the same entries
    cnt = [8, 0, 5]
    for name, (kf, kp) in {"negative_key": (-1, 1), "both_negative": (-1, -5), "row_before_start": (2, -6), "key_int32_min": (-2 ** 31, 6),
                           "row_int32_max": (0, 2 ** 31 - 1)}.items():
        k2, p2 = AR.entry_keys([kf], [kp], cnt, 7)
        assert rules[name][1] == "%d,%d" % (k2[0], p2[0]), name


# ---- the masked selection --------------------------------------------------------------------------------------------------------------------
def _selections(kf_desc, obs, words, weights, asking, kw_list):
    kc, W, _ = LR.prepared(kf_desc, *obs, words)
    for p in asking:
        for kw in kw_list:
            yield W, kc, p, kw


def _same_selection(a, b):
    assert set(a) == set(b)
    for k in a:
        assert a[k] == b[k], k


@pytest.mark.parametrize("n_kf", [70, 129])
def test_masked_select_with_an_all_ones_mask_is_select_on_the_tiny_worlds(n_kf):
    w = LW.tiny_world(n_kf)
    n = 0
    for W, kc, p, kw in _selections(w.kf_desc, (w.obs_off, w.obs_kf, w.obs_kp), w.words, w.weights, w.asking(),
                                    [dict(n_best=10, max_cand=4), dict(n_best=2, max_cand=16), dict(n_best=0, max_cand=1)]):
        r = LR.select(W, kc, w.weights, p, LW.TINY_MIN_WEIGHT, **kw)
        _same_selection(AR.select_among(W, kc, w.weights, p, np.ones(n_kf, np.uint8), LW.TINY_MIN_WEIGHT, **kw), r)
        _same_selection(AR.select_among(W, kc, w.weights, p, None, LW.TINY_MIN_WEIGHT, **kw), r)
        n += len(r["cand"])
    assert n > 0


def test_masked_select_on_the_loop_world():
    w = LW.loop_world()
    words, weights = LW.loop_vocabulary()
    kc, W, _ = LR.prepared(w.kf_desc, w.obs_off, w.obs_kf, w.obs_kp, words)
    own = (np.arange(LW.N_KF) < MW.SPLIT).astype(np.uint8)
    for p in LW.RETURN_POS:
        r = LR.select(W, kc, weights, p)
        _same_selection(AR.select_among(W, kc, weights, p, np.ones(LW.N_KF, np.uint8)), r)
        m = AR.select_among(W, kc, weights, p, own)
        assert m["cand"] and all(k < MW.SPLIT for k in m["cand"]) and all(m["common"][k] == 0 for k in range(MW.SPLIT, LW.N_KF))
        assert m["connected"] == r["connected"] and m["min_score"] == r["min_score"]
        # masking everything leaves no candidate, and the counts say why
        z = AR.select_among(W, kc, weights, p, np.zeros(LW.N_KF, np.uint8))
        assert z["cand"] == [] and z["max_common"] == 0 and z["n_connected"] == r["n_connected"]


def test_a_same_side_keyframe_wins_unmasked_and_the_mask_names_the_other_side():
    w = MW.same_side_world()
    kc, W, _ = LR.prepared(w.kf_desc, w.obs_off, w.obs_kf, w.obs_kp, w.words)
    r = LR.select(W, kc, w.weights, 3, **MW.SAME_SIDE_KW)
    assert r["cand"] == [2] and r["S"] == [0, 2] and r["M"] == [0, 2] and r["retained"] == [2] and r["min_score"] == 0.0
    assert r["scores"][2] == 1.0 and r["scores"][0] < 0.75
    m = AR.select_among(W, kc, w.weights, 3, MW.SAME_SIDE_AMONG, **MW.SAME_SIDE_KW)
    assert m["cand"] == [0] and m["S"] == [0] and m["common"][2] == 0 and m["score"] == [r["scores"][0]] and m["group"] == [[0]]


# ---- the struct layouts and declarations -------------------------------------------------------------------------------------------------------
def test_absorb_struct_layouts_match_the_header(tmp_path):
    import vslam_amd as V
    structs = [("mo_map_absorb_params", V.MapAbsorbParams), ("mo_map_absorb_out", V.MapAbsorbOut)]
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
    assert C.sizeof(V.MapAbsorbParams) == 8 and C.sizeof(V.MapAbsorbOut) == 88


def test_absorb_calls_are_declared():
    import vslam_amd as V
    lib = V.load_library()
    for name in ("mo_map_absorb", "mo_map_loop_candidates_among"):
        assert name in V.SIGNATURES and hasattr(lib, name)
    from vslam_amd.mapper import LocalMapper
    assert callable(LocalMapper.absorb) and callable(LocalMapper.merge_map)
