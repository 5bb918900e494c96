"""The map snapshot without a GPU: the validation rules of visual-slam_amd/csrc/snapshot.h under AddressSanitizer and UBSan
(tests/native/snapshot_check.cpp), the file checks of LocalMapper.load_state, and the layouts of the new boundary structs."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs a host C++ compiler")


# ---- the native validation check ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def native_lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("snapshot") / "snapshot_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "snapshot_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and lines and lines[-1] == "mismatches 0", out.stdout + out.stderr
    return [tuple(part.strip() for part in ln.split("|")) for ln in lines[:-1]]


@needs_gxx
def test_native_valid_shapes_pass(native_lines):
    got = {ln[0].split()[1]: ln[2] for ln in native_lines if ln[0].startswith("valid ")}
    for shape in ("empty_map", "one_keyframe", "keyframe_of_0_rows", "stale_observation_keys"):
        assert got[shape] == "ok", (shape, got[shape])
    assert all(v == "ok" for v in got.values()), got


@needs_gxx
def test_native_every_rule_refuses_with_its_text(native_lines):
    """one broken snapshot at least per rule text the header defines, each refused with exactly that text"""
    hdr = open(os.path.join(ROOT, "visual-slam_amd", "csrc", "snapshot.h")).read()
    import re
    texts = dict(re.findall(r'#define (SNAP_[A-Z0-9_]+) "([^"]+)"', hdr))
    assert len(texts) >= 12
    broken = [ln for ln in native_lines if ln[0].startswith("broken ")]
    for kind, want, got in broken:
        assert want == got and want != "ok", (kind, want, got)
    assert {ln[1] for ln in broken} == set(texts.values())


# ---- the struct layouts --------------------------------------------------------------------------------------------------------------------
def test_snapshot_struct_layouts_match_the_header(tmp_path):
    import vslam_amd as V
    structs = [("mo_map_snapshot_dims_t", V.MapSnapshotDims), ("mo_map_snapshot", V.MapSnapshot)]
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
    assert C.sizeof(V.MapSnapshotDims) == 112


def test_snapshot_calls_are_declared():
    import vslam_amd as V
    lib = V.load_library()
    for name in ("mo_map_snapshot_dims", "mo_map_export", "mo_map_import"):
        assert name in V.SIGNATURES and hasattr(lib, name)


# ---- the file checks of load_state -------------------------------------------------------------------------------------------------------
def valid_file_arrays():
    """the arrays of a state file of a small map (two keyframes, one removed before them; two points, one injected), built by hand"""
    import vslam_amd as V
    from vslam_amd import snapshot as S
    dims = dict.fromkeys(S.DIM_NAMES, 0)
    dims.update(n_kf=2, kf_rows=5, n_pts=2, n_obs=3, kf_stored=3, id_bound=2, st_live0=2, st_live1=3, img_cur=1, img_w1=4, img_h1=3, img_ch1=1,
                img_bytes1=12, img_ch0=1)
    out = {"format_version": np.array(S.FORMAT_VERSION, np.int64), "dims": np.array([dims[k] for k in S.DIM_NAMES], np.int64)}
    m = {name: np.zeros(shape, dtype) for name, (dtype, shape) in S.array_specs(out["dims"]).items()}
    m["kf_cnt"][:] = (3, 2)
    m["kf_ord"][:] = (1, 2)
    m["obs_off"][:] = (0, 2, 3)
    m["dref_kf"][:] = (0, -1)       # point 0: a row of the removed keyframe (ordinal 0); point 1: injected dict 0
    m["dref_row"][:] = (4, 0)
    m["id"][:] = (0, 1)
    m["life"][:] = ((1, 1, 0, 0), (1, 1, 2, 0))
    out.update({"map_" + k: v for k, v in m.items()})
    i8, f8, u1 = np.int64, np.float64, np.uint8
    out.update(camera_matrix=np.eye(3), settings=np.array([0.9, 2, 0.05, 1.0]), sampling=np.array([1024, 4096, 0], np.uint64),
               kf_ids=np.arange(2, dtype=i8), kf_poses=np.tile(np.eye(4), (2, 1, 1)), kf_serials=np.array([1, 2], i8), next_serial=np.array(3, i8),
               list_rows=np.array([-1, -1], i8), covis=np.zeros((0, 3), i8), rec_n=np.array([6, 3, 2], i8),
               dead_ref=np.array([[0, 4]], i8), dead_desc=np.zeros((1, 32), u1),
               n_injected=np.array(1, i8), inj_index=np.zeros(1, i8), inj_id=np.ones(1, i8), inj_pos=np.zeros((1, 3), f8),
               inj_flags=np.zeros((1, 3), u1), inj_color=np.zeros((1, 3), u1), inj_desc=np.zeros((1, 32), u1), inj_obs_off=np.zeros(2, i8),
               inj_obs=np.zeros((0, 2), i8), lc_threshold=np.array(-1, i8), lc_counts=np.zeros(0, i8), lc_off=np.zeros(1, i8),
               lc_serials=np.zeros(0, i8), vocab_words=np.zeros((0, 32), u1), vocab_weights=np.zeros(0, np.int32),
               images_all=np.array(0, i8), image_shapes=np.zeros((0, 3), i8), last_image=np.zeros((3, 4), u1),
               last_image_size=np.array([4, 3], i8))
    return out


def write(tmp_path, arrays, allow_pickle=False):
    path = str(tmp_path / "state.npz")
    with open(path, "wb") as fh:
        np.savez(fh, **arrays)
    return path


@pytest.fixture
def no_context(monkeypatch):
    """load_state must fail on the file before it asks for a context or the library"""
    import vslam_amd as V

    def refuse(*a, **k):
        raise AssertionError("load_state touched the library before the file was checked")
    monkeypatch.setattr(V, "default_context", refuse)
    monkeypatch.setattr(V, "Context", refuse)
    monkeypatch.setattr(V, "load_library", refuse)


def test_the_hand_built_file_passes_the_file_checks(tmp_path):
    from vslam_amd import snapshot as S
    with np.load(write(tmp_path, valid_file_arrays()), allow_pickle=False) as z:
        f = S.check_file(z)
    assert f["kf_cnt"].tolist() == [3, 2] and int(f["n_injected"]) == 1


def edit_version(a):
    a["format_version"] = np.array(2, np.int64)


def edit_missing(a):
    del a["map_life"]


def edit_missing_host(a):
    del a["kf_serials"]


def edit_dtype(a):
    a["map_xyz"] = a["map_xyz"].astype(np.float64)


def edit_dtype_kps(a):
    a["map_kf_kps"] = np.zeros((5, 7), np.float32)


def edit_shape(a):
    a["map_kf_desc"] = np.zeros((5, 16), np.uint8)


def edit_shape_count(a):
    a["map_obs_kf"] = np.zeros(4, np.int32)


def edit_counts_kf(a):
    a["map_kf_cnt"] = np.array([3, 1], np.int32)


def edit_counts_obs(a):
    a["map_obs_off"] = np.array([0, 2, 2], np.int32)


def edit_counts_rec(a):
    a["rec_n"] = np.array([6, 3, 5], np.int64)


def edit_dead_ref(a):
    a["dead_ref"] = np.array([[0, 3]], np.int64)


def edit_injected(a):
    a["inj_index"] = np.zeros(0, np.int64)
    for k in ("inj_id", "inj_pos", "inj_flags", "inj_color", "inj_desc"):
        a[k] = a[k][:0]
    a["inj_obs_off"] = np.zeros(1, np.int64)


def edit_id(a):
    a["map_id"] = np.array([0, 2], np.int32)


def edit_life(a):
    a["map_life"] = np.array([[1, 1, 0, 0], [1, 1, 3, 0]], np.int32)


def edit_st_live(a):
    a["dims"] = a["dims"].copy()
    a["dims"][15] = 1


def edit_image_bytes(a):
    a["dims"] = a["dims"].copy()
    a["dims"][8], a["dims"][10], a["dims"][12] = 2, 2, 3   # image 0: 2 x 2 x 3 with 0 bytes


def edit_last_image(a):
    a["last_image_size"] = np.array([5, 3], np.int64)


def edit_object(a):
    a["kf_ids"] = np.array([{"id": 0}, None], dtype=object)


@pytest.mark.parametrize("edit,name", [
    (edit_version, "format_version"), (edit_missing, "map_life"), (edit_missing_host, "kf_serials"), (edit_dtype, "map_xyz"),
    (edit_dtype_kps, "map_kf_kps"), (edit_shape, "map_kf_desc"), (edit_shape_count, "map_obs_kf"), (edit_counts_kf, "map_kf_cnt"),
    (edit_counts_obs, "map_obs_off"), (edit_counts_rec, "rec_n"), (edit_dead_ref, "dead_ref"), (edit_injected, "inj_index"),
    (edit_id, "map_id"), (edit_life, "map_life"), (edit_st_live, "dims"), (edit_image_bytes, "dims"), (edit_last_image, "last_image_size"),
    (edit_object, "kf_ids")])
def test_load_state_refuses_a_bad_file_before_any_context(tmp_path, no_context, edit, name):
    from vslam_amd.mapper import LocalMapper
    a = valid_file_arrays()
    edit(a)
    path = str(tmp_path / "state.npz")
    with open(path, "wb") as fh:
        np.savez(fh, **a)   # (numpy pickles the object array on writing; reading it back without pickle is what must fail)
    with pytest.raises(ValueError, match=r"'%s'" % name):
        LocalMapper.load_state(path)
