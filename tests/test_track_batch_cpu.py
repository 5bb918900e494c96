"""mo_map_track_batch / LocalMapper.track_local_map_batch without a device: the struct as a C compiler sees it against the ctypes
mirror, the exported symbol, and the argument errors the Python side raises before any device call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batch_out_layout_matches_the_header(tmp_path):
    """the method of tests/test_cabi_cpu.py::test_struct_layouts_match_the_header on mo_map_track_batch_out, and MO_TRACK_BATCH_MAX"""
    import vslam_amd as V
    cname, cls = "mo_map_track_batch_out", V.MapTrackBatchOut
    body = '  printf("%%zu\\n", sizeof(%s));\n' % cname
    body += "".join('  printf("%%zu\\n", offsetof(%s, %s));\n' % (cname, f[0]) for f in cls._fields_)
    body += '  printf("%d\\n", MO_TRACK_BATCH_MAX);\n'
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vslam_amd.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    offs = [getattr(cls, f[0]).offset for f in cls._fields_]
    assert got[0] == C.sizeof(cls)
    assert got[1:1 + len(offs)] == offs
    assert got[1 + len(offs)] == V.TRACK_BATCH_MAX == 1024
    assert [f[0] for f in cls._fields_] == ["stride", "point", "dist", "inlier", "pose", "pass_pose", "pass_radius", "pass_cand", "pass_matches",
                                            "pass_inliers", "n_pass_run", "ok", "from_token", "n_local", "n_ok"]


def test_symbol_is_exported_with_its_signature():
    import vslam_amd as V
    lib = V.load_library()
    assert hasattr(lib, "mo_map_track_batch")
    restype, argtypes = V.SIGNATURES["mo_map_track_batch"]
    assert restype is C.c_int and len(argtypes) == 7 and argtypes[2] is C.c_int32


def _mapper_without_a_device():
    """an instance whose every attribute access fails: the argument checks must come before anything touches the map or the library"""
    from vslam_amd.mapper import LocalMapper

    class Untouchable(LocalMapper):
        def __init__(self):
            pass

        def __getattr__(self, name):
            raise AssertionError("the call reached for %r before it had checked its arguments" % name)

        def __del__(self):
            pass
    return Untouchable()


def test_argument_errors_come_before_any_device_call():
    import vslam_amd as V
    m = _mapper_without_a_device()
    kps, desc = np.zeros(5, V.KP_DTYPE), np.zeros((5, 32), np.uint8)
    eye = np.eye(4)
    with pytest.raises(ValueError, match="poses"):   # wrong length
        m.track_local_map_batch([(kps, desc), (kps, desc)], [eye])
    with pytest.raises(ValueError, match="poses"):   # a single 4 x 4 in place of [n][4][4]
        m.track_local_map_batch([(kps, desc)], eye)
    with pytest.raises(ValueError, match="poses"):   # [n][4][3]
        m.track_local_map_batch([(kps, desc)], np.zeros((1, 4, 3)))
    with pytest.raises(ValueError, match="poses"):   # [n][12]
        m.track_local_map_batch([(kps, desc)], np.zeros((1, 12)))
    with pytest.raises(ValueError, match="pairs"):   # an entry that is not a pair
        m.track_local_map_batch([(kps, desc), kps], [eye, eye])
    with pytest.raises(ValueError, match="pairs"):
        m.track_local_map_batch([(kps, desc, 1)], [eye])
    with pytest.raises(ValueError, match="radii"):
        m.track_local_map_batch([(kps, desc)], [eye], radii=())
    with pytest.raises(ValueError, match="at most"):
        m.track_local_map_batch([(kps, desc)] * (V.TRACK_BATCH_MAX + 1), np.tile(eye, (V.TRACK_BATCH_MAX + 1, 1, 1)))
