"""mo_map_relocalize_batch / LocalMapper.relocalize_batch without a device: the group plan on hand cases, the structs as a C compiler
sees them against the ctypes mirrors, the exported symbols, and the argument errors the Python side raises before any device call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GIB = 1 << 30


def _plan(*a, **kw):
    from vslam_amd.mapper import LocalMapper
    return LocalMapper.reloc_batch_plan(*a, **kw)


def test_group_plan_hand_cases():
    """(frames per group, groups): whole frames under max_pairs, at least one frame per group"""
    # 7 frames of 8 pairs: one frame per group at a budget of one frame's pairs, and below it
    assert _plan(7, 8, 2400, max_pairs=8) == (1, 7)
    assert _plan(7, 8, 2400, max_pairs=1) == (1, 7)        # one frame above the budget: still one frame per group
    assert _plan(7, 8, 2400, max_pairs=7) == (1, 7)
    # boundaries that do not divide the batch: 23 pairs hold two frames, 7 frames run as 2 + 2 + 2 + 1
    assert _plan(7, 8, 2400, max_pairs=23) == (2, 4)
    assert _plan(7, 8, 2400, max_pairs=24) == (3, 3)       # an exact fit of three frames: 3 + 3 + 1
    assert _plan(6, 8, 2400, max_pairs=24) == (3, 2)       # ... and one that divides the batch
    assert _plan(7, 8, 2400, max_pairs=56) == (7, 1)       # the whole batch fits exactly
    assert _plan(7, 8, 2400, max_pairs=10 ** 12) == (7, 1)
    # no frames: no group; a map without keyframes has no pairs: one group
    assert _plan(0, 8, 2400, max_pairs=8) == (1, 0)
    assert _plan(0, 8, 2400) == (1, 0)
    assert _plan(5, 0, 2400) == (5, 1)


def test_group_plan_default_budget():
    """1 GiB of matcher output at 17 bytes per (pair, row), never more than the 65535 pairs of one matcher launch"""
    # 1024 keyframes of 2000 rows: 31580 pairs, 30 frames per group
    pairs = GIB // (17 * 2000)
    assert pairs == 31580
    assert _plan(1024, 1024, 2000) == (30, 35)
    assert _plan(30, 1024, 2000) == (30, 1) and _plan(31, 1024, 2000) == (30, 2)
    # exact fits of the default: 1 GiB / (17 * 4096) = 15420 pairs = 15420 frames of one pair, 7710 of two
    assert GIB // (17 * 4096) == 15420
    assert _plan(1024, 15420, 4096) == (1, 1024) and _plan(1024, 15421, 4096) == (1, 1024)
    assert _plan(1024, 7710, 4096) == (2, 512) and _plan(1024, 7711, 4096) == (1, 1024)
    # short rows: the launch limit, not the memory, bounds the group
    assert GIB // (17 * 64) > 65535
    assert _plan(1024, 64, 64) == (1023, 2) and _plan(1024, 64, 64, max_pairs=10 ** 9) == (1023, 2)
    assert _plan(1000, 65535, 64) == (1, 1000) and _plan(1000, 65536, 64) == (1, 1000)
    with pytest.raises(ValueError):
        _plan(-1, 8, 2400)
    with pytest.raises(ValueError):
        _plan(1, -8, 2400)


def test_layouts_match_the_header(tmp_path):
    """the method of tests/test_cabi_cpu.py::test_struct_layouts_match_the_header on the two batch structs, and MO_RELOC_BATCH_MAX"""
    import vslam_amd as V
    structs = [("mo_map_reloc_batch_params", V.MapRelocBatchParams), ("mo_map_reloc_batch_out", V.MapRelocBatchOut)]
    body = ""
    for cname, cls in structs:
        body += '  printf("%%zu\\n", sizeof(%s));\n' % cname
        body += "".join('  printf("%%zu\\n", offsetof(%s, %s));\n' % (cname, f[0]) for f in cls._fields_)
    body += '  printf("%d\\n", MO_RELOC_BATCH_MAX);\n'
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vslam_amd.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    k = 0
    for cname, cls in structs:
        offs = [getattr(cls, f[0]).offset for f in cls._fields_]
        assert got[k] == C.sizeof(cls), cname
        assert got[k + 1:k + 1 + len(offs)] == offs, cname
        k += 1 + len(offs)
    assert got[k] == V.RELOC_BATCH_MAX == 1024
    assert [f[0] for f in V.MapRelocBatchParams._fields_] == ["p", "n_pre", "max_pairs"]
    assert [f[0] for f in V.MapRelocBatchOut._fields_] == ["stride", "point", "inlier", "cand_pos", "cand_score", "cand_inliers", "pose", "ok", "kf_pos",
                                                            "n_cand", "n_corr", "n_inliers", "from_token", "n_ok", "n_groups"]


def test_symbols_are_exported_with_their_signatures():
    import vslam_amd as V
    lib = V.load_library()
    for name, n_args in (("mo_map_relocalize_batch", 6), ("mo_map_query_keyframes_batch", 8), ("mo_map_reloc_batch_plan", 6)):
        assert hasattr(lib, name), name
        restype, argtypes = V.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == n_args, name
    # the plan refuses what it cannot hold, through the C boundary too
    fpg, ng = C.c_int32(-5), C.c_int32(-5)
    assert lib.mo_map_reloc_batch_plan(3, 8, 100, -1, C.byref(fpg), C.byref(ng)) == V.MO_ERR_ARG and fpg.value == -5
    assert lib.mo_map_reloc_batch_plan(3, 8, 100, 0, None, C.byref(ng)) == V.MO_ERR_ARG
    assert lib.mo_map_reloc_batch_plan(3, 8, 100, 16, C.byref(fpg), C.byref(ng)) == 0 and (fpg.value, ng.value) == (2, 2)


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
    with pytest.raises(ValueError, match="pairs"):   # an entry that is not a pair
        m.relocalize_batch([(kps, desc), kps])
    with pytest.raises(ValueError, match="pairs"):
        m.relocalize_batch([(kps, desc, 1)])
    with pytest.raises(ValueError, match="at most"):
        m.relocalize_batch([(kps, desc)] * (V.RELOC_BATCH_MAX + 1))
    with pytest.raises(ValueError, match="max_pairs"):
        m.relocalize_batch([(kps, desc)], max_pairs=0)
    with pytest.raises(ValueError, match="max_pairs"):
        m.relocalize_batch([(kps, desc)], max_pairs=-3)
    with pytest.raises(ValueError, match="max_candidates"):
        m.relocalize_batch([(kps, desc)], max_candidates=0)
    with pytest.raises(ValueError, match="max_candidates"):
        m.relocalize_batch([(kps, desc)], max_candidates=65)
    with pytest.raises(ValueError, match="pairs"):
        m.query_keyframes_batch([kps])
    with pytest.raises(ValueError, match="at most"):
        m.query_keyframes_batch([(kps, desc)] * (V.RELOC_BATCH_MAX + 1))
    with pytest.raises(ValueError, match="n_best"):
        m.query_keyframes_batch([(kps, desc)], n_best=-1)
