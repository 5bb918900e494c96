"""CPU checks of relocalization: the mo_map_relocalize boundary (export, struct layouts against the ctypes mirror) and the numpy
restatement's rules on hand-built cases."""
import os
import subprocess

import numpy as np

from tests.reloc_restatement import knn2_ratio, point_of, rank, restate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_relocalize_is_exported_and_bound():
    import vslam_amd as V
    lib = V.load_library()
    assert hasattr(lib, "mo_map_relocalize") and "mo_map_relocalize" in V.SIGNATURES
    assert lib.mo_abi_version() == V.ABI_VERSION == 7


def test_reloc_struct_layouts_match_the_header(tmp_path):
    import ctypes as C
    import vslam_amd as V
    structs = [("mo_map_reloc_params", V.MapRelocParams), ("mo_map_reloc_out", V.MapRelocOut)]
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


def test_restatement_rules():
    # knn-2: ties to the lower train index, a single train row passes, the ratio is strict
    q = np.zeros((2, 32), np.uint8)
    t = np.zeros((3, 32), np.uint8)
    t[2, 0] = 0xff
    idx, dist, keep = knn2_ratio(q, t, 0.75)
    assert idx[0].tolist() == [0, 1] and dist[0].tolist() == [0, 0] and not keep[0]
    idx, dist, keep = knn2_ratio(q, t[2:], 0.75)
    assert idx[0].tolist() == [0, -1] and keep.all()
    # point_of: lowest point, negative positions and rows count from the end, bad entries skipped
    off = np.array([0, 2, 4, 6])
    okf = np.array([0, 1, -1, 5, 0, 1])
    okp = np.array([1, -1, 0, 0, 1, 7])
    tab = point_of(off, okf, okp, [2, 3])
    assert tab[0].tolist() == [-1, 0] and tab[1].tolist() == [1, -1, 0]
    # ranking: score >= 15, highest first, ties to the lower position, capped
    assert rank([15, 40, 14, 40, 20], 3) == [1, 3, 4]
    assert rank([3, 14], 4) == []


def test_restated_correspondences_follow_the_table():
    rng = np.random.default_rng(3)
    kf = [rng.integers(0, 256, (40, 32)).astype(np.uint8) for _ in range(2)]
    query = kf[1][::2].copy()
    off = np.arange(0, 41, 2)
    okf = np.tile([1, 0], 20)
    okp = np.repeat(np.arange(20), 2) * 2
    r = restate(query, kf, off, okf, okp)
    assert r["scores"] == [0, 20] and r["candidates"] == [1]
    qi, pi = r["C"][1]
    assert qi.tolist() == list(range(20)) and pi.tolist() == list(range(20))
