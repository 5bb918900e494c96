"""The local and the global bundle adjustment follow each other on one map.  Both build their problem in the same scratch arrays
(BaProblem of csrc/ba_problem.h), so a chain that read what the other solver's call left there would go unnoticed by the tests that run
one solver per map.  Here the sequence local (window form), global, local (set form, erasing its outliers), global runs on a rebuilt map
under every poison byte, and every returned array and scalar and the map after every step must keep the bytes of the unpoisoned run.

Cases of tests/gba_cases.py: A, 24 keyframes x 40 rows (under a thousand points, many keyframes, a conjugate gradient over several free
blocks); C, 4 keyframes x 1500 rows (more than 256 problem points: the point kernels span several workgroups and the 1024-thread
reductions several waves; the fewest free keyframes behind the two-keyframe gauge)."""
import pytest

from tests.gba_cases import case
from tests.test_gpu_bundle_adjust import _mapper
from tests.test_gpu_scratch_poison import BYTES, _checked, _ctx, _flat, _map_state, _same, _set

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name, window", [("A", 8), ("C", 0)])
def test_local_and_global_ba_in_turn_under_poison(name, window):
    s = case(name)
    poses, xyz = s.perturbed()
    free = list(range(s.n_kf - 3, s.n_kf))
    c = _ctx()
    try:
        def run(poisoned):
            m = _checked(c, lambda: _mapper(c, s, poses, xyz), poisoned)
            steps = [lambda: m.bundle_adjust(window=window, want_points=True),
                     lambda: m.global_bundle_adjust(fixed=[0, 1], want_points=True),
                     lambda: m.bundle_adjust(free=free, erase_outliers=True, want_points=True),
                     lambda: m.global_bundle_adjust(fixed=[0, 1], want_points=True)]
            out = []
            for fn in steps:
                ok, info = _checked(c, fn, poisoned)
                out.append({"ok": ok, "info": info, "kf_poses": [kf["pose"].copy() for kf in m.keyframes], "map": _map_state(m)})
            accepted = [sum(o["info"]["accepted"]) if i % 2 == 0 else o["info"]["accepted"] for i, o in enumerate(out)]
            print("case %s, poisoned %s: accepted steps per call %s, entries erased %d" % (name, poisoned, accepted, out[2]["info"]["n_erased"]))
            assert accepted[0] > 0 and accepted[1] > 0 and accepted[3] > 0, accepted   # (a map on which nothing ran would pass too)
            assert out[2]["info"]["n_free"] > 0
            m.close()
            return _flat(out)
        want = run(False)
        for byte in BYTES:
            _set(c, byte)
            _same(run(True), want, (byte, "case " + name))
            assert c.dev_status() == 0
    finally:
        c.close()
