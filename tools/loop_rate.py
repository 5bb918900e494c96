"""Loop candidates against the number of keyframes: the stages of mo_map_loop_candidates for max_cand = 0 (detection alone) and 4
(with the matching), next to its yardsticks on the same map in the same process: query_keyframes(8) + covisibility() for the detection,
the reloc_match stage of relocalize(preselect=4) for the matching (the same four matcher pairs).

The maps of tools/bow_rate.py (2000-row keyframes of random descriptors, 100000 injected points with two observations each) at 64, 256
and 1024 keyframes, vocabularies of 1024 and 4096 words trained on 10^5 random rows.  Device medians of 10 warm calls per line.
With a library that predates the call (VSLAM_AMD_LIB pointing at the parent commit's build) only the yardsticks are measured.
python tools/loop_rate.py   (one MI355X)
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "visual-slam_amd"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402

import vslam_amd as V  # noqa: E402
from bow_rate import ROWS, build, medians  # noqa: E402

ASK = 10   # the asking keyframe: one that shares points with its two neighbours (the last keyframes of these maps share none)


def loop_call(m, max_cand):
    """the native call with no output array but the candidates: nothing is copied out that the timing would have to carry"""
    cand = np.full(max(max_cand, 1), -1, np.int32)
    n_match = np.zeros(max(max_cand, 1), np.int32)
    prm = V.MapLoopParams(ASK, 15, 10, max_cand, 0.75)
    out = V.MapLoopOut(cand.ctypes.data, None, None, None, None, None, None, None, n_match.ctypes.data)

    def call():
        m._check(m.lib.mo_map_loop_candidates(m._h, C.byref(prm), C.byref(out)))
        return int(out.n_found), int(out.n_scored), int(out.n_passed), cand[:int(out.n_cand)].tolist(), n_match[:int(out.n_cand)].tolist()
    return call


def line(st):
    return "  ".join("%s %.3f" % kv for kv in st.items())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", default="64,256,1024")
    ap.add_argument("--words", default="1024,4096")
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    ctx = V.Context(device=0, max_w=640, max_h=480, max_batch=1)
    ctx.set_host_timing(True)
    have = hasattr(ctx.lib, "mo_map_loop_candidates")
    vocs = {}
    for W in [int(x) for x in args.words.split(",")]:
        vocs[W] = V.Vocabulary.train([rng.integers(0, 256, (ROWS, 32)).astype(np.uint8) for _ in range(50)], W, 10, context=ctx)
    for n_kf in [int(x) for x in args.keyframes.split(",")]:
        m, qk, qd = build(ctx, n_kf, rng)
        for W, v in vocs.items():
            m.set_vocabulary(v)
            m.query_keyframes(qk, qd, 8)   # every keyframe counted
            q_st, q_dev, _, _ = medians(ctx, lambda: m.query_keyframes(qk, qd, 8))
            c_st, c_dev, _, _ = medians(ctx, lambda: m.covisibility())
            r_st, _, _, _ = medians(ctx, lambda: m.relocalize(qk, qd, preselect=4))
            print("keyframes %4d  words %5d  yardstick detection: query_keyframes(8) %.3f + covisibility %.3f = %.3f ms  | %s  %s"
                  % (n_kf, W, q_dev, c_dev, q_dev + c_dev, line(q_st), line(c_st)), flush=True)
            print("keyframes %4d  words %5d  yardstick matching: relocalize(preselect=4) reloc_match %.3f ms" % (n_kf, W, r_st["reloc_match"]), flush=True)
            if not have:
                continue
            for mc in (0, 4):
                st, dev, wall, res = medians(ctx, loop_call(m, mc))
                print("keyframes %4d  words %5d  loop_candidates(max_cand=%d): device median %.3f ms  wall median %.3f ms  found %d scored %d passed %d "
                      "cand %s matches %s  | %s" % ((n_kf, W, mc, dev, wall) + res + (line(st),)), flush=True)
                if mc == 0:
                    print("keyframes %4d  words %5d  detection / yardstick: %.3f" % (n_kf, W, dev / (q_dev + c_dev)), flush=True)
        m.close()
    ctx.close()


if __name__ == "__main__":
    main()
