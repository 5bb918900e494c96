"""The place-recognition rules (the comment above mo_vocab_train in include/vslam_amd.h) on their numpy restatement
(tests/bow_restatement.py): hand cases of quantisation and training, the score against exact rational arithmetic, and place
recognition on the pan-back world and on the relocalization world the GPU tests run."""
from fractions import Fraction

import numpy as np
import pytest

from tests import bow_restatement as B
from tests import bow_worlds as BW
from tests.covis_worlds import pan_back

_VOC = {}

# Place recognition on the pan-back world at W = 1024, 10 iterations, strided initialisation: the restatement ranks the keyframes
# 5, 4, 3, 2, 1 (scores 0.3717, 0.3455, 0.3159, 0.2754, 0.2691), all of region A, before the first other keyframe (14, 0.2431); the
# sixth A keyframe, 0, comes eleventh.  So the first 5 places are asserted.
PAN_WORDS, PAN_FIRST = 1024, 5
RELOC_WORDS, RELOC_PRE = 1024, 3


def vocabulary(name):
    return BW.vocabulary(name, PAN_WORDS if name == "pan" else RELOC_WORDS)


def test_equidistant_descriptor_goes_to_the_lower_word():
    d, words = BW.hand_equidistant()
    assert B.hamming(d[None], words).tolist() == [[4, 2, 2]]
    assert B.quantise(d[None], words).tolist() == [1]


def test_majority_bits_and_early_stop():
    desc, off, W = BW.hand_split()
    words, weights, ran = B.train(desc, off, W, 10)
    bits = np.unpackbits(words, axis=1, bitorder="little")
    assert bits[0, 5] == 0 and bits[0, 9] == 1 and bits[0].sum() == 1          # 2 / 2 -> 0, 3 / 1 -> 1
    assert bits[1, 200] == 0 and bits[1, 77] == 1 and bits[1].sum() == 255
    assert ran == 2                                                            # the second iteration changes nothing
    assert B.train(desc, off, W, 1)[2] == 1
    # word 0 is seen in both images, word 1 in the second only
    assert weights.tolist() == [0, int(np.rint(np.log(2.0) * 1024))]


def test_word_without_members_and_duplicate_words():
    desc, off, W = BW.hand_duplicates()
    words, weights, ran = B.train(desc, off, W, 10)
    assert np.array_equal(words[1], desc[2])                                   # the duplicate: no member, unchanged
    assert np.array_equal(words[0], desc[0])
    assert np.array_equal(words[2], desc[5])                                   # bit 100 set in 1 of 2: cleared
    assert B.quantise(desc, words).tolist() == [0, 0, 0, 0, 2, 2]
    assert weights.tolist() == [0, 0, 0] and ran == 2                          # (one image: log(1 / max(n_w, 1)) = 0)


def test_fewer_rows_than_words_is_refused():
    desc, off, _ = BW.hand_split()
    with pytest.raises(ValueError):
        B.train(desc, off, 9, 10)
    with pytest.raises(ValueError):
        B.train(desc, np.array([0], np.int64), 2, 10)
    B.train(desc, off, 8, 10)


def test_score_equals_the_rational_l1_score():
    rng = np.random.default_rng(12)
    for _ in range(20):
        W = int(rng.integers(2, 300))
        wt = rng.integers(0, B.MAX_WEIGHT + 1, W)
        qc = rng.multinomial(int(rng.integers(1, B.MAX_ROWS + 1)), rng.dirichlet(np.ones(W) * 0.2))
        kc = rng.multinomial(int(rng.integers(1, B.MAX_ROWS + 1)), rng.dirichlet(np.ones(W) * 0.2))
        q = [int(c) * int(w) for c, w in zip(qc, wt)]
        k = [int(c) * int(w) for c, w in zip(kc, wt)]
        if sum(q) == 0 or sum(k) == 0:
            assert B.score(qc, kc, wt) == 0.0
            continue
        exact = 1 - Fraction(1, 2) * sum(abs(Fraction(a, sum(q)) - Fraction(b, sum(k))) for a, b in zip(q, k))
        assert abs(Fraction(B.score(qc, kc, wt)) - exact) < Fraction(1, 10 ** 15)
        D, nq, nk = B.distance(qc, kc, wt)
        assert D <= 2 * nq * nk < 2 ** 61


def test_largest_distance_stays_inside_int64():
    # two frames of 65535 rows in one word each, the largest weight: D = 2 |q| |k|
    wt = np.array([B.MAX_WEIGHT, B.MAX_WEIGHT])
    D, nq, nk = B.distance([B.MAX_ROWS, 0], [0, B.MAX_ROWS], wt)
    assert nq == nk == B.MAX_ROWS * B.MAX_WEIGHT < 2 ** 30 and D == 2 * nq * nk < 2 ** 61
    assert B.score([B.MAX_ROWS, 0], [0, B.MAX_ROWS], wt) == 0.0


def test_disjoint_vectors_score_zero_and_a_vector_against_itself_one():
    wt = np.array([5, 1024, 0, 77, 14336, 3])
    a, b = np.array([3, 0, 9, 0, 2, 0]), np.array([0, 4, 1, 6, 0, 1])
    assert B.score(a, b, wt) == 0.0
    assert B.score(a, a, wt) == 1.0 and B.score(b, b, wt) == 1.0
    assert B.score(a, np.zeros(6, np.int64), wt) == 0.0                        # a zero norm
    assert B.score(np.array([0, 0, 5, 0, 0, 0]), a, wt) == 0.0                 # every word of the frame has weight 0


def test_pan_back_first_places_are_region_a():
    w = pan_back()
    words, weights, _ = vocabulary("pan")
    _, qd = w.query()
    pos, sc = B.query(qd, w.kf_desc, words, weights, 20)
    print("pan-back, W = %d: positions %s scores %s" % (PAN_WORDS, pos, ["%.4f" % s for s in sc]))
    assert len(pos) > PAN_FIRST and all(p in range(0, 6) for p in pos[:PAN_FIRST])
    assert pos[PAN_FIRST] not in range(0, 6) and sc[PAN_FIRST - 1] > sc[PAN_FIRST]   # the gap to the first keyframe outside A
    assert sc == sorted(sc, reverse=True)


@pytest.mark.parametrize("k", [5, 0])
def test_preselection_keeps_the_brute_force_winner(k):
    w = BW.reloc_world()
    words, weights, _ = vocabulary("reloc")
    _, qd = w.query(k, w.query_pose(k))
    cand, scores, _VOC["tab"] = B.brute_force_candidates(qd, w.kf_desc, w.obs_off, w.obs_kf, w.obs_kp, 0.75, 4, _VOC.get("tab"))
    pos, _ = B.query(qd, w.kf_desc, words, weights, RELOC_PRE)
    print("query near keyframe %d: brute force %s (scores %s), query %s" % (k, cand, [scores[p] for p in cand], pos))
    assert cand[0] == k and cand[0] in pos, (cand, pos)
