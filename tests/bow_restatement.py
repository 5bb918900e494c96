"""numpy restatement of the place-recognition rules (the comment above mo_vocab_train in include/vslam_amd.h), step for step:
quantisation, vocabulary training, the per-keyframe term counts, the integer L1 distance D_k, the f64 score and the ranking.
Everything is integer work except the logarithm of the weights and the one division of the score."""
import numpy as np

MAX_WORDS = 8192
MAX_WEIGHT = 14 * 1024
MAX_ROWS = 65535
MAX_IMAGES = 1 << 20


def _bits(d):
    """[n][256] float32 0 / 1 of 32-byte descriptors, bit b = bit (b % 8) of byte b // 8"""
    d = np.asarray(d, np.uint8).reshape(-1, 32)
    return np.unpackbits(d, axis=1, bitorder="little").astype(np.float32)


def hamming(qd, td):
    """[nq][nt] Hamming distances by a matmul over the unpacked bits: |a ^ b| = |a| + |b| - 2 a.b (exact in f32: every value <= 256)"""
    a, b = _bits(qd), _bits(td)
    return (a.sum(1)[:, None] + b.sum(1)[None, :] - 2.0 * (a @ b.T)).astype(np.int32)


def quantise(desc, words):
    """the word of every descriptor: lowest Hamming distance, ties to the lower word index"""
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    out = np.zeros(len(desc), np.int32)
    for b in range(0, len(desc), 4096):
        out[b:b + 4096] = np.argmin(hamming(desc[b:b + 4096], words), axis=1)   # (argmin returns the first minimum)
    return out


def train(desc, img_off, n_words, iters=10, init=None):
    """(words [W][32] u8, weights [W] i32, iterations run); init: initial rows in place of the strided ones (the seeded control run)"""
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    img_off = np.asarray(img_off, np.int64)
    n, n_img, W = len(desc), len(img_off) - 1, int(n_words)
    if not (2 <= W <= MAX_WORDS) or n < W or n_img < 1 or n_img > MAX_IMAGES or iters < 0:
        raise ValueError("MO_ERR_ARG")
    if img_off[0] != 0 or img_off[-1] != n or (np.diff(img_off) < 0).any():
        raise ValueError("MO_ERR_ARG")
    rows = (np.arange(W, dtype=np.int64) * n) // W if init is None else np.asarray(init, np.int64)
    words = desc[rows].copy()
    bits = np.unpackbits(desc, axis=1, bitorder="little").astype(np.int64)
    ran = 0
    word_of = None
    for _ in range(iters):
        word_of = quantise(desc, words)
        ran += 1
        members = np.bincount(word_of, minlength=W).astype(np.int64)
        ones = np.zeros((W, 256), np.int64)
        np.add.at(ones, word_of, bits)
        new_bits = (2 * ones > members[:, None]).astype(np.uint8)
        new = np.packbits(new_bits, axis=1, bitorder="little")
        new[members == 0] = words[members == 0]
        changed = not np.array_equal(new, words)
        words = new
        if not changed:
            break
        word_of = None   # (the words moved: the weights quantise again)
    if word_of is None:
        word_of = quantise(desc, words)
    img_of = np.repeat(np.arange(n_img), np.diff(img_off))
    seen = np.zeros((n_img, W), bool)
    seen[img_of, word_of] = True
    n_w = seen.sum(0).astype(np.int64)
    return words, weights_of(n_w, n_img), ran


def weights_of(n_w, n_img):
    """rint(log(n_img / max(n_w, 1)) * 1024) in f64"""
    return np.rint(np.log(float(n_img) / np.maximum(np.asarray(n_w, np.float64), 1.0)) * 1024.0).astype(np.int32)


def counts(desc, words):
    """term counts [W] int64 of one frame"""
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    if len(desc) == 0:
        return np.zeros(len(words), np.int64)
    return np.bincount(quantise(desc, words), minlength=len(words)).astype(np.int64)


def distance(qc, kc, weights):
    """(D, |q|, |k|) of two count vectors, int64 (Python ints)"""
    w = np.asarray(weights, np.int64)
    q, k = np.asarray(qc, np.int64) * w, np.asarray(kc, np.int64) * w
    nq, nk = int(q.sum()), int(k.sum())
    return int(np.abs(q * nk - k * nq).sum()), nq, nk


def score(qc, kc, weights):
    D, nq, nk = distance(qc, kc, weights)
    if nq == 0 or nk == 0:
        return 0.0
    return float(np.float64(1.0) - np.float64(0.5) * np.float64(D) / (np.float64(nq) * np.float64(nk)))


def query(q_desc, kf_desc, words, weights, n_best, kf_counts=None):
    """(positions, scores) of the keyframes with score > 0, highest first, ties to the lower position, at most n_best"""
    qc = counts(q_desc, words)
    kc = kf_counts if kf_counts is not None else [counts(d, words) for d in kf_desc]
    s = [score(qc, c, weights) for c in kc]
    pos = [k for k in range(len(s)) if s[k] > 0.0]
    pos.sort(key=lambda k: (-s[k], k))
    pos = pos[:max(int(n_best), 0)]
    return pos, [s[k] for k in pos]


def brute_force_candidates(q_desc, kf_desc, obs_off, obs_kf, obs_kp, ratio=0.75, max_candidates=4, tab=None):
    """mo_map_relocalize's candidate list and scores |C_k| (tests/reloc_restatement.py's rules, its Hamming loop replaced by the matmul)"""
    from tests import reloc_restatement as RR
    if tab is None:
        tab = RR.point_of(obs_off, obs_kf, obs_kp, [len(d) for d in kf_desc])
    scores = []
    for k, td in enumerate(kf_desc):
        d = hamming(q_desc, td)
        order = np.argsort(d, axis=1, kind="stable")[:, :2]   # stable: ties to the lower train index
        r = np.arange(len(d))
        d0, d1 = d[r, order[:, 0]], d[r, order[:, 1]]
        keep = d0.astype(np.float64) < ratio * d1.astype(np.float64)
        scores.append(int((keep & (tab[k][order[:, 0]] >= 0)).sum()))
    return RR.rank(scores, max_candidates), scores, tab
