"""Constructed frame pairs for the tracking filters (k_track_select, reference matcher.py:109-169).

The filters only ever see what the matcher hands them, so a chosen match list has to be built out of descriptors: query i is a copy of
train row j(i) with exactly d_i bits flipped, and the train keypoint is the query keypoint plus a designed displacement.  A Case carries
the two frames, the call's free parameters (w, h, disp_frac - no image is involved) and the design: train index and best distance per
query.  Every builder checks with a brute-force Hamming 2-NN that the descriptors realise the design and redraws with another seed when
they do not; the gate builders also drop any input on which math.hypot is not the correctly rounded root of the exact sum of squares
(exact_hypot).  Tests never skip or redraw: they take all_cases() as it stands.

`kept` states the number of matches the two filters keep, per ratio setting (None = ratio test off, 0.75 = on), where the case was
designed to give a known count; it is written down by hand next to the case, not computed.
"""
import functools
import math
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np

RATIOS = (None, 0.75)
F32 = np.float32
IN_GATE = (1.5, -2.0)     # 2.5 px: inside every limit used below except where a case says otherwise
OUT_GATE = (30.0, 40.0)   # 50 px: outside


@dataclass
class Case:
    name: str
    xy1: np.ndarray            # (n1, 2) float32 query keypoints
    desc1: np.ndarray          # (n1, 32) uint8
    xy2: np.ndarray            # (n2, 2) float32 train keypoints
    desc2: np.ndarray          # (n2, 32) uint8
    w: int
    h: int
    disp_frac: float
    train: np.ndarray          # (n1,) designed nearest train row
    dist: np.ndarray           # (n1,) designed Hamming distance to it
    kept: dict = field(default_factory=dict)   # ratio -> stated number of kept matches
    gate: tuple = ()           # query indices whose displacement sits at the gate's edge (checked against exact arithmetic)
    gate_keep: tuple = ()      # what the reference decides for each of them
    tie_heavy: bool = False    # run twice in one context
    fresh: bool = False        # needs a context of its own (the row capacity follows the largest frame a context has seen)

    @property
    def limit(self):
        return ((self.w + self.h) / 2.0) * self.disp_frac


# ---- arithmetic ------------------------------------------------------------------------------------------------------------------
def exact_hypot(dx, dy):
    """The correctly rounded (nearest-even) double square root of the EXACT dx^2 + dy^2, by rational arithmetic and integer sqrt."""
    s = Fraction(float(dx)) ** 2 + Fraction(float(dy)) ** 2
    if s == 0:
        return 0.0
    e = 0   # scale so that sqrt(s) * 2^e lies in [2^52, 2^53)
    while s * Fraction(4) ** e < Fraction(2) ** 104:
        e += 1
    while s * Fraction(4) ** e >= Fraction(2) ** 106:
        e -= 1
    v = s * Fraction(4) ** e
    k = math.isqrt(v.numerator // v.denominator)          # floor(sqrt(v))
    half = Fraction(k) ** 2 + k + Fraction(1, 4)          # (k + 1/2)^2
    if v > half or (v == half and k & 1):
        k += 1
    return float(Fraction(k) / Fraction(2) ** e) if e >= 0 else float(k * 2 ** (-e))


def brute_knn2(desc1, desc2):
    """numpy brute-force Hamming 2-NN with BFMatcher's tie order (lowest train index first) -> idx (n1, 2), dist (n1, 2) int32;
    a missing neighbour is (-1, INT32_MAX)"""
    a = np.unpackbits(desc1, axis=1).astype(np.float32)
    b = np.unpackbits(desc2, axis=1).astype(np.float32)
    d = (a.sum(1)[:, None] + b.sum(1)[None, :] - 2.0 * (a @ b.T)).astype(np.int32)   # exact: integers below 2^24
    n1, n2 = d.shape
    idx = np.full((n1, 2), -1, np.int32)
    dist = np.full((n1, 2), np.iinfo(np.int32).max, np.int32)
    r = np.arange(n1)
    idx[:, 0] = d.argmin(1)
    dist[:, 0] = d[r, idx[:, 0]]
    if n2 > 1:
        d[r, idx[:, 0]] = 1 << 20
        idx[:, 1] = d.argmin(1)
        dist[:, 1] = d[r, idx[:, 1]]
    return idx, dist


def _pack(bits):
    return np.packbits(bits.astype(np.uint8), axis=1)


def _flip(rows_bits, d, rng):
    """every row with exactly d[i] of its 256 bits flipped"""
    rank = rng.random((len(d), 256)).argsort(1).argsort(1)
    return rows_bits ^ (rank < np.asarray(d)[:, None])


# ---- builders --------------------------------------------------------------------------------------------------------------------
def _frames(name, d, rng, gated=None, train_rows="random", w=640, h=480, frac=0.02, disp=None, xy1=None, extra=3, **kw):
    """One candidate frame pair for the distances d (query order).  gated: bool mask of the queries pushed outside the displacement
    limit.  train_rows: 'random' (n1 + extra random rows, every query its own), 'single' (nt == 1) or 'zero_one' (nt == 2: all zeros, all
    ones).  disp: (n1, 2) designed displacements (default IN_GATE / OUT_GATE by `gated`); xy1: query keypoints (default random)."""
    d = np.asarray(d, np.int32)
    n1 = len(d)
    gated = np.zeros(n1, bool) if gated is None else np.asarray(gated, bool)
    if train_rows == "random":
        n2 = n1 + extra
        tb = rng.integers(0, 2, (n2, 256)).astype(bool)
        train = rng.permutation(n2)[:n1].astype(np.int32)
    elif train_rows == "single":
        n2 = 1
        tb = rng.integers(0, 2, (1, 256)).astype(bool)
        train = np.zeros(n1, np.int32)
    else:
        n2 = 2
        tb = np.stack([np.zeros(256, bool), np.ones(256, bool)])
        train = np.zeros(n1, np.int32)
    desc1 = _pack(_flip(tb[train], d, rng)) if n1 else np.zeros((0, 32), np.uint8)
    if disp is None:
        disp = np.where(gated[:, None], np.array(OUT_GATE), np.array(IN_GATE))
    disp = np.asarray(disp, np.float64).reshape(n1, 2)
    if xy1 is None:
        xy1 = np.stack([rng.uniform(40, 600, n1), rng.uniform(40, 440, n1)], 1)
    xy1 = np.asarray(xy1, F32).reshape(n1, 2)
    if n2 >= n1:   # train keypoint = query keypoint + displacement
        xy2 = np.stack([rng.uniform(0, 640, n2), rng.uniform(0, 480, n2)], 1).astype(F32)
        xy2[train] = (xy1.astype(np.float64) + disp).astype(F32)
    else:          # a handful of train rows shared by all queries: the query keypoint moves instead
        xy2 = np.stack([rng.uniform(100, 500, n2), rng.uniform(100, 400, n2)], 1).astype(F32)
        xy1 = (xy2[train].astype(np.float64) - disp).astype(F32)
    return Case(name, xy1, desc1, xy2, _pack(tb), w, h, frac, train, d, **kw)


def realised(c):
    if len(c.dist) == 0:
        return True
    idx, dist = brute_knn2(c.desc1, c.desc2)
    return np.array_equal(idx[:, 0], c.train) and np.array_equal(dist[:, 0], c.dist)


def _build(name, d, seed, **kw):
    for attempt in range(8):   # (a design with distances up to 40 among random rows practically always holds at the first draw)
        c = _frames(name, d, np.random.default_rng(seed + 1000 * attempt), **kw)
        if realised(c):
            return c
    raise AssertionError("case %s: no seed realises the design" % name)


def _interleaved_gate(n1, n, rng, force=()):
    """bool mask with exactly n1 - n gated-out queries spread over the whole index range; `force` indices always survive"""
    g = np.ones(n1, bool)
    force = [i for i in force if i < n1]
    g[force] = False
    rest = np.setdiff1d(np.arange(n1), force)
    g[rng.choice(rest, n - len(force), replace=False)] = False
    return g


def _median_cases():
    out = []
    add = lambda name, d, kept, seed, **kw: out.append(_build(name, d, seed, kept={None: kept, 0.75: kept}, **kw))
    add("n1_d0", [0], 0, 1)                                   # median 0, 0 < 0 fails
    add("n1_d5", [5], 1, 2)                                   # median 5, 5 < 10
    add("n2_1_3", [1, 3], 2, 3)                               # median 2, both < 4
    add("n2_0_5", [0, 5], 1, 4)                               # median 2.5, 5 < 5 fails
    add("odd_integer_median", [9, 3, 4, 1, 9], 3, 5)          # sorted 1 3 4 9 9: median 4, keeps 1 3 4
    add("even_half_median", [12, 1, 7, 3, 11, 4, 1, 8], 6, 6)  # sorted 1 1 3 4 | 7 8 11 12: median 5.5, 11 < 11 fails
    add("even_half_median_3_4", [4, 2, 3, 5, 1, 6], 6, 7)     # sorted 1 2 3 | 4 5 6: median 3.5, all < 7
    add("equal_to_threshold", [1, 2, 1, 1], 3, 8)             # median 1, 2 < 2 fails
    add("majority_zero_odd", [0, 5, 0, 9, 0], 0, 9)           # identical frames: median 0 keeps nothing
    add("majority_zero_even", [0, 0, 3, 0, 7, 0], 0, 10)
    add("all_equal_17", [17] * 100, 100, 11, tie_heavy=True)  # everything, in query order
    add("nt1_all_256", [256] * 70, 70, 12, train_rows="single", tie_heavy=True)   # threshold 512: bin 256, ballot bit 8, the clamp
    rng = np.random.default_rng(13)
    add("nt1_129_to_256", rng.permutation(np.arange(129, 257)), 128, 13, train_rows="single")   # median 192.5, all < 385
    # 172 x 100 and 129..256 once each: median 100, keeps the 172 and 129..199 (71 values)
    add("nt1_spread_cut", rng.permutation(np.r_[[100] * 172, np.arange(129, 257)]), 243, 14, train_rows="single")
    # nt == 2 (zeros, ones): second distance 256 - d.  Ratio off: 0..128 once each, median 64, keeps 0..127.  Ratio 0.75 passes
    # d < 0.75 (256 - d), i.e. d <= 109: median 54.5, keeps 0..108
    out.append(_build("nt2_0_to_128", rng.permutation(np.arange(0, 129)), 15, train_rows="zero_one", kept={None: 128, 0.75: 109}))
    return out


def _placement_cases():
    out = []
    i = np.arange(3000)
    all_ = {None: 3000, 0.75: 3000}
    out.append(_build("waves_4_5_6_7", 4 + i % 4, 21, kept=all_, tie_heavy=True))          # median 5.5: all kept; one value per wave
    out.append(_build("wave0_8_12_16_20", 8 + 4 * (i % 4), 22, kept=all_, tie_heavy=True))  # median 14: all kept; bits 2..4 only
    rng = np.random.default_rng(23)
    d = rng.choice([4, 5, 6, 7, 8, 12, 16, 20], 3000)
    out.append(_build("mixed_ties_gated", d, 23, gated=_interleaved_gate(3000, 1700, rng), tie_heavy=True))
    # runs of one distance over exactly 64, 65 and 128 consecutive survivors, at offsets that are no multiple of 64, with gated-out
    # queries inside the runs (consecutive among the survivors, not among the queries); median 9: all 282 kept
    d, g = [], []
    for val, run in ((3, 5), (9, 64), (4, 3), (9, 65), (2, 7), (9, 128), (5, 10)):
        for k in range(run):
            d.append(val); g.append(False)
            if k % 5 == 2:
                d.append(1); g.append(True)
    out.append(_build("runs_64_65_128", d, 24, gated=g, kept={None: 282, 0.75: 282}, tie_heavy=True))
    return out


def _size_cases():
    out = []
    for n in (0, 1, 63, 64, 65, 255, 256, 257):
        rng = np.random.default_rng(300 + n)
        n1 = 2 * n + 7
        out.append(_build("survivors_%d" % n, rng.choice([3, 4, 5, 6, 9, 11], n1), 300 + n, gated=_interleaved_gate(n1, n, rng),
                          kept={None: 0, 0.75: 0} if n == 0 else {}))
    for n1 in (1, 1023, 1024, 1025, 2049):
        rng = np.random.default_rng(400 + n1)
        edge = (0, 1022, 1023, 1024, 1025, 2047, 2048)
        n = max(1, (n1 * 3) // 5)
        out.append(_build("queries_%d" % n1, rng.choice([3, 4, 5, 6, 9, 11], n1), 400 + n1, gated=_interleaved_gate(n1, n, rng, edge),
                          kept={None: 1, 0.75: 1} if n1 == 1 else {}))
    return out


def _capacity_cases():
    out = []
    for n1 in (5984, 6000, 6016):   # both frames n1 rows, so the row capacity is n1: LDS keys up to 6000 rows, the HBM scratch beyond
        rng = np.random.default_rng(500 + n1)
        out.append(_build("capacity_%d" % n1, rng.choice([4, 5, 6, 7, 8, 9, 12, 16, 20], n1), 500 + n1,
                          gated=_interleaved_gate(n1, (n1 * 2) // 3, rng), extra=0, tie_heavy=True, fresh=True))
    return out


# ---- the displacement gate -------------------------------------------------------------------------------------------------------
def solve_limit(target):
    """integers w, h and a double disp_frac with ((w + h) / 2.0) * disp_frac == target exactly"""
    for wh in range(80, 4000):
        s = wh / 2.0
        f = target / s
        for cand in (f, math.nextafter(f, 0.0), math.nextafter(f, math.inf)):
            if s * cand == target:
                return wh // 2, wh - wh // 2, cand
    raise AssertionError("no (w, h, disp_frac) gives the limit %r" % target)


def _gate_case(name, pts, seed, w, h, frac, filler=16):
    """pts: list of ((x1, y1), (x2, y2)) float32 coordinates whose displacement sits at the edge of the limit.  They get the distances
    3, 4, 5, ... (so the kept list names them) among `filler` matches of distance 9 well inside the gate: the median is 9 and the
    second filter keeps everything the gate lets through."""
    rng = np.random.default_rng(seed)
    n1 = len(pts) + filler
    slots = np.sort(rng.choice(n1, len(pts), replace=False))
    d = np.full(n1, 9, np.int32)
    d[slots] = 3 + np.arange(len(pts)) % 5
    xy1 = np.stack([rng.uniform(40, 600, n1), rng.uniform(40, 440, n1)], 1).astype(F32)
    disp = np.tile(np.array(IN_GATE), (n1, 1))
    for s, (a, b) in zip(slots, pts):
        xy1[s] = a
    for attempt in range(8):
        c = _frames(name, d, np.random.default_rng(seed + 1000 * attempt), w=w, h=h, frac=frac, disp=disp, xy1=xy1)
        for s, (a, b) in zip(slots, pts):
            c.xy2[c.train[s]] = b   # the designed float32 coordinates themselves, not a rounded sum
        if realised(c):
            break
    else:
        raise AssertionError("case %s: no seed realises the design" % name)
    keep = []
    for s in slots:
        dx = float(c.xy2[c.train[s], 0]) - float(c.xy1[s, 0]); dy = float(c.xy2[c.train[s], 1]) - float(c.xy1[s, 1])
        assert math.hypot(dx, dy) == exact_hypot(dx, dy), "case %s: math.hypot is not correctly rounded on (%r, %r)" % (name, dx, dy)
        keep.append(math.hypot(dx, dy) <= c.limit)
    c.gate, c.gate_keep = tuple(int(s) for s in slots), tuple(keep)
    c.kept = {None: filler + sum(keep), 0.75: filler + sum(keep)}
    return c


def _f32(v):
    return float(F32(v))


def _gate_cases():
    out = []
    up = lambda v: _f32(np.nextafter(F32(v), F32(np.inf)))
    # limit exactly 10.0: (6, 8) and (-8, 6) and (10, 0) lie on it, (6, 8 + 2^-20) and (0, 10 + ulp) just outside
    pts = [((0, 0), (6, 8)), ((0, 0), (6, 8 + 2.0 ** -20)), ((8, 0), (0, 6)), ((0, 0), (10, 0)), ((0, 0), (0, up(10.0)))]
    c = _gate_case("gate_limit_10", pts, 601, 24, 16, 0.5)
    assert c.limit == 10.0 and c.gate_keep == (True, False, True, True, False)
    out.append(c)
    # the shipping limit 560 * 0.02 is no float32: one float32 step either side of it, along both axes and both signs
    lim = 560 * 0.02
    lo = _f32(lim) if _f32(lim) <= lim else _f32(np.nextafter(F32(lim), F32(0)))
    hi = up(lo)
    assert lo <= lim < hi
    pts = [((100, 100), (100, 100 + lo)), ((100, 100), (100, 100 + hi)), ((100, 100), (100 + lo, 100)), ((100, 100), (100 + hi, 100)),
           ((100 + hi, 50), (100, 50)), ((0, 0), (0, lo)), ((0, 0), (hi, 0))]
    pts = [p for p in pts if all(_f32(v) == v for xy in p for v in xy)]   # (100 + lo is only used where it is a float32)
    pts += [((0, 0), (0, lo)), ((0, 0), (0, hi)), ((0, 0), (lo, 0)), ((hi, 0), (0, 0))]
    c = _gate_case("gate_shipping_limit", pts, 602, 640, 480, 0.02)
    assert c.gate_keep[-4:] == (True, False, True, False)
    out.append(c)
    out += _disagreeing_cases()
    return out


def _disagreeing_cases():
    """float32 coordinate pairs (displacement below 20 px) on which the correctly rounded hypot and sqrt(dx*dx + dy*dy) of rounded
    products differ by one ulp, each with limits equal to the smaller and to the larger of the two values.  At the smaller limit the
    two formulas decide differently: 'ref_keeps' pairs have hypot below the naive root (the reference keeps, the naive root drops),
    'ref_drops' pairs the other way round.  Each pair comes with its three mirror images (x and y swapped, either sign flipped)."""
    rng = np.random.default_rng(603)
    n = 40000
    x1 = rng.uniform(0, 640, n).astype(F32); y1 = rng.uniform(0, 480, n).astype(F32)
    x2 = (x1 + rng.uniform(-13, 13, n).astype(F32)).astype(F32); y2 = (y1 + rng.uniform(-13, 13, n).astype(F32)).astype(F32)
    dx = x2.astype(np.float64) - x1.astype(np.float64); dy = y2.astype(np.float64) - y1.astype(np.float64)
    naive = np.sqrt(dx * dx + dy * dy)
    found = {"ref_keeps": [], "ref_drops": []}
    for i in np.nonzero(naive < 20.0)[0]:
        hyp = math.hypot(dx[i], dy[i])
        if hyp == naive[i] or hyp != exact_hypot(dx[i], dy[i]):
            continue
        kind = "ref_keeps" if hyp < naive[i] else "ref_drops"
        if len(found[kind]) < 2:
            found[kind].append((i, min(hyp, float(naive[i])), max(hyp, float(naive[i]))))
        if all(len(v) == 2 for v in found.values()):
            break
    out = []
    for kind, lst in found.items():
        assert len(lst) == 2
        for k, (i, small, large) in enumerate(lst):
            a, b = (float(x1[i]), float(y1[i])), (float(x2[i]), float(y2[i]))
            pts = [(a, b), ((a[1], a[0]), (b[1], b[0])), ((b[0], a[1]), (a[0], b[1])), ((a[1], b[0]), (b[1], a[0]))]
            for which, target in (("small", small), ("large", large)):
                w, h, frac = solve_limit(target)
                c = _gate_case("gate_%s_%d_limit_%s" % (kind, k, which), pts, 610 + 4 * k + (which == "large"), w, h, frac)
                assert c.limit == target
                assert c.gate_keep == ((kind == "ref_keeps" or which == "large"),) * 4
                out.append(c)
    return out


# ---- the two cases that go on into the two-view stage -----------------------------------------------------------------------------
def _pose_cases():
    """exactly 7 and exactly 8 kept matches, spread over the frame (tracker.py:234: fewer than 8 matches fail)"""
    out = []
    for n in (7, 8):
        rng = np.random.default_rng(700 + n)
        xy1 = np.stack([np.linspace(60, 580, n) + rng.uniform(-20, 20, n), rng.permutation(np.linspace(50, 430, n))], 1)
        disp = np.stack([rng.uniform(2, 5, n), rng.uniform(-1, 1, n)], 1)
        d = np.r_[np.full(n, 6), [40, 40]]   # two more matches beyond 2 x median = 12
        xy1 = np.r_[xy1, [[300.0, 200.0], [320.0, 260.0]]]
        disp = np.r_[disp, [[1.0, 1.0], [1.0, -1.0]]]
        out.append(_build("pose_%d_kept" % n, d, 700 + n, xy1=xy1, disp=disp, kept={None: n, 0.75: n}))
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = _median_cases() + _placement_cases() + _size_cases() + _gate_cases() + _pose_cases() + _capacity_cases()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    return tuple(sorted(cases, key=lambda c: max(len(c.xy1), len(c.xy2))))   # (a shared context's row capacity only ever grows)


def case(name):
    return next(c for c in all_cases() if c.name == name)
