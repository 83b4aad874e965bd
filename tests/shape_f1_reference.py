"""Float64 restatement of the shape F1 (calculate_f1.py's _compute_sampling_metrics) and the seeded clouds of tests/golden/shape_f1.npz.
TEST INFRASTRUCTURE: numpy + scipy only, nothing here is imported by the package.

Clouds are points on the surfaces of a few random axis-aligned boxes (area-weighted), scaled like the reference's scale="gt-10"
(the ground truth's longest bounding-box edge becomes 10) and rounded to fp32.  Pair kinds: "unrelated" (two independent sets of
boxes), "near" (the prediction's boxes are the ground truth's jittered by 1 %, sampled independently) and "identical".
"""
import hashlib
from collections import namedtuple

import numpy as np
from scipy.spatial import cKDTree

THRESHOLDS = (0.1, 0.2, 0.3, 0.5)
D2_REL = 2.0 ** -21            # bound on the fp32 difference-form d2 against float64: five roundings of 2^-24 with headroom for FMA order
UNDECIDABLE_REL = 2.0 ** -20   # a point whose float64 distance is within this (times t) of fp32(t) may fall on either side in fp32
MAX_UNDECIDABLE = 2            # per pair and threshold, of the points of both directions: the generator rejects a seed above this


def _boxes(rng, k):
    return rng.random((k, 3)) * 2.0 - 1.0, 0.2 + 0.8 * rng.random((k, 3))


def _sample(centres, sizes, S, rng):
    """S points on the surfaces of the boxes, faces drawn with probability proportional to their area."""
    k = centres.shape[0]
    area = np.stack([sizes[:, 1] * sizes[:, 2], sizes[:, 0] * sizes[:, 2], sizes[:, 0] * sizes[:, 1]], axis=1)      # [k, 3]: faces normal to x, y, z
    cum = np.cumsum(np.repeat(area.reshape(-1), 2))
    face = np.minimum(np.searchsorted(cum, rng.random(S) * cum[-1], side="right"), 6 * k - 1)
    box, axis, side = face // 6, (face % 6) // 2, face % 2
    uvw = rng.random((S, 3)) - 0.5
    uvw[np.arange(S), axis] = side - 0.5
    return centres[box] + uvw * sizes[box]


def make_pair(kind, S_pred, S_gt, seed, boxes=3):
    """(pred [S_pred, 3], gt [S_gt, 3]) float32, scaled gt-10."""
    rng = np.random.default_rng(seed)
    c_gt, s_gt = _boxes(rng, boxes)
    gt = _sample(c_gt, s_gt, S_gt, rng)
    if kind == "unrelated":
        c_pr, s_pr = _boxes(rng, boxes)
        pred = _sample(c_pr, s_pr, S_pred, rng)
    elif kind == "near":
        c_pr = c_gt * (1.0 + 0.01 * (2.0 * rng.random(c_gt.shape) - 1.0))
        s_pr = s_gt * (1.0 + 0.01 * (2.0 * rng.random(s_gt.shape) - 1.0))
        pred = _sample(c_pr, s_pr, S_pred, rng)
    elif kind == "identical":
        assert S_pred == S_gt
        pred = gt.copy()
    else:
        raise ValueError(kind)
    scale = 10.0 / (gt.max(axis=0) - gt.min(axis=0)).max()
    return (pred * scale).astype(np.float32), (gt * scale).astype(np.float32)


def sha256(pred, gt):
    return hashlib.sha256(pred.tobytes() + gt.tobytes()).hexdigest()


def nn_exact(p, q):
    """Exact nearest neighbour of every row of p [S1, 3] among q [S2, 3] in float64: (d2 [S1] float64, idx [S1])."""
    p64, q64 = np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)
    _, idx = cKDTree(q64).query(p64, k=1)
    diff = p64 - q64[idx]
    return (diff * diff).sum(axis=1), idx.astype(np.int64)


def dist2_to(p, q, idx):
    """Float64 |p[i] - q[idx[i]]|^2."""
    diff = np.asarray(p, dtype=np.float64) - np.asarray(q, dtype=np.float64)[np.asarray(idx)]
    return (diff * diff).sum(axis=1)


Counts = namedtuple("Counts", "below undecidable")


def threshold_counts(d2_64, t):
    """Float64 count of decidable points with distance below fp32(t), and the number of undecidable points."""
    dist, t32 = np.sqrt(d2_64), float(np.float32(t))
    und = np.abs(dist - t32) <= UNDECIDABLE_REL * t
    return Counts(int(((dist < t32) & ~und).sum()), int(und.sum()))


def f1_fp32(count_p, len_p, count_q, len_q, eps=1e-8):
    """The reference's expression in numpy float32 (one rounding per operation, as torch evaluates it)."""
    f = np.float32
    precision = f(100.0) * (f(count_p) / f(len_p))
    recall = f(100.0) * (f(count_q) / f(len_q))
    with np.errstate(invalid="ignore", divide="ignore"):
        return precision, recall, (f(2.0) * precision * recall) / (precision + recall + f(eps))


def check_d2(d2, d2_64, what=""):
    """Condition 1: |d2 - d2_64| <= 2^-21 * d2_64 for every point; returns the largest relative error (in units of 2^-24)."""
    d2 = np.asarray(d2, dtype=np.float64)
    err = np.abs(d2 - d2_64)
    worst = float((err / np.maximum(d2_64, 1e-300)).max()) if d2_64.size else 0.0
    print(f"{what} d2: worst relative error {worst / 2.0 ** -24:.3f} x 2^-24 (bound 8 x 2^-24) over {d2_64.size} points")
    assert (err <= D2_REL * d2_64).all(), (what, worst)
    return worst


def check_counts(counts, d2_64, thresholds, what=""):
    """Condition 3: each count inside [decidable below, decidable below + undecidable]; returns the float64 Counts per threshold."""
    out = []
    for k, t in enumerate(thresholds):
        c = threshold_counts(d2_64, t)
        print(f"{what} t={t}: count {int(counts[k])}, float64 decidable {c.below}, undecidable {c.undecidable}")
        assert c.below <= int(counts[k]) <= c.below + c.undecidable, (what, t, int(counts[k]), c)
        out.append(c)
    return out
