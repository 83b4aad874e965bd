"""Shape -> text retrieval: inputs and the float64 numpy reference of tests/test_s2t_cpu.py and tests/test_gpu_s2t.py.

A shape asks for captions and several captions are correct: a query names a CLASS, a candidate belongs to one (or to none).  The order
is the one of tests/head_reference.py: float64 dot products, larger first, equal similarities with the HIGHER candidate index first;
first_hit[q] is the position of the first candidate of the query's class in that order, -1 when there is none.

class_int_inputs makes every similarity an integer below 2^24 (|query| <= 2, |candidate| <= 3, D <= 4096: |sim| <= 24,576), exact in
float64 and float32 in any summation order, so a kernel must return indices, similarities and first_hit EQUAL to class_reference.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "s2t.npz")

# (Nq, Nc, D, k) at the edges of the gallery kernel's tiles: 8 / 4 / 2 / 1 queries per workgroup for D <= 512 / 1024 / 2048 / 4096, four
# waves of two candidate rows each = 8 rows per trip
CASES = [(7, 15, 64, 5), (9, 17, 64, 5),          # one side and the other of the 8-query tile and the 8-rows-per-trip step
         (3, 9, 520, 3), (5, 7, 1024, 3),         # the 4-query tile
         (1, 10, 1030, 2),                        # the 2-query tile
         (2, 9, 2049, 2),                         # the 1-query tile
         (64, 400, 80, 5), (33, 257, 68, 8),
         (5, 64, 130, 64), (17, 65, 4, 64),       # k at the limit of 64, D % 64 != 0 and D < 64
         (40, 1000, 36, 5)]


def class_int_inputs(Nq, Nc, D, seed=None):
    """-> (query [Nq,D] f32, cand [Nc,D] f32, query_class [Nq] i32 = 0..Nq-1, cand_class [Nc] i32).  Three quarters of the queries are
    distinct integer rows from {-2..2}, the rest copies of them; a candidate's class is drawn from [1, Nq) (class 0 is empty whenever
    Nq > 1: a query with no relevant candidate); the first Nc - Nc // 4 candidates are the query row of their class plus noise from
    {-1..1}, the last Nc // 4 exact copies of earlier candidates that keep their OWN drawn class - so a best relevant candidate often
    ties with a non-relevant one."""
    rng = np.random.default_rng(104729 * Nq + 7919 * Nc + D if seed is None else seed)
    nb = max(1, (3 * Nq + 3) // 4)
    base = rng.integers(-2, 3, (nb, D))
    query = np.concatenate([base, base[rng.integers(0, nb, Nq - nb)]], axis=0)
    cand_class = rng.integers(1 if Nq > 1 else 0, Nq, Nc)
    nfresh = Nc - Nc // 4
    fresh = query[cand_class[:nfresh]] + rng.integers(-1, 2, (nfresh, D))
    src = rng.integers(0, nfresh, Nc // 4)
    cand = np.concatenate([fresh, fresh[src]], axis=0)
    return query.astype(np.float32), cand.astype(np.float32), np.arange(Nq, dtype=np.int32), cand_class.astype(np.int32)


def skewed_inputs():
    """Nq = 4, Nc = 600, D = 64, k = 5 with 500 candidates in class 1 (a class far longer than a wave), 40 / 30 in classes 2 / 3, 30 in
    no class (-1) and class 0 empty.  Integer-valued like class_int_inputs; every fifth candidate of class 1 is a copy of the one
    before it, so the best of the class is reached through ties."""
    rng = np.random.default_rng(600)
    Nq, Nc, D, k = 4, 600, 64, 5
    query = rng.integers(-2, 3, (Nq, D))
    query[2] = query[1]                               # queries 2 and 3 look like query 1, whose 500 captions crowd in before their own
    query[3, 8:] = query[1, 8:]
    cand_class = np.concatenate([np.full(500, 1), np.full(40, 2), np.full(30, 3), np.full(30, -1)])
    cand_class = cand_class[rng.permutation(Nc)]
    cand = query[np.maximum(cand_class, 0)] + rng.integers(-1, 2, (Nc, D))
    ones = np.flatnonzero(cand_class == 1)
    cand[ones[4::5]] = cand[ones[3::5]]
    return (query.astype(np.float32), cand.astype(np.float32), np.arange(Nq, dtype=np.int32), cand_class.astype(np.int32)), k


def class_order(query, cand):
    """-> (sims [Nq,Nc] f64, order [Nq,Nc]): every candidate, best first (a stable ascending argsort, flipped)."""
    sims = query.astype(np.float64) @ cand.astype(np.float64).T
    return sims, np.argsort(sims, axis=1, kind="stable")[:, ::-1]


def class_reference(query, cand, query_class, cand_class, k):
    """-> (top [Nq,k] int64, top_sims [Nq,k] f64, first_hit [Nq] int64)."""
    sims, order = class_order(query, cand)
    top = order[:, :k]
    rel = np.asarray(cand_class)[order] == np.asarray(query_class)[:, None]
    first_hit = np.where(rel.any(axis=1), rel.argmax(axis=1), -1).astype(np.int64)
    return top.astype(np.int64), np.take_along_axis(sims, top, axis=1), first_hit


def class_csr_reference(cand_class, ncls=None):
    """The grouping rule of ops.class_csr, restated (ops needs the library to import): (class_off [ncls + 1], class_rows): the rows of
    class g are class_rows[class_off[g] : class_off[g + 1]], ascending; a negative class - or one not below ncls - joins no class."""
    cand_class = np.asarray(cand_class, dtype=np.int64)
    if ncls is None:
        ncls = max(int(cand_class.max()) + 1, 0) if cand_class.size else 0
    groups = [np.flatnonzero(cand_class == g) for g in range(ncls)]
    off = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32)
    rows = (np.concatenate(groups) if groups else np.zeros(0)).astype(np.int32)
    return off, rows


def tie_census(query, cand, query_class, cand_class):
    """What a case exercises: dict(no_relevant, max_first_hit, tie_higher, tie_lower, multi) - queries without a relevant candidate, the
    largest first_hit, queries whose best relevant candidate ties with a non-relevant one of higher / lower index, classes with more
    than one candidate."""
    sims, order = class_order(query, cand)
    rel = np.asarray(cand_class)[order] == np.asarray(query_class)[:, None]
    has = rel.any(axis=1)
    pos = rel.argmax(axis=1)
    higher = lower = 0
    for q in np.flatnonzero(has):
        b = order[q, pos[q]]
        tied = np.flatnonzero((sims[q] == sims[q, b]) & (np.asarray(cand_class) != query_class[q]))
        higher += bool((tied > b).any())
        lower += bool((tied < b).any())
    counts = np.bincount(np.asarray(cand_class)[np.asarray(cand_class) >= 0])
    return dict(no_relevant=int((~has).sum()), max_first_hit=int(np.where(has, pos, -1).max()), tie_higher=higher, tie_lower=lower,
                multi=int((counts > 1).sum()))


def golden():
    """tests/golden/s2t.npz (tools/make_s2t_golden.py): inputs and what the reference's own functions gave for them."""
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {name: z[name] for name in z.files}


def golden_tuples(g):
    """The per-caption tuples compute_metrics takes, from the golden inputs: caption i belongs to shape caption_labels[i].  The fixture
    numbers its shapes by their first caption, so compute_metrics rebuilds exactly its shape matrix and labels."""
    text, shape, lab = g["text"], g["shape"], g["caption_labels"]
    return [(None, "cat", f"model{int(lab[i]):03d}", text[i], shape[lab[i]]) for i in range(len(lab))]
