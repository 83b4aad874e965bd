"""Generate tests/golden/s2t.npz from the REAL reference functions of tricolo/evaluation/eval_retrieval.py, called in the shape -> text
direction its own comments mark (`# change text_em and shape_em`, `# change labels and fit_labels`).  TEST INFRASTRUCTURE.

Runs only where the reference checkout is present (oracle.make_golden.REF); the fixture travels, the reference does not.

    python tools/make_s2t_golden.py

eval_retrieval.py imports jsonlines, which only its nearest.jsonl writer uses: the module is loaded with an empty stub in its place.
Called: compute_nearest_neighbors(text, shape, 5) - the captions are the fitted side, the shapes ask - and
compute_pr_at_k(indices, sort_indices, arange(Ns), 5, Ns, caption_labels).

Inputs: NS unit shape rows of width D, 1 to 7 captions each, a caption = its shape's row + Gaussian noise of NOISE / sqrt(D) per
component, all float32 values; the captions are shuffled and the shapes then numbered in order of their first caption, which is the
numbering compute_metrics gives them.  Two conditions on the fixture (not measurements of any code under test): the reference's
argsort is not stable, so no query may have two similarities closer than MIN_GAP; and the metrics must not be saturated - RR@1 in
[0.3, 0.8] and MRR < 0.9 - or a wrong ranking would score like a right one.

Written: text, shape, caption_labels; precision, recall, recall_rate, ndcg (five numbers each), mrr; indices [Ns, 5]; first_hit [Ns],
the position of the first correct caption in the reference's full ordering.
"""
import importlib.util
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import make_golden as mg            # noqa: E402

NS, D, K, SEED, NOISE, MIN_GAP = 48, 64, 5, 20, 3.5, 1e-9


def load_reference_module():
    sys.modules["jsonlines"] = types.ModuleType("jsonlines")
    spec = importlib.util.spec_from_file_location("reference_eval_retrieval", os.path.join(mg.REF, "tricolo", "evaluation", "eval_retrieval.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_inputs():
    rng = np.random.default_rng(SEED)
    shape = rng.standard_normal((NS, D))
    shape = (shape / np.linalg.norm(shape, axis=1, keepdims=True)).astype(np.float32)
    owner = np.repeat(np.arange(NS), rng.integers(1, 8, NS))
    owner = owner[rng.permutation(len(owner))]
    text = (shape[owner] + NOISE / np.sqrt(D) * rng.standard_normal((len(owner), D))).astype(np.float32)
    # number the shapes by their first caption (construct_embeddings_matrix's rule)
    first = {}
    for s in owner:
        first.setdefault(int(s), len(first))
    labels = np.array([first[int(s)] for s in owner], dtype=np.int64)
    new_shape = np.empty_like(shape)
    for old, new in first.items():
        new_shape[new] = shape[old]
    return text, new_shape, labels


def main():
    ref = load_reference_module()
    text, shape, labels = make_inputs()
    ns, nt = shape.shape[0], text.shape[0]
    assert list(dict.fromkeys(labels.tolist())) == list(range(ns))
    t64, s64 = text.astype(np.float64), shape.astype(np.float64)
    gaps = np.diff(np.sort(s64 @ t64.T, axis=1), axis=1)
    assert gaps.min() >= MIN_GAP, f"two similarities of one query {gaps.min():.3g} apart: the reference's argsort is not stable"
    distances, indices, sort_indices = ref.compute_nearest_neighbors(t64, s64, K)
    m = ref.compute_pr_at_k(indices, sort_indices, np.arange(ns), K, ns, labels)
    first_hit = np.array([list(labels[sort_indices[q]]).index(q) for q in range(ns)], dtype=np.int64)
    assert abs(float(np.mean(1.0 / (first_hit + 1))) - float(m["mrr"])) < 1e-12
    rr1, mrr = float(m["recall_rate"][0]), float(m["mrr"])
    assert 0.3 <= rr1 <= 0.8 and mrr < 0.9, f"saturated or degenerate fixture: RR@1 {rr1:.3f} MRR {mrr:.3f}"
    path = os.path.join(mg.GOLD, "s2t.npz")
    np.savez_compressed(path, text=text, shape=shape, caption_labels=labels, precision=np.asarray(m["precision"], dtype=np.float64),
                        recall=np.asarray(m["recall"], dtype=np.float64), recall_rate=np.asarray(m["recall_rate"], dtype=np.float64),
                        ndcg=np.asarray(m["ndcg"], dtype=np.float64), mrr=np.float64(m["mrr"]), indices=np.asarray(indices, dtype=np.int64),
                        first_hit=first_hit)
    print(f"{ns} shapes, {nt} captions, smallest gap {gaps.min():.3g}; RR@1 {rr1:.3f} RR@5 {float(m['recall_rate'][4]):.3f} "
          f"NDCG@5 {float(m['ndcg'][4]):.3f} MRR {mrr:.3f}")
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
