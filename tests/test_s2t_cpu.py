"""CPU: the shape -> text direction without a kernel - what the generator of tests/s2t_reference.py exercises, CaptionGallery's float64
torch restatement against class_reference, its labels against ShapeGallery's, storage, the CSR grouping rule, and compute_pr_at_k on
the fixture the REAL reference functions produced (tests/golden/s2t.npz, tools/make_s2t_golden.py)."""
import numpy as np
import pytest
import torch

from tests import s2t_reference as sr
from tricolo_amd.evaluation.gallery import CaptionGallery, ShapeGallery


def test_the_cases_exercise_what_they_are_meant_to():
    """The aggregates the integer cases were chosen for, asserted before any kernel is compared with them."""
    census = {case: sr.tie_census(*sr.class_int_inputs(*case[:3])) for case in sr.CASES}
    for case, c in census.items():
        assert (c["no_relevant"] > 0) == (case != (1, 10, 1030, 2)), case          # class 0 is empty whenever Nq > 1
        assert c["multi"] > 0, case                                                # classes with more than one candidate
    for case in ((64, 400, 80, 5), (40, 1000, 36, 5)):
        assert census[case]["max_first_hit"] >= case[3]                            # the first correct caption outside the top k
    assert sum(c["tie_higher"] > 0 for c in census.values()) == 7                  # best relevant tied with a non-relevant of higher index
    assert sum(c["tie_lower"] > 0 for c in census.values()) == 5                   # ... of lower index
    assert len(census) == 11 and census[(2, 9, 2049, 2)]["multi"] > 0
    (q, c, qc, cc), k = sr.skewed_inputs()
    assert q.shape == (4, 64) and c.shape == (600, 64) and k == 5 and int((cc == 1).sum()) == 500      # a class far longer than a wave
    hit = sr.class_reference(q, c, qc, cc, k)[2]
    assert hit[0] == -1 and hit.max() >= k
    for arrays in [sr.class_int_inputs(*case[:3]) for case in sr.CASES] + [(q, c, qc, cc)]:
        sims = arrays[0].astype(np.float64) @ arrays[1].astype(np.float64).T
        assert np.abs(sims).max() < 2**24 and np.array_equal(sims, np.rint(sims))


@pytest.mark.parametrize("case", sr.CASES + ["skewed"], ids=str)
def test_caption_gallery_equals_the_reference_on_integer_inputs(case):
    """CaptionGallery on CPU tensors: indices, similarities and first_hit EQUAL class_reference, ties and -1 included."""
    (q, c, qc, cc), k = sr.skewed_inputs() if case == "skewed" else (sr.class_int_inputs(*case[:3]), case[3])
    top, top_sims, first_hit = sr.class_reference(q, c, qc, cc, k)
    g = CaptionGallery(torch.from_numpy(c), cc)
    idx, sim, hit = g.rank(torch.from_numpy(q), qc, k=k)
    assert idx.dtype == torch.int64 and sim.dtype == torch.float64 and hit.dtype == torch.int64
    np.testing.assert_array_equal(idx.numpy(), top)
    np.testing.assert_array_equal(sim.numpy(), top_sims)
    np.testing.assert_array_equal(hit.numpy(), first_hit)
    idx2, sim2 = g.query(torch.from_numpy(q), k=k)
    assert torch.equal(idx2, idx) and torch.equal(sim2, sim)
    # a label no caption carries, below and above the classes in use
    odd = g.rank(torch.from_numpy(q), np.where(np.arange(len(qc)) % 2 == 0, -1, int(cc.max()) + 1), k=k)[2]
    assert (odd == -1).all()


def test_caption_gallery_arguments():
    q, c, qc, cc = sr.class_int_inputs(7, 15, 64)
    g = CaptionGallery(torch.from_numpy(c), cc)
    assert len(g) == 15 and g.num_classes == int(cc.max()) + 1 and g.device.type == "cpu"
    with pytest.raises(ValueError, match="1 <= k"):
        g.query(torch.from_numpy(q), k=16)
    with pytest.raises(ValueError, match="one shape label per query"):
        g.rank(torch.from_numpy(q), qc[:3], k=5)
    with pytest.raises(ValueError, match="queries must be"):
        g.query(torch.zeros(2, 65), k=5)
    with pytest.raises(ValueError, match="classes"):
        CaptionGallery(torch.from_numpy(c), cc[:4])
    with pytest.raises(ValueError, match="captions"):
        CaptionGallery(torch.from_numpy(c), cc, captions=["a"])


def test_both_galleries_agree_on_labels():
    """One set of per-caption tuples: a caption's class in the CaptionGallery is its label from ShapeGallery.from_captions - the gallery
    row of its shape -, under the model-id key and under the "Primitives" swap."""
    model_ids = ["a", "b", "a", "c", "b", "a"]
    cats = ["x", "y", "x", "x", "z", "y"]
    text = torch.arange(6 * 4, dtype=torch.float32).reshape(6, 4)
    shape = torch.arange(6 * 4, dtype=torch.float32).reshape(6, 4) * 0.5
    for dataset, want in ((None, [0, 1, 0, 2, 1, 0]), ("Primitives", [0, 1, 0, 0, 2, 1])):
        shapes, labels = ShapeGallery.from_captions(model_ids, cats, shape, dataset=dataset)
        captions = CaptionGallery.from_captions(model_ids, cats, text, dataset=dataset, captions=[f"caption {i}" for i in range(6)])
        assert captions.classes.tolist() == labels.tolist() == want
        assert captions.num_classes == len(shapes) and torch.equal(captions.embeddings, text)
        assert captions.model_ids == model_ids and captions.categories == cats and captions.captions[3] == "caption 3"
        # every shape's first correct caption, asked with the shape gallery's own rows
        hit = captions.rank(shapes.embeddings, torch.arange(len(shapes)), k=3)[2]
        order = torch.flip(torch.argsort(shapes.embeddings.double() @ text.double().t(), dim=1, stable=True), dims=(1,))
        assert hit.tolist() == [[int(labels[j]) for j in row].index(s) for s, row in enumerate(order.tolist())]
    with pytest.raises(ValueError, match="one entry per caption"):
        CaptionGallery.from_captions(model_ids[:5], cats, text)


def test_save_load_round_trip(tmp_path):
    q, c, qc, cc = sr.class_int_inputs(9, 17, 64)
    g = CaptionGallery(torch.from_numpy(c), cc, [f"m{j}" for j in cc], ["chair"] * 17, [f"a chair, number {i}" for i in range(17)])
    g.save(tmp_path / "captions.npz")
    h = CaptionGallery.load(tmp_path / "captions.npz")
    assert torch.equal(h.embeddings, g.embeddings) and torch.equal(h.classes, g.classes)
    assert (h.model_ids, h.categories, h.captions) == (g.model_ids, g.categories, g.captions)
    a, b = g.rank(torch.from_numpy(q), qc, k=5), h.rank(torch.from_numpy(q), qc, k=5)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    with np.load(tmp_path / "captions.npz", allow_pickle=False) as z:       # ShapeGallery's columns, one row per caption, plus two
        assert sorted(z.files) == ["captions", "categories", "classes", "embeddings", "model_ids"]
    bare = CaptionGallery(torch.from_numpy(c), cc)
    bare.save(tmp_path / "bare.npz")
    h = CaptionGallery.load(tmp_path / "bare.npz", device="cpu")
    assert h.model_ids is None and h.categories is None and h.captions is None and torch.equal(h.classes, bare.classes)


def test_csr_grouping_rule():
    """The rule ops.class_csr implements on the device, restated in class_csr_reference: rows grouped by class, ascending within one;
    a negative class joins none; an empty class has equal offsets."""
    cls = np.array([2, 0, -1, 2, 4, 0, 2, -3, 4])
    off, rows = sr.class_csr_reference(cls)
    assert off.tolist() == [0, 2, 2, 5, 5, 7] and rows.tolist() == [1, 5, 0, 3, 6, 4, 8]
    assert off.dtype == np.int32 and rows.dtype == np.int32
    off, rows = sr.class_csr_reference(cls, ncls=3)                                  # classes past an explicit ncls join none either
    assert off.tolist() == [0, 2, 2, 5] and rows.tolist() == [1, 5, 0, 3, 6]
    # the torch expression of ops.class_csr, written out here because ops does not import without the library
    cc = torch.from_numpy(cls)
    key = torch.where((cc >= 0) & (cc < 5), cc, torch.full_like(cc, 5))
    order = torch.argsort(key, stable=True)
    counts = torch.bincount(key, minlength=6)[:5]
    assert torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)]).tolist() == [0, 2, 2, 5, 5, 7]
    assert order[:7].tolist() == [1, 5, 0, 3, 6, 4, 8]
    for case in sr.CASES:
        cc = sr.class_int_inputs(*case[:3])[3]
        off, rows = sr.class_csr_reference(cc, ncls=case[0])
        assert off[-1] == len(cc) and all(sorted(rows[off[g]:off[g + 1]]) == np.flatnonzero(cc == g).tolist() for g in range(case[0]))


def test_compute_pr_at_k_reproduces_the_reference_on_the_golden_fixture():
    """tests/golden/s2t.npz holds what the reference's compute_nearest_neighbors(text, shape, 5) and compute_pr_at_k(indices,
    sort_indices, arange(Ns), 5, Ns, caption_labels) gave.  The CPU ranking of the same inputs fed to this package's compute_pr_at_k
    gives the same: indices equal, recall_rate exactly, precision / recall / ndcg / mrr within 1e-12 (the tolerances of the text ->
    shape golden test)."""
    from tricolo_amd.evaluation.eval_retrieval import compute_pr_at_k
    g = sr.golden()
    text, shape, labels = g["text"], g["shape"], g["caption_labels"]
    ns = shape.shape[0]
    assert text.dtype == np.float32 and shape.dtype == np.float32 and list(dict.fromkeys(labels.tolist())) == list(range(ns))
    assert 0.3 <= g["recall_rate"][0] <= 0.8 and g["mrr"] < 0.9                       # not saturated: a wrong ranking would show
    idx, sim, hit = CaptionGallery(torch.from_numpy(text), labels).rank(torch.from_numpy(shape), np.arange(ns), k=5)
    np.testing.assert_array_equal(idx.numpy(), g["indices"])
    np.testing.assert_array_equal(hit.numpy(), g["first_hit"])
    top, _, first_hit = sr.class_reference(shape, text, np.arange(ns), labels, 5)
    np.testing.assert_array_equal(top, g["indices"])
    np.testing.assert_array_equal(first_hit, g["first_hit"])
    m = compute_pr_at_k(idx.numpy(), hit.numpy(), np.arange(ns), 5, ns, labels)
    np.testing.assert_array_equal(m["recall_rate"], g["recall_rate"])
    for name in ("precision", "recall", "ndcg"):
        np.testing.assert_allclose(m[name], g[name], rtol=0, atol=1e-12)
    assert abs(m["mrr"] - float(g["mrr"])) <= 1e-12
