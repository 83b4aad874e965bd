"""CPU: evaluation.gallery.ShapeGallery on host tensors (its float64 torch restatement of the ranking) against
tests/head_reference.py: retrieval_reference, the checkpoint key filter of tricolo_amd.test and the argument handling of the two
inference commands.  Nothing here launches a kernel."""
import numpy as np
import pytest
import torch

from tests import head_reference as hr
from tricolo_amd import config as tcfg
from tricolo_amd.evaluation.gallery import ShapeGallery

BASE = ["data=synthetic", "model.text_encoder=BiGRUEncoder", "experiment_name=gallery_cpu"]


def ids_of(n):
    return [f"m{i:05d}" for i in range(n)]


@pytest.mark.parametrize("case", hr.RETRIEVAL_INT, ids=str)
def test_rank_equals_the_reference_on_integer_inputs(case):
    """Integer similarities (exact in any summation order): indices, similarities and first_hit EQUAL retrieval_reference, ties
    (a third of the shape rows are copies) included."""
    Nq, Ns, D, k = case
    txt, shp, lab = hr.retrieval_int_inputs(Nq, Ns, D)
    top, top_sims, first_hit, _ = hr.retrieval_reference(txt, shp, lab, k)
    g = ShapeGallery(torch.from_numpy(shp), ids_of(Ns))
    idx, sim, names, hit = g.rank(torch.from_numpy(txt), lab, k=k)
    assert idx.dtype == torch.int64 and sim.dtype == torch.float64 and hit.dtype == torch.int64
    np.testing.assert_array_equal(idx.numpy(), top)
    np.testing.assert_array_equal(sim.numpy(), top_sims)
    np.testing.assert_array_equal(hit.numpy(), first_hit)
    assert names == [[f"m{j:05d}" for j in row] for row in top.tolist()]


def test_query_without_labels():
    Nq, Ns, D, k = hr.RETRIEVAL_INT[0]
    txt, shp, lab = hr.retrieval_int_inputs(Nq, Ns, D)
    g = ShapeGallery(torch.from_numpy(shp), ids_of(Ns))
    out = g.query(torch.from_numpy(txt), k=k)
    assert len(out) == 3
    ranked = g.rank(torch.from_numpy(txt), torch.from_numpy(lab), k=k)
    assert torch.equal(out[0], ranked[0]) and torch.equal(out[1], ranked[1]) and out[2] == ranked[2]
    with pytest.raises(ValueError, match="1 <= k"):
        g.query(torch.from_numpy(txt), k=Ns + 1)
    with pytest.raises(ValueError, match="label"):
        g.rank(torch.from_numpy(txt), np.full(Nq, Ns), k=k)
    with pytest.raises(ValueError, match="queries must be"):
        g.query(torch.zeros(2, D + 1), k=k)


def test_from_captions_first_occurrence_and_primitives_swap():
    """construct_embeddings_matrix's rule: the first row of a model id supplies the shape embedding; "Primitives" keys on the category."""
    from tricolo_amd.evaluation.eval_retrieval import construct_embeddings_matrix
    model_ids = ["a", "b", "a", "c", "b", "a"]
    cats = ["x", "y", "x", "x", "z", "y"]
    feats = torch.arange(6 * 4, dtype=torch.float32).reshape(6, 4)
    g, labels = ShapeGallery.from_captions(model_ids, cats, feats)
    assert g.model_ids == ["a", "b", "c"] and g.categories == ["x", "y", "x"]
    assert torch.equal(g.embeddings, feats[[0, 1, 3]]) and labels.tolist() == [0, 1, 0, 2, 1, 0]
    tuples = {"caption_embedding_tuples": [(None, cats[i], model_ids[i], np.zeros(4, np.float32), feats[i].numpy()) for i in range(6)]}
    for dataset in ("Text2ShapeChairTable", "Primitives"):
        _, shape, lab, _, _, _, label_to_id = construct_embeddings_matrix(dataset, tuples)
        g, labels = ShapeGallery.from_captions(model_ids, cats, feats, dataset=dataset)
        np.testing.assert_array_equal(g.embeddings.numpy(), shape)
        np.testing.assert_array_equal(labels, lab)
        assert g.model_ids == [label_to_id[i] for i in range(len(g))]
    assert g.model_ids == ["x", "y", "z"] and g.categories == ["a", "b", "b"]          # Primitives: id and category swapped
    with pytest.raises(ValueError, match="one entry per caption"):
        ShapeGallery.from_captions(model_ids[:5], cats, feats)


def test_save_load_round_trip(tmp_path):
    Nq, Ns, D, k = hr.RETRIEVAL_INT[2]
    txt, shp, lab = hr.retrieval_int_inputs(Nq, Ns, D)
    g = ShapeGallery(torch.from_numpy(shp), ids_of(Ns), ["chair" if i % 2 else "table" for i in range(Ns)])
    g.save(tmp_path / "gallery.npz")
    h = ShapeGallery.load(tmp_path / "gallery.npz")
    assert torch.equal(h.embeddings, g.embeddings) and h.model_ids == g.model_ids and h.categories == g.categories
    a, b = g.rank(torch.from_numpy(txt), lab, k=k), h.rank(torch.from_numpy(txt), lab, k=k)
    assert all(torch.equal(x, y) for x, y in zip((a[0], a[1], a[3]), (b[0], b[1], b[3]))) and a[2] == b[2]
    bare = ShapeGallery(torch.from_numpy(shp), ids_of(Ns))
    bare.save(tmp_path / "bare.npz")
    assert ShapeGallery.load(tmp_path / "bare.npz", device="cpu").categories is None
    with pytest.raises(ValueError, match="model ids"):
        ShapeGallery(torch.from_numpy(shp), ids_of(Ns - 1))


def test_select_checkpoint_keys():
    """A Tri(I+V) state dict under Bi(V), Bi(I) and Tri configs (the reference's test.py:21-27), CLIP-text weights dropped."""
    from tricolo_amd.test import select_checkpoint_keys
    sd = {k: torch.zeros(1) for k in ("text_encoder.embedding.weight", "text_encoder.clip_model.visual.proj", "image_encoder.net_1.0.weight",
                                      "image_encoder.net_2.0.bias", "voxel_encoder.mlp.0.weight", "voxel_encoder.conv1.weight")}
    img, vox = "model.image_encoder=MVCNNEncoder", "model.voxel_encoder=SparseCNNEncoder"
    text = ["text_encoder.embedding.weight"]
    image = ["image_encoder.net_1.0.weight", "image_encoder.net_2.0.bias"]
    voxel = ["voxel_encoder.mlp.0.weight", "voxel_encoder.conv1.weight"]
    assert list(select_checkpoint_keys(sd, tcfg.compose(overrides=BASE + [vox]))) == text + voxel
    assert list(select_checkpoint_keys(sd, tcfg.compose(overrides=BASE + [img]))) == text + image
    assert list(select_checkpoint_keys(sd, tcfg.compose(overrides=BASE + [img, vox]))) == text + image + voxel
    assert len(sd) == 6                                                                 # the checkpoint's own dict is left alone


def test_test_main_without_a_checkpoint_raises_the_reference_message(tmp_path):
    from tricolo_amd import test as inference
    args = BASE + ["model.voxel_encoder=SparseCNNEncoder"]
    with pytest.raises(FileNotFoundError, match="Error: Checkpoint path does not exists."):
        inference.main(args + [f"+ckpt_path={tmp_path / 'none.ckpt'}"])
    with pytest.raises(FileNotFoundError, match="Error: Checkpoint path does not exists."):
        inference.main(args)
    with pytest.raises(SystemExit, match="tricolo_amd.test reads"):
        inference.main(args + ["data.dataset=SomethingElse"])


def test_eval_parses_its_overrides(tmp_path):
    from tricolo_amd import eval as evaluate
    cfg, path, nearest = evaluate.parse(["data=synthetic", "+prediction_file_path=/some/output.p"])
    assert cfg.data.dataset == "Synthetic" and path == "/some/output.p" and nearest is None
    _, path, nearest = evaluate.parse(["data=synthetic", "+prediction_file_path=o.p", "+nearest_path=n.jsonl"])
    assert (path, nearest) == ("o.p", "n.jsonl")
    with pytest.raises(SystemExit, match="prediction_file_path"):
        evaluate.parse(["data=synthetic"])
    with pytest.raises(FileNotFoundError):
        evaluate.main(["data=synthetic", f"+prediction_file_path={tmp_path / 'missing.p'}"])
