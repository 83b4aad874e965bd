"""GPU: the shape -> text direction - tri_retrieval_classes (csrc/gallery.hip) through ops.retrieval_classes, CaptionGallery on the
device, compute_metrics(direction=...) and the test command with +inference.direction=both.  References and inputs:
tests/s2t_reference.py (integer-valued inputs make every similarity exact, so indices, similarities and first_hit must be EQUAL to the
float64 numpy ranking) and tests/golden/s2t.npz (what the reference's own functions gave, tools/make_s2t_golden.py); with one row per
class the entry point must return the very bytes of ops.retrieval_gallery."""
import contextlib
import io
import json
import pickle

import numpy as np
import pytest
import torch

from tests import head_reference as hr
from tests import s2t_reference as sr
from tests.guard_bands import POISON, ZERO, guarded_ops, same_bytes

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tricolo_amd import ops

DEV = "cuda"
NUMBERS = ("precision", "recall", "recall_rate", "ndcg")


def dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def csr_call(q, c, qc, off, rows, ncls, k):
    """ops.retrieval_classes_csr on host arrays -> host arrays."""
    idx, sim, hit = ops.retrieval_classes_csr(*dev(q, c, qc.astype(np.int32), off.astype(np.int32), rows.astype(np.int32)), ncls, k)
    return idx.cpu().numpy(), sim.cpu().numpy(), hit.cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. integer-exact cases
@pytest.mark.parametrize("case", sr.CASES + ["skewed"], ids=str)
def test_classes_ranking_integer_exact(case):
    """retrieval_gallery_kernel<QT, true> on integer similarities (exact in any order; a quarter of the candidates are copies that keep
    their own class, so ties between a best relevant candidate and a non-relevant one are exact too): idx, sim and first_hit EQUAL
    class_reference, -1 for the queries whose class is empty.  sr.CASES sit at the edges of the kernel's tiles
    (tests/test_s2t_cpu.py asserts what each exercises); "skewed" holds 500 of 600 candidates in one class: a pass over a class far
    longer than a wave."""
    (q, c, qc, cc), k = sr.skewed_inputs() if case == "skewed" else (sr.class_int_inputs(*case[:3]), case[3])
    top, top_sims, first_hit = sr.class_reference(q, c, qc, cc, k)
    idx, sim, hit = ops.retrieval_classes(*dev(q, c, qc, cc), k=k)
    assert idx.dtype == torch.int32 and sim.dtype == torch.float64 and hit.dtype == torch.int32
    np.testing.assert_array_equal(idx.cpu().numpy(), top)
    np.testing.assert_array_equal(sim.cpu().numpy(), top_sims)
    np.testing.assert_array_equal(hit.cpu().numpy(), first_hit)
    idx1, sim1, hit1 = ops.retrieval_classes(*dev(q, c), k=k)                   # the top k do not depend on the classes
    assert hit1 is None and torch.equal(idx1, idx) and same_bytes(sim1, sim)
    off, rows = sr.class_csr_reference(cc, ncls=int(cc.max()) + 1)               # the device CSR is the restated rule's
    off_d, rows_d, ncls = ops.class_csr(torch.from_numpy(cc).to(DEV))
    assert ncls == int(cc.max()) + 1 and off_d.dtype == torch.int32 and rows_d.dtype == torch.int32
    np.testing.assert_array_equal(off_d.cpu().numpy(), off)
    np.testing.assert_array_equal(rows_d.cpu().numpy()[:off[-1]], rows)


# ------------------------------------------------------------------------------------------------ 2. metamorphic
@pytest.mark.parametrize("case", [(16, 300, 512, 5), (33, 1486, 512, 5)], ids=str)
def test_identity_classes_return_the_bytes_of_retrieval_gallery(case):
    """One candidate per class (class_off = 0..Nc, class_rows = 0..Nc-1, query_class = label): idx, the raw bytes of sim and first_hit
    are those of ops.retrieval_gallery with label; a second run repeats the first bit for bit."""
    Nq, Ns, D, k = case
    txt, shp, lab = dev(*hr.retrieval_float_inputs(Nq, Ns, D))
    idx0, sim0, hit0 = ops.retrieval_gallery(txt, shp, lab, k=k)
    off = torch.arange(Ns + 1, dtype=torch.int32, device=DEV)
    rows = torch.arange(Ns, dtype=torch.int32, device=DEV)
    idx, sim, hit = ops.retrieval_classes_csr(txt, shp, lab, off, rows, Ns, k)
    print(f"CLASSES {case} idx_mismatch={int((idx != idx0).sum())} sim_mismatch={int((sim.view(torch.int64) != sim0.view(torch.int64)).sum())} "
          f"hit_mismatch={int((hit != hit0).sum())}")
    assert torch.equal(idx, idx0) and same_bytes(sim, sim0) and torch.equal(hit, hit0)
    idx1, sim1, hit1 = ops.retrieval_classes(txt, shp, lab, torch.arange(Ns, device=DEV), k=k)      # the same CSR, built by ops
    assert torch.equal(idx1, idx0) and same_bytes(sim1, sim0) and torch.equal(hit1, hit0)
    idx2, sim2, hit2 = ops.retrieval_classes_csr(txt, shp, lab, off, rows, Ns, k)
    assert torch.equal(idx2, idx) and same_bytes(sim2, sim) and torch.equal(hit2, hit)


def test_swapped_operands_at_the_val_split_size():
    """1,486 shapes ask 7,424 captions at D = 512, k = 5: idx and the bytes of sim are those of ops.retrieval_gallery(shape, text, None).
    A caption belongs to the shape it is closest to, except that every tenth shape trades its captions with its neighbour - so there are
    shapes whose first correct caption is the best, shapes whose first correct caption lies far outside the top k, and shapes with no
    caption.  first_hit EQUALS the float64 numpy ranking: the closest two similarities of any one shape are 4e-9 apart (asserted), the
    two float64 summation orders differ by 1e-13 at most, so both rank alike.  A second run repeats the first bit for bit."""
    Nt, Ns, D, k = 7424, 1486, 512, 5
    txt, shp, _ = hr.retrieval_float_inputs(Nt, Ns, D)
    sims, order = sr.class_order(shp, txt)
    assert np.diff(np.sort(sims, axis=1), axis=1).min() > 1e-10
    owner = np.argmax(sims, axis=0)
    traded = np.where(owner % 10 == 0, owner + 1, np.where(owner % 10 == 1, owner - 1, owner))
    qc = np.arange(Ns, dtype=np.int32)
    rel = traded[order] == qc[:, None]
    want = np.where(rel.any(axis=1), rel.argmax(axis=1), -1)
    assert (want == -1).any() and (want == 0).any() and (want >= k).any()        # all three kinds of query occur
    txt, shp, qc, traded = dev(txt, shp, qc, traded)
    idx0, sim0, _ = ops.retrieval_gallery(shp, txt, None, k=k)
    idx, sim, hit = ops.retrieval_classes(shp, txt, qc, traded, k=k, ncls=Ns)
    assert torch.equal(idx, idx0) and same_bytes(sim, sim0)
    np.testing.assert_array_equal(idx.cpu().numpy(), order[:, :k])
    np.testing.assert_array_equal(hit.cpu().numpy(), want)
    idx2, sim2, hit2 = ops.retrieval_classes(shp, txt, qc, traded, k=k, ncls=Ns)
    assert torch.equal(idx2, idx) and same_bytes(sim2, sim) and torch.equal(hit2, hit)


# ------------------------------------------------------------------------------------------------ 3. rejections and the -1 convention
def test_classes_rejections():
    """tri_retrieval_classes' argument checks are tri_retrieval_gallery's: 1 <= k <= min(Nc, 64), D <= 4096, first_hit only with the
    three class arguments; no queries is no work."""
    q, c, qc, cc = dev(*sr.class_int_inputs(4, 70, 68))
    for k in (0, 71):
        with pytest.raises(RuntimeError, match="tri_retrieval_classes: need 1 <= k <= number of shapes"):
            ops.retrieval_classes(q, c, qc, cc, k=k)
    with pytest.raises(RuntimeError, match="TRI_GALLERY_MAX_K"):
        ops.retrieval_classes(q, c, qc, cc, k=65)
    with pytest.raises(RuntimeError, match="D > 4096"):
        ops.retrieval_classes(torch.zeros(2, 4097, device=DEV), torch.zeros(9, 4097, device=DEV), k=5)
    with pytest.raises(ValueError, match="go together"):
        ops.retrieval_classes(q, c, qc, None, k=5)
    idx, sim, hit = torch.empty(4, 5, dtype=torch.int32, device=DEV), torch.empty(4, 5, dtype=torch.float64, device=DEV), torch.empty(4, dtype=torch.int32, device=DEV)
    off, rows, ncls = ops.class_csr(cc)
    for args in ((None, None, None), (qc, None, rows), (qc, off, None), (None, off, rows)):
        rc = ops.lib().tri_retrieval_classes(ops.ptr(q), ops.ptr(c), *(ops.ptr(a) for a in args), 4, 70, 68, ncls, 5, ops.ptr(idx), ops.ptr(sim),
                                             ops.ptr(hit), ops.stream())
        assert rc == -1 and b"first_hit needs query_class, class_off and class_rows" in ops.lib().tri_last_error()
    idx, sim, hit = ops.retrieval_classes(q[:0], c, qc[:0], cc, k=5)
    assert idx.shape == (0, 5) and sim.shape == (0, 5) and hit.shape == (0,)


def test_no_class_gives_minus_one_and_leaves_the_others_alone():
    """A query class of -1 or ncls, and an empty class, give first_hit -1; a class_rows entry of Nc (or a negative one) is skipped as if
    the candidate had no class.  Every other query keeps its result."""
    q, c, qc, cc = sr.class_int_inputs(9, 17, 64)
    k, ncls = 5, 9
    top, top_sims, want = sr.class_reference(q, c, qc, cc, k)
    assert want[0] == -1 and (want[1:] >= 0).sum() >= 4                          # class 0 is empty as generated
    off, rows = sr.class_csr_reference(cc, ncls=ncls)
    qc2 = qc.copy()
    live = np.flatnonzero(want >= 0)
    qc2[live[0]], qc2[live[1]] = -1, ncls
    idx, sim, hit = csr_call(q, c, qc2, off, rows, ncls, k)
    expect = want.copy()
    expect[live[:2]] = -1
    np.testing.assert_array_equal(hit, expect)
    np.testing.assert_array_equal(idx, top)
    np.testing.assert_array_equal(sim, top_sims)
    # knock the best candidate of one class, and another candidate of a second class, out of class_rows
    order = sr.class_order(q, c)[1]
    g1, g2 = int(live[2]), int(live[3])
    best = int(order[g1][np.argmax(cc[order[g1]] == g1)])
    other = int(np.flatnonzero(cc == g2)[-1])
    rows2, cc2 = rows.copy(), cc.copy()
    rows2[np.flatnonzero(rows == best)[0]] = 17
    rows2[np.flatnonzero(rows == other)[0]] = -5
    cc2[[best, other]] = -1
    idx, sim, hit = csr_call(q, c, qc, off, rows2, ncls, k)
    np.testing.assert_array_equal(hit, sr.class_reference(q, c, qc, cc2, k)[2])
    np.testing.assert_array_equal(idx, top)
    # ops.retrieval_classes: a negative candidate class is no class
    hit3 = ops.retrieval_classes(*dev(q, c, qc, cc2), k=k, ncls=ncls)[2]
    np.testing.assert_array_equal(hit3.cpu().numpy(), sr.class_reference(q, c, qc, cc2, k)[2])


# ------------------------------------------------------------------------------------------------ 4. guard bands
def test_classes_inside_guard_bands():
    """test_gallery_inside_guard_bands on the new entry point: Nq = 3, Nc = 37, D = 64, k = 5 with an exact tie between a relevant and
    a non-relevant candidate; every operand - the three CSR arrays included - and every output between poisoned bands, under 0xFF and
    0x00 fills with identical bytes."""
    rng = np.random.default_rng(3)
    c = rng.standard_normal((37, 64)).astype(np.float32)
    c[20] = c[7]                                                     # an exact tie
    q = c[[7, 36, 0]] + 0.01 * rng.standard_normal((3, 64)).astype(np.float32)
    cc = rng.integers(0, 3, 37).astype(np.int32)
    cc[7], cc[20], cc[36] = 0, 1, 1                                  # query 0: its best caption 7 ties with caption 20 of another class
    cc[cc == 2] = 3                                                  # query 2 (class 2) has no caption
    qc = np.arange(3, dtype=np.int32)
    off, rows = sr.class_csr_reference(cc, ncls=4)
    runs = []
    for fill in (POISON, ZERO):
        with guarded_ops(fill) as g:
            idx, sim, hit = ops.retrieval_classes_csr(*(g.put(torch.from_numpy(a)) for a in (q, c, qc, off, rows)), 4, k=5)
            out = dict(idx=idx.cpu(), sim=sim.cpu(), hit=hit.cpu())
        assert g.launched == ["tri_retrieval_classes"]
        runs.append(out)
    for name in runs[0]:
        assert same_bytes(runs[0][name], runs[1][name]), f"{name} depends on memory outside the operands"
    got = runs[0]
    top, top_sims, first_hit = sr.class_reference(q, c, qc, cc, 5)
    np.testing.assert_array_equal(got["idx"].numpy(), top)
    np.testing.assert_array_equal(got["hit"].numpy(), first_hit)
    np.testing.assert_allclose(got["sim"].numpy(), top_sims, rtol=1e-13, atol=1e-13)
    assert list(top[0, :2]) == [20, 7] and list(first_hit) == [1, 0, -1]        # the tie: higher index first, so the relevant one is second


# ------------------------------------------------------------------------------------------------ 5. metrics
def test_compute_metrics_s2t_reproduces_the_reference(tmp_path):
    """compute_metrics on tuples built from the golden inputs: direction="s2t" gives the numbers the reference's functions gave (indices
    equal, recall_rate exactly, precision / recall / ndcg / mrr within 1e-12); "both" is today's text -> shape dict plus "s2t";
    nearest_s2t.jsonl holds one record per shape, nearest.jsonl is the same file with and without the switch."""
    from tricolo_amd.evaluation.eval_retrieval import compute_metrics
    g = sr.golden()
    tuples = {"caption_embedding_tuples": sr.golden_tuples(g)}
    labels, ns = g["caption_labels"], g["shape"].shape[0]
    s2t = compute_metrics("Text2Shape", tuples, direction="s2t")
    np.testing.assert_array_equal(s2t["indices"], g["indices"])
    np.testing.assert_array_equal(s2t["recall_rate"], g["recall_rate"])
    for name in ("precision", "recall", "ndcg"):
        np.testing.assert_allclose(s2t[name], g[name], rtol=0, atol=1e-12)
    assert abs(s2t["mrr"] - float(g["mrr"])) <= 1e-12
    plain_dir, both_dir = tmp_path / "plain", tmp_path / "both"
    plain_dir.mkdir(), both_dir.mkdir()
    plain = compute_metrics("Text2Shape", tuples, nearest_path=str(plain_dir / "nearest.jsonl"))
    both = compute_metrics("Text2Shape", tuples, nearest_path=str(both_dir / "nearest.jsonl"), direction="both")
    assert sorted(plain) == ["indices", "mrr", "ndcg", "precision", "recall", "recall_rate"] and sorted(both) == sorted(plain) + ["s2t"]
    for name in NUMBERS + ("indices",):
        np.testing.assert_array_equal(both[name], plain[name])
        np.testing.assert_array_equal(both["s2t"][name], s2t[name])
    assert both["mrr"] == plain["mrr"] and both["s2t"]["mrr"] == s2t["mrr"]
    assert (both_dir / "nearest.jsonl").read_bytes() == (plain_dir / "nearest.jsonl").read_bytes()
    assert not (plain_dir / "nearest_s2t.jsonl").exists()
    with open(both_dir / "nearest_s2t.jsonl") as f:
        records = [json.loads(line) for line in f]
    assert len(records) == ns
    for s, rec in enumerate(records):
        assert rec["groundtruth"] == f"model{s:03d}" and rec["cat_id"] == "cat" and len(rec["distance"]) == 5
        assert rec["retrieved_captions"] == g["indices"][s].tolist()
        assert rec["retrieved_models"] == [f"model{int(labels[c]):03d}" for c in rec["retrieved_captions"]]
    with pytest.raises(ValueError, match="direction"):
        compute_metrics("Text2Shape", tuples, direction="t2t")


# ------------------------------------------------------------------------------------------------ 6. the test command
@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """tricolo_amd.test.main twice over the held-out set of data=synthetic from one checkpoint, made as tests/test_gpu_inference_cli.py
    makes its own: without the switch and with +inference.direction=both; what each printed and returned."""
    from tests.test_gpu_inference_cli import BIV
    from tricolo_amd import config as tcfg
    from tricolo_amd import test as inference
    from tricolo_amd.checkpoint import save_reference_checkpoint
    from tricolo_amd.model.tricolo_net import TriCoLoNet
    tmp = tmp_path_factory.mktemp("s2t_cli")
    torch.manual_seed(5)
    net = TriCoLoNet(tcfg.compose(overrides=BIV))
    ckpt = tmp / "biv.ckpt"
    save_reference_checkpoint(net, ckpt, epoch=3, global_step=40)
    out = {}
    for name, extra in (("plain", []), ("both", ["+inference.direction=both"])):
        printed = io.StringIO()
        with contextlib.redirect_stdout(printed):
            metrics = inference.main(BIV + [f"inference.output_dir={tmp / name}", f"+ckpt_path={ckpt}"] + extra)
        out[name] = dict(metrics=metrics, printed=printed.getvalue(), dir=tmp / name)
    return out


def test_command_prints_and_returns_the_s2t_numbers(runs):
    from tests.test_gpu_inference_cli import same_metrics
    from tricolo_amd.evaluation.gallery import CaptionGallery, ShapeGallery
    plain, both = runs["plain"], runs["both"]
    # without the switch: the line and the dict of the parent commit
    pm = plain["metrics"]
    line = (f'\nRR@1 RR@5 NDCG@5 MRR\n{round(pm["recall_rate"][0] * 100, 2)} {round(pm["recall_rate"][4] * 100, 2)} '
            f'{round(pm["ndcg"][4] * 100, 2)} {round(pm["mrr"] * 100, 2)}\n')
    assert plain["printed"] == line + f"\nPredictions saved at {plain['dir'] / 'output.p'}\n"
    assert sorted(pm) == ["indices", "mrr", "ndcg", "precision", "recall", "recall_rate"]
    assert not (plain["dir"] / "nearest_s2t.jsonl").exists()
    # with it: the same text -> shape numbers and files, and the S2T line between the two
    bm = both["metrics"]
    same_metrics(bm, pm)
    s2t = bm["s2t"]
    s2t_line = (f'\nS2T RR@1 RR@5 NDCG@5 MRR\n{round(s2t["recall_rate"][0] * 100, 2)} {round(s2t["recall_rate"][4] * 100, 2)} '
                f'{round(s2t["ndcg"][4] * 100, 2)} {round(s2t["mrr"] * 100, 2)}\n')
    assert both["printed"] == line + s2t_line + f"\nPredictions saved at {both['dir'] / 'output.p'}\n"
    assert (both["dir"] / "nearest.jsonl").read_bytes() == (plain["dir"] / "nearest.jsonl").read_bytes()
    assert (both["dir"] / "output.p").read_bytes() == (plain["dir"] / "output.p").read_bytes()
    # the S2T numbers against a CaptionGallery asked directly with the saved embeddings
    with open(both["dir"] / "output.p", "rb") as f:
        tuples = pickle.load(f)["caption_embedding_tuples"]
    ids, cats = [t[2] for t in tuples], [t[1] for t in tuples]
    text, shape = dev(np.stack([t[3] for t in tuples]).astype(np.float32), np.stack([t[4] for t in tuples]).astype(np.float32))
    shapes, labels = ShapeGallery.from_captions(ids, cats, shape)
    captions = CaptionGallery.from_captions(ids, cats, text)
    assert len(shapes) == 256 and len(captions) == 512 and captions.classes.tolist() == labels.tolist()
    idx, sim, hit = captions.rank(shapes.embeddings, torch.arange(len(shapes)), k=5)
    assert s2t["indices"].shape == (256, 5)
    np.testing.assert_array_equal(idx.cpu().numpy(), s2t["indices"])
    assert int(hit.min()) >= 0 and s2t["mrr"] == float(np.mean(1.0 / (hit.cpu().numpy() + 1)))
    with open(both["dir"] / "nearest_s2t.jsonl") as f:
        records = [json.loads(r) for r in f]
    assert len(records) == 256 and [r["groundtruth"] for r in records] == shapes.model_ids
    assert records[0]["retrieved_models"] == [ids[c] for c in records[0]["retrieved_captions"]]


def test_eval_command_scores_s2t_from_the_saved_predictions(runs, capsys):
    from tricolo_amd import eval as evaluate
    m = evaluate.main(["data=synthetic", f"+prediction_file_path={runs['plain']['dir'] / 'output.p'}", "+direction=both"])
    assert "\nS2T RR@1 RR@5 NDCG@5 MRR\n" in capsys.readouterr().out
    want = runs["both"]["metrics"]
    for name in NUMBERS + ("indices",):
        np.testing.assert_array_equal(m[name], want[name])
        np.testing.assert_array_equal(m["s2t"][name], want["s2t"][name])
    assert m["mrr"] == want["mrr"] and m["s2t"]["mrr"] == want["s2t"]["mrr"]


# ------------------------------------------------------------------------------------------------ 7. the validation log
def test_validation_log_carries_the_s2t_numbers_when_asked():
    """train.fit over one epoch without training batches and three validation batches of data=synthetic: with inference.direction=both
    (or s2t) the epoch's record and the net's log hold val_eval/S2T_RR@1, S2T_RR@5, S2T_NDCG@5 and S2T_MRR - the numbers of
    compute_metrics on the same embeddings - beside the text -> shape ones, which are those of a run without the switch (the monitor);
    without it no S2T key appears."""
    import itertools

    from tests.test_gpu_inference_cli import BIV
    from tricolo_amd import config as tcfg
    from tricolo_amd.evaluation.eval_retrieval import compute_metrics
    from tricolo_amd.model.tricolo_net import TriCoLoNet
    from tricolo_amd.train import fit, split_batches
    s2t_keys = ["val_eval/S2T_MRR", "val_eval/S2T_NDCG@5", "val_eval/S2T_RR@1", "val_eval/S2T_RR@5"]
    recs, logged = {}, {}
    for name, extra in (("plain", []), ("both", ["+inference.direction=both"]), ("s2t", ["+inference.direction=s2t"])):
        cfg = tcfg.compose(overrides=BIV + ["trainer.max_epochs=1", "trainer.check_val_every_n_epoch=1"] + extra)
        torch.manual_seed(5)
        net = TriCoLoNet(cfg)
        out = fit(net, cfg, lambda epoch: [], lambda epoch: itertools.islice(split_batches(cfg, "val")(epoch), 3), log=lambda rec: None)
        recs[name], logged[name] = out["history"][0], dict(net.logged)
    assert [k for k in recs["plain"] if "S2T" in k] == [] and [k for k in logged["plain"] if "S2T" in k] == []
    with torch.no_grad():
        net.eval()
        for i, batch in enumerate(itertools.islice(split_batches(cfg, "val")(0), 3)):
            net.test_step(batch, i)
    want = compute_metrics("Synthetic", net._collate_output(), direction="s2t")
    net.val_test_step_outputs.clear()
    for name in ("both", "s2t"):
        assert sorted(k for k in recs[name] if "S2T" in k) == s2t_keys and sorted(k for k in logged[name] if "S2T" in k) == s2t_keys
        assert recs[name]["val_eval/RR@5"] == recs["plain"]["val_eval/RR@5"] and recs[name]["val_eval/RR@1"] == recs["plain"]["val_eval/RR@1"]
        assert recs[name]["val_eval/S2T_RR@1"] == float(want["recall_rate"][0] * 100)
        assert recs[name]["val_eval/S2T_RR@5"] == float(want["recall_rate"][4] * 100)
        assert recs[name]["val_eval/S2T_NDCG@5"] == float(want["ndcg"][4] * 100) and recs[name]["val_eval/S2T_MRR"] == float(want["mrr"] * 100)
        assert logged[name]["val_eval/S2T_MRR"] == want["mrr"] * 100 and logged[name]["val_eval/MRR"] == logged["plain"]["val_eval/MRR"]
