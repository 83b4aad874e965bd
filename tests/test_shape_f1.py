"""CPU: tricolo_amd.evaluation.shape_f1 (torch fallback) against tests/golden/shape_f1.npz (written by tools/make_shape_f1_golden.py from
the REAL calculate_f1._compute_sampling_metrics) and the float64 restatement tests/shape_f1_reference.py; nearest.jsonl reading.

check_case states conditions 1-4 once; tests/test_gpu_shape_f1.py runs it on the device for every fixture pair."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from tests import shape_f1_reference as sr

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO_ROOT, "tests", "golden", "shape_f1.npz")
CASES = [str(t) for t in np.load(GOLDEN, allow_pickle=False)["cases"]]
SMALL = [t for t in CASES if t.startswith("small_")]


def case_clouds(g, tag):
    """The pair's fp32 clouds from its recipe, checked against the recorded SHA-256."""
    pred, gt = sr.make_pair(str(g[f"{tag}/kind"]), int(g[f"{tag}/S_pred"]), int(g[f"{tag}/S_gt"]), int(g[f"{tag}/seed"]))
    assert hashlib.sha256(pred.tobytes() + gt.tobytes()).hexdigest() == str(g[f"{tag}/sha256"]), \
        f"{tag}: the recipe no longer yields the clouds the fixture was computed from"
    return pred, gt


def check_idx(idx, d2_64, p, q, what):
    """Condition 2: in range, and the float64 distance to the chosen point meets the d2 bound against the true minimum."""
    idx = np.asarray(idx)
    assert idx.dtype == np.int64 and (idx >= 0).all() and (idx < q.shape[0]).all(), what
    chosen = sr.dist2_to(p, q, idx)
    assert (np.abs(chosen - d2_64) <= sr.D2_REL * d2_64).all(), what


def check_case(g, tag, device):
    """Conditions 1-4 for one fixture pair on `device`."""
    from tricolo_amd.evaluation import shape_f1 as sf
    thresholds = tuple(float(t) for t in g["thresholds"])
    pred, gt = case_clouds(g, tag)
    S1, S2 = pred.shape[0], gt.shape[0]
    tp, tg = torch.from_numpy(pred)[None].to(device), torch.from_numpy(gt)[None].to(device)
    d2p_64, _ = sr.nn_exact(pred, gt)
    d2g_64, _ = sr.nn_exact(gt, pred)
    # the restatement sees what the generator saw
    np.testing.assert_allclose(d2p_64[g[f"{tag}/rows_pred"]], g[f"{tag}/d2_pred"], rtol=1e-13, atol=0)
    np.testing.assert_allclose(d2g_64[g[f"{tag}/rows_gt"]], g[f"{tag}/d2_gt"], rtol=1e-13, atol=0)
    # 1, 2
    d2p, idxp = sf.nn_dist2(tp, tg, return_idx=True)
    d2g, idxg = sf.nn_dist2(tg, tp, return_idx=True)
    assert d2p.shape == (1, S1) and d2p.dtype == torch.float32 and idxg.shape == (1, S2) and idxg.dtype == torch.int64
    sr.check_d2(d2p[0].cpu().numpy(), d2p_64, f"{tag} pred->gt")
    sr.check_d2(d2g[0].cpu().numpy(), d2g_64, f"{tag} gt->pred")
    check_idx(idxp[0].cpu().numpy(), d2p_64, pred, gt, f"{tag} pred->gt idx")
    check_idx(idxg[0].cpu().numpy(), d2g_64, gt, pred, f"{tag} gt->pred idx")
    assert torch.equal(sf.nn_dist2(tp, tg), d2p)                          # without idx: the same distances
    # 3
    cp, sp, cg, sg = sf.sampling_counts(tp, tg, thresholds)
    assert cp.shape == (1, len(thresholds)) and cp.dtype == torch.int32
    fp = sr.check_counts(cp[0].cpu().numpy(), d2p_64, thresholds, f"{tag} pred->gt")
    fg = sr.check_counts(cg[0].cpu().numpy(), d2g_64, thresholds, f"{tag} gt->pred")
    assert [c.below for c in fp] == g[f"{tag}/below_pred"].tolist() and [c.undecidable for c in fp] == g[f"{tag}/undecidable_pred"].tolist()
    assert [c.below for c in fg] == g[f"{tag}/below_gt"].tolist() and [c.undecidable for c in fg] == g[f"{tag}/undecidable_gt"].tolist()
    assert all(a.undecidable + b.undecidable <= sr.MAX_UNDECIDABLE for a, b in zip(fp, fg))
    # 4
    m = sf.compute_sampling_metrics(tp, tg, thresholds=thresholds)
    precision, recall, f1 = sf.f1_from_counts(cp.cpu(), cg.cpu(), S1, S2)
    for k, t in enumerate(thresholds):
        got = {n: m[f"{n}@%f" % t].cpu() for n in ("F1", "Precision", "Recall")}
        assert all(v.shape == (1,) and v.dtype == torch.float32 for v in got.values())
        print(f"{tag} t={t}: F1 {float(got['F1']):.9g} precision {float(got['Precision']):.9g} recall {float(got['Recall']):.9g}  "
              f"reference F1 {float(g[f'{tag}/ref_f1'][k]):.9g}")
        assert got["Precision"].numpy().tobytes() == precision[k].numpy().tobytes()
        assert got["Recall"].numpy().tobytes() == recall[k].numpy().tobytes()
        assert got["F1"].numpy().tobytes() == f1[k].numpy().tobytes()
        if fp[k].undecidable == 0 and fg[k].undecidable == 0:
            assert got["F1"].numpy().tobytes() == g[f"{tag}/ref_f1"][k:k + 1].tobytes(), (tag, t)
    assert torch.equal(sf.f1_score(tp, tg, thresholds[-1]).cpu(), m["F1@%f" % thresholds[-1]].cpu())
    c64 = float(g[f"{tag}/chamfer64"])
    assert c64 == pytest.approx(d2p_64.mean() + d2g_64.mean(), rel=1e-12)
    chamfer = float(m["Chamfer-L2"][0])
    print(f"{tag}: Chamfer-L2 {chamfer:.9g} float64 {c64:.9g}")
    assert abs(chamfer - c64) <= (sr.D2_REL + max(S1, S2) * 2.0 ** -24) * c64


@pytest.mark.parametrize("tag", SMALL)
def test_cpu_fallback_meets_the_fixture(golden, tag):
    check_case(golden("shape_f1"), tag, torch.device("cpu"))


def test_fixture_populates_both_sides_of_the_thresholds(golden):
    g = golden("shape_f1")
    f1 = np.concatenate([g[f"{t}/ref_f1"] for t in CASES])
    assert f1.min() < 2.0 and f1.max() == 100.0 and ((f1 > 5.0) & (f1 < 99.0)).sum() >= 4
    assert os.path.getsize(GOLDEN) < 1 << 20


def test_reference_expression_restatements_agree():
    """numpy fp32 (the fixture generator's check against the reference) and torch fp32 (the tests' check of the kernel)."""
    from tricolo_amd.evaluation import shape_f1 as sf
    rng = np.random.default_rng(5)
    cp, cq = rng.integers(0, 10001, size=(200, 1)), rng.integers(0, 9001, size=(200, 1))
    cp[:3], cq[:3] = [[0], [0], [10000]], [[0], [7], [9000]]
    p, r, f = sf.f1_from_counts(torch.from_numpy(cp), torch.from_numpy(cq), 10000, 9000)
    for i in range(200):
        want = sr.f1_fp32(int(cp[i, 0]), 10000, int(cq[i, 0]), 9000)
        assert (float(p[0, i]), float(r[0, i]), float(f[0, i])) == tuple(float(w) for w in want)
    assert float(f[0, 0]) == 0.0 and float(f[0, 2]) == float(np.float32(2.0 * 100.0 * 100.0) / (np.float32(200.0) + np.float32(1e-8)))


def test_lengths_padding_shared_and_empty_on_cpu():
    from tricolo_amd.evaluation import shape_f1 as sf
    rng = np.random.default_rng(9)
    p = torch.from_numpy(rng.standard_normal((3, 50, 3)).astype(np.float32))
    q = torch.from_numpy(rng.standard_normal((3, 40, 3)).astype(np.float32))
    lp, lq = torch.tensor([50, 17, 5]), torch.tensor([40, 0, 33])
    p[1, 17:], p[2, 5:], q[2, 33:] = float("nan"), 1e30, float("nan")
    d2, idx = sf.nn_dist2(p, q, lp, lq, return_idx=True)
    for n in range(3):
        a, b = p[n, :lp[n]].numpy(), q[n, :lq[n]].numpy()
        assert (d2[n, lp[n]:] == 0).all() and (idx[n, lp[n]:] == -1).all()
        if lq[n] == 0:
            assert torch.isinf(d2[n, :lp[n]]).all() and (idx[n, :lp[n]] == -1).all()
            continue
        want, _ = sr.nn_exact(a, b)
        sr.check_d2(d2[n, :lp[n]].numpy(), want, f"cloud {n}")
        check_idx(idx[n, :lp[n]].numpy(), want, a, b, f"cloud {n}")
    # one ground truth for the whole batch = the expanded ground truth
    shared = sf.compute_sampling_metrics(p[:, :5].contiguous(), q[:1], thresholds=(0.5, 1.0))
    full = sf.compute_sampling_metrics(p[:, :5].contiguous(), q[:1].expand(3, -1, -1).contiguous(), thresholds=(0.5, 1.0))
    assert shared.keys() == full.keys() and list(shared) == ["F1@0.500000", "Precision@0.500000", "Recall@0.500000", "F1@1.000000",
                                                             "Precision@1.000000", "Recall@1.000000", "Chamfer-L2"]
    assert all(torch.equal(shared[k], full[k]) and shared[k].shape == (3,) for k in shared)
    with pytest.raises(ValueError):
        sf.nn_dist2(p.double(), q)
    with pytest.raises(ValueError):
        sf.nn_dist2(p[:2], q)
    with pytest.raises(ValueError):
        sf.compute_sampling_metrics(p, q, thresholds=[0.1] * 9)


def test_scale_to_gt():
    from tricolo_amd.evaluation import shape_f1 as sf
    rng = np.random.default_rng(3)
    pred = torch.from_numpy(rng.standard_normal((2, 30, 3)).astype(np.float32))
    gt = torch.from_numpy((rng.random((2, 20, 3)) * [1.0, 4.0, 2.0]).astype(np.float32))
    sp, sg = sf.scale_to_gt(pred, gt)
    edge = (sg.amax(1) - sg.amin(1)).amax(1)
    assert torch.allclose(edge, torch.full((2,), 10.0), rtol=1e-6)
    assert torch.allclose(sp / pred, (sg / gt)[:, :1, :1].expand_as(pred), rtol=1e-6)


def write_nearest(path, records):
    """Lines as compute_metrics(nearest_path=...) writes them (tricolo_amd/evaluation/eval_retrieval.py)."""
    with open(path, "w") as f:
        for i, (gt_id, retrieved) in enumerate(records):
            f.write(json.dumps({"cat_id": "03001627", "groundtruth": f"{gt_id}-{i:04d}", "retrieved_models": retrieved,
                                "distance": [0.9, 0.8, 0.7, 0.6, 0.5][:len(retrieved)]}) + "\n")


def make_point_cache(tmp_path, g):
    """A point-cache directory from the small fixture pairs; clouds in both of the reference's layouts."""
    cache = tmp_path / "point_cache"
    cache.mkdir()
    a_pred, a_gt = case_clouds(g, "small_unrelated")
    b_pred, b_gt = case_clouds(g, "small_near")
    np.save(cache / "aaaa.npy", a_gt[None])                 # [1, S, 3]
    np.save(cache / "bbbb.npy", a_pred)                     # [S, 3]
    np.save(cache / "cccc.npy", b_gt[None])
    np.save(cache / "dddd.npy", b_pred[None])
    records = [("aaaa", ["bbbb", "aaaa", "cccc", "dddd", "eeee"]), ("cccc", ["dddd", "cccc", "aaaa", "bbbb", "eeee"]),
               ("aaaa", ["aaaa", "bbbb", "cccc", "dddd", "eeee"]), ("eeee", ["aaaa", "bbbb", "cccc", "dddd", "eeee"]),
               ("cccc", ["zzzz", "cccc", "aaaa", "bbbb", "dddd"])]
    write_nearest(tmp_path / "nearest.jsonl", records)
    k = list(g["thresholds"]).index(0.5)
    want = [float(g["small_unrelated/ref_f1"][k]), float(g["small_near/ref_f1"][k]), 100.0]
    return str(tmp_path / "nearest.jsonl"), str(cache), want


def test_shape_f1_from_nearest(golden, tmp_path, capsys):
    from tricolo_amd.evaluation import shape_f1 as sf
    nearest, cache, want = make_point_cache(tmp_path, golden("shape_f1"))
    for batch in (64, 2, 1):                                 # mixed sizes in one batch (padding + lengths) and one pair at a time
        r = sf.shape_f1_from_nearest(nearest, cache, threshold=0.5, batch=batch, device=torch.device("cpu"))
        assert r["skipped"] == 2 and r["records"] == [0, 1, 2]
        assert [np.float32(v) for v in r["f1"]] == [np.float32(v) for v in want]
        assert r["mean_f1"] == sum(r["f1"]) / 3
    if not torch.cuda.is_available():                        # the command line picks the device itself
        sf.main([nearest, "--point-cache", cache, "--threshold", "0.5"])
        out = capsys.readouterr().out.strip().splitlines()
        assert "skipped 2 of 5 records" in out[0] and float(out[-1]) == r["mean_f1"]
