"""GPU: csrc/chamfer.hip through tricolo_amd.evaluation.shape_f1 - every pair of tests/golden/shape_f1.npz under conditions 1-4
(tests/test_shape_f1.check_case), then the edges: sizes around the tile boundaries, padding with garbage, a shared cloud, identical
clouds, empty clouds, launch splitting, rejected inputs, run-to-run bit identity, and nearest.jsonl from compute_metrics."""
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import shape_f1_reference as sr
from tests.test_shape_f1 import CASES, REPO_ROOT, check_case, check_idx, make_point_cache

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def cloud(rng, *shape):
    return torch.from_numpy((3.0 * rng.standard_normal(shape + (3,))).astype(np.float32)).to(DEV)


def check_against_float64(d2, idx, p, q, what):
    want, _ = sr.nn_exact(p.cpu().numpy(), q.cpu().numpy())
    sr.check_d2(d2.cpu().numpy(), want, what)
    check_idx(idx.cpu().numpy(), want, p.cpu().numpy(), q.cpu().numpy(), what)


@pytest.mark.parametrize("tag", CASES)
def test_fixture_pairs(golden, tag):
    check_case(golden("shape_f1"), tag, DEV)


@pytest.mark.parametrize("S1,S2", [(1, 1), (63, 65), (64, 257), (65, 64), (257, 1), (10000, 63), (1, 65536), (2049, 2048), (4097, 2055),
                                   (65536, 65536)])
def test_sizes_around_the_tiles(S1, S2):
    from tricolo_amd.evaluation import shape_f1 as sf
    rng = np.random.default_rng(S1 * 7 + S2)
    p, q = cloud(rng, 1, S1), cloud(rng, 1, S2)
    d2, idx = sf.nn_dist2(p, q, return_idx=True)
    check_against_float64(d2[0], idx[0], p[0], q[0], f"{S1} x {S2}")
    assert torch.equal(sf.nn_dist2(p, q), d2)


def test_padding_garbage_does_not_leak():
    from tricolo_amd.evaluation import shape_f1 as sf
    rng = np.random.default_rng(17)
    p, q = cloud(rng, 4, 3000), cloud(rng, 4, 2600)
    lp, lq = [3000, 17, 2049, 0], [2600, 2048, 5, 1300]
    for n in range(4):
        p[n, lp[n]:] = float("nan") if n % 2 else 1e30
        q[n, lq[n]:] = 1e30 if n % 2 else float("nan")
    tlp, tlq = torch.tensor(lp, device=DEV), torch.tensor(lq, device=DEV)
    d2, idx = sf.nn_dist2(p, q, tlp, tlq, return_idx=True)
    thresholds = (0.5, 1.0, 2.0)
    m = sf.compute_sampling_metrics(p, q, thresholds=thresholds, lengths_pred=tlp, lengths_gt=tlq)
    for n in range(4):
        assert (d2[n, lp[n]:] == 0).all() and (idx[n, lp[n]:] == -1).all()
        if lp[n] == 0:
            assert all(torch.isnan(m[k][n]) for k in m if not k.startswith("Recall"))            # the mean of nothing
            continue
        pn, qn = p[n:n + 1, :lp[n]].contiguous(), q[n:n + 1, :lq[n]].contiguous()
        d2n, idxn = sf.nn_dist2(pn, qn, return_idx=True)
        assert torch.equal(d2[n, :lp[n]], d2n[0]) and torch.equal(idx[n, :lp[n]], idxn[0])      # the cut-out clouds, bit for bit
        check_against_float64(d2n[0], idxn[0], pn[0], qn[0], f"cloud {n}")
        mn = sf.compute_sampling_metrics(pn, qn, thresholds=thresholds)
        for k in m:
            assert torch.equal(m[k][n:n + 1], mn[k]), (n, k)


@pytest.mark.parametrize("N", [1, 3, 70])
def test_shared_cloud(N):
    """One ground truth for N predictions (the reference's gt_points.expand): the same bits as the expanded batch, on either side.
    N = 70 x 10,000 points runs the four-points-per-thread kernel, N = 1 and 3 the one-point one; they must agree."""
    from tricolo_amd.evaluation import shape_f1 as sf
    rng = np.random.default_rng(N)
    p, q = cloud(rng, N, 10000), cloud(rng, 1, 9000)
    qx = q.expand(N, -1, -1).contiguous()
    d2, idx = sf.nn_dist2(p, q, return_idx=True)
    d2x, idxx = sf.nn_dist2(p, qx, return_idx=True)
    assert d2.shape == (N, 10000) and torch.equal(d2, d2x) and torch.equal(idx, idxx)
    r2, ridx = sf.nn_dist2(q, p, return_idx=True)                                               # the shared cloud on the left
    r2x, ridxx = sf.nn_dist2(qx, p, return_idx=True)
    assert r2.shape == (N, 9000) and torch.equal(r2, r2x) and torch.equal(ridx, ridxx)
    for n in {0, N - 1}:
        one, ione = sf.nn_dist2(p[n:n + 1], q, return_idx=True)
        assert torch.equal(one[0], d2[n]) and torch.equal(ione[0], idx[n])
        check_against_float64(d2[n], idx[n], p[n], q[0], f"N={N} cloud {n}")
        check_against_float64(r2[n], ridx[n], q[0], p[n], f"N={N} cloud {n} reversed")
    m, mx = sf.compute_sampling_metrics(p, q, thresholds=(0.2, 0.4)), sf.compute_sampling_metrics(p, qx, thresholds=(0.2, 0.4))
    assert all(torch.equal(m[k], mx[k]) and m[k].shape == (N,) for k in m)
    again = sf.compute_sampling_metrics(p, q, thresholds=(0.2, 0.4))                             # two runs, the same bits
    assert all(torch.equal(m[k], again[k]) for k in m) and torch.equal(sf.nn_dist2(p, q), d2)


def test_identical_clouds():
    from tricolo_amd.evaluation import shape_f1 as sf
    rng = np.random.default_rng(2)
    p = cloud(rng, 2, 10000)
    d2, idx = sf.nn_dist2(p, p.clone(), return_idx=True)
    assert (d2 == 0).all() and torch.equal(idx, torch.arange(10000, device=DEV).expand(2, -1))
    m = sf.compute_sampling_metrics(p, p.clone(), thresholds=(0.1,))
    want = float(np.float32(2.0 * 100.0 * 100.0) / (np.float32(200.0) + np.float32(1e-8)))
    assert m["F1@0.100000"].tolist() == [want, want] and m["Precision@0.100000"].tolist() == [100.0, 100.0]
    assert m["Chamfer-L2"].tolist() == [0.0, 0.0]


def test_empty_clouds():
    from tricolo_amd.evaluation import shape_f1 as sf
    rng = np.random.default_rng(4)
    p, q = cloud(rng, 2, 100), cloud(rng, 2, 80)
    d2, idx = sf.nn_dist2(p, q, lengths_q=torch.tensor([80, 0], device=DEV), return_idx=True)
    assert torch.isinf(d2[1]).all() and (d2[1] > 0).all() and (idx[1] == -1).all() and torch.isfinite(d2[0]).all()
    d2, idx = sf.nn_dist2(p, q[:, :0], return_idx=True)                                         # S2 = 0
    assert d2.shape == (2, 100) and torch.isinf(d2).all() and (idx == -1).all()
    d2, idx = sf.nn_dist2(p[:, :0], q, return_idx=True)                                         # S1 = 0
    assert d2.shape == (2, 0) and idx.shape == (2, 0)
    m = sf.compute_sampling_metrics(p, q, thresholds=(1.0,), lengths_gt=torch.tensor([80, 0], device=DEV))
    assert float(m["Precision@1.000000"][1]) == 0.0 and torch.isnan(m["Recall@1.000000"][1]) and torch.isfinite(m["F1@1.000000"][0])


def test_batch_beyond_one_launch():
    """More clouds than one grid holds (2^23 workgroups per launch): the batch is split over launches."""
    from tricolo_amd.evaluation import shape_f1 as sf
    N = (1 << 23) + 5
    gen = torch.Generator(device=DEV).manual_seed(1)
    p = torch.randn((N, 1, 3), device=DEV, generator=gen)
    q = torch.randn((1, 3, 3), device=DEV, generator=gen)
    d2, idx = sf.nn_dist2(p, q, return_idx=True)
    diff = p.double() - q.double()                                                              # [N, 3, 3]
    want = (diff * diff).sum(-1).min(-1).values
    assert ((d2[:, 0].double() - want).abs() <= sr.D2_REL * want).all()
    assert ((idx >= 0) & (idx < 3)).all()
    assert (((diff * diff).sum(-1).gather(1, idx)[:, 0] - want).abs() <= sr.D2_REL * want).all()


def test_rejected_and_copied_inputs():
    from tricolo_amd import ops
    from tricolo_amd.evaluation import shape_f1 as sf
    rng = np.random.default_rng(6)
    p, q = cloud(rng, 2, 300), cloud(rng, 2, 200)
    wide = cloud(rng, 2, 300)[:, ::2]                                                           # not contiguous
    assert not wide.is_contiguous()
    assert torch.equal(sf.nn_dist2(wide, q), sf.nn_dist2(wide.contiguous(), q))                 # the interface copies ...
    with pytest.raises(ValueError, match="contiguous"):
        ops.nn_dist2(wide, q)                                                                   # ... the op refuses
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.nn_dist2(p.cpu(), q.cpu())
    with pytest.raises(ValueError, match="one device"):
        sf.nn_dist2(p, q.cpu())
    with pytest.raises(ValueError):
        sf.nn_dist2(p.double(), q.double())
    with pytest.raises(ValueError):
        sf.nn_dist2(p, q, lengths_p=torch.tensor([300], device=DEV))
    # the CPU fallback and the kernel: the same counts wherever float64 leaves no doubt (conditions 1-4 hold for both)
    c_gpu = sf.sampling_counts(p, q, (1.0, 2.0))
    c_cpu = sf.sampling_counts(p.cpu(), q.cpu(), (1.0, 2.0))
    for n in range(2):
        truth, _ = sr.nn_exact(p[n].cpu().numpy(), q[n].cpu().numpy())
        for k, t in enumerate((1.0, 2.0)):
            if sr.threshold_counts(truth, t).undecidable == 0:
                assert int(c_gpu[0][n, k]) == int(c_cpu[0][n, k])


def test_nearest_jsonl_from_compute_metrics(golden, tmp_path):
    """compute_metrics(nearest_path=...) writes the file, shape_f1_from_nearest and the command line read it."""
    from tricolo_amd.evaluation import eval_retrieval as er, shape_f1 as sf
    _, cache, _ = make_point_cache(tmp_path, golden("shape_f1"))
    ids = ["aaaa", "bbbb", "cccc", "dddd", "eeee", "ffff"]                                        # eeee, ffff: no cloud
    rng = np.random.default_rng(8)
    shape_emb = {m: np.eye(16, dtype=np.float32)[k] for k, m in enumerate(ids)}
    tuples = [(f"caption {i}", "03001627", m, shape_emb[ids[(j + i % 2) % 6]] + 0.01 * rng.standard_normal(16).astype(np.float32), shape_emb[m])
              for i in range(2) for j, m in enumerate(ids)]
    nearest = str(tmp_path / "nearest_cm.jsonl")
    er.compute_metrics("Text2Shape", {"caption_embedding_tuples": tuples}, nearest_path=nearest)
    r = sf.shape_f1_from_nearest(nearest, cache, threshold=0.5, batch=3)
    assert len(r["f1"]) == 7 and r["skipped"] == 5                  # even captions: own shape (4 with clouds); odd ones: the next (3)
    assert r["mean_f1"] == sum(r["f1"]) / len(r["f1"])
    assert r["f1"][:4] == [100.0] * 4 and max(r["f1"][4:]) < 100.0
    one = sf.shape_f1_from_nearest(nearest, cache, threshold=0.5, batch=1, device=torch.device("cpu"))
    assert [np.float32(v) for v in one["f1"]] == [np.float32(v) for v in r["f1"]]                # counts are pinned on these pairs
    out = subprocess.run([sys.executable, "-m", "tricolo_amd.evaluation.shape_f1", nearest, "--point-cache", cache, "--threshold", "0.5"],
                         cwd=REPO_ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    assert lines[0].startswith(f"skipped {r['skipped']} of 12 records") and float(lines[-1]) == pytest.approx(r["mean_f1"], rel=1e-6)
