"""GPU: tri_retrieval_gallery (csrc/gallery.hip) through ops.retrieval_gallery - the ranking of tri_retrieval_topk for galleries of any
size.  References and inputs: tests/head_reference.py (integer-valued inputs make every similarity exact, so indices, similarities and
first_hit must be EQUAL to the float64 numpy ranking); on real-valued inputs the kernel must return the very bits of
ops.retrieval_topk.  The guarded case follows test_retrieval_topk of tests/test_gpu_guard_bands.py."""
import numpy as np
import pytest
import torch

from tests import head_reference as hr
from tests.guard_bands import POISON, ZERO, guarded_ops, same_bytes

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tricolo_amd import ops

DEV = "cuda"

# the kernel's own tiles: QT = 8 / 4 / 2 / 1 queries per workgroup for D <= 512 / 1024 / 2048 / 4096; a wave holds 2 shape rows at a
# time, the four waves of a workgroup advance 8 rows per trip
TILE_EDGES = [(7, 15, 64, 5), (9, 17, 64, 5),          # QT = 8: one query short of a tile / one into the second; Ns one short of two trips
                                                       # (wave 3's second row missing) / one into the third (wave 0's second row missing)
              (3, 9, 520, 3), (5, 7, 1024, 3),         # QT = 4 on either side of its tile, D at both ends of its range
              (1, 10, 1030, 2), (3, 6, 2048, 2),       # QT = 2
              (2, 9, 2049, 2)]                         # QT = 1: every query a workgroup of its own
PAST_THE_OLD_LIMIT = [(3, 19137, 64, 5), (5, 40003, 36, 8)]
CASES = hr.RETRIEVAL_INT + [(1, 7, 68, 7), (17, 65, 4, 64), (5, 64, 130, 64)] + PAST_THE_OLD_LIMIT + [(2, 300, 2048, 5)] + TILE_EDGES


def dev(*arrays):
    return [torch.from_numpy(a).to(DEV) for a in arrays]


@pytest.mark.parametrize("case", CASES, ids=str)
def test_gallery_ranking_integer_exact(case):
    """retrieval_gallery_kernel on integer similarities (below 2^24: exact in any order, a third of the shape rows are copies, so ties
    are exact too): idx, sim and first_hit EQUAL retrieval_reference.  The four RETRIEVAL_INT shapes of the old kernel; (1, 7, 68, 7)
    k == Ns with one query; (17, 65, 4, 64) and (5, 64, 130, 64) k at TRI_GALLERY_MAX_K with Ns = k + 1 and Ns = k, D < 64 and
    D % 64 != 0 (a full-width list merge: all 256 threads hold an entry); (3, 19137, 64, 5) and (5, 40003, 36, 8) are past
    tri_retrieval_topk's Ns + D = 19200; (2, 300, 2048, 5) the widest rows the issue names (QT = 2).  TILE_EDGES: (7, 15, 64, 5) /
    (9, 17, 64, 5) sit one below / one above the 8-query tile and the 8-rows-per-trip shape step (15: the last wave's second row is
    missing; 17: a third trip with one row); (3, 9, 520, 3) / (5, 7, 1024, 3) the 4-query tile at both ends of its D range;
    (1, 10, 1030, 2) / (3, 6, 2048, 2) the 2-query tile; (2, 9, 2049, 2) the 1-query tile."""
    Nq, Ns, D, k = case
    txt, shp, lab = hr.retrieval_int_inputs(Nq, Ns, D)
    top, top_sims, first_hit, _ = hr.retrieval_reference(txt, shp, lab, k)
    idx, sim, hit = ops.retrieval_gallery(*dev(txt, shp, lab), k=k)
    assert idx.dtype == torch.int32 and sim.dtype == torch.float64 and hit.dtype == torch.int32
    np.testing.assert_array_equal(idx.cpu().numpy(), top)
    np.testing.assert_array_equal(sim.cpu().numpy(), top_sims)
    np.testing.assert_array_equal(hit.cpu().numpy(), first_hit)


@pytest.mark.parametrize("case", [(16, 300, 512, 5), (33, 1486, 512, 5)], ids=str)
def test_gallery_returns_the_bits_of_retrieval_topk(case):
    """Real-valued inputs at the evaluation's width, the second at the val split's gallery size with a ragged last query tile: idx, the
    raw bytes of sim and first_hit are those of ops.retrieval_topk; without labels the same idx / sim and no first_hit; a second run
    repeats the first bit for bit."""
    Nq, Ns, D, k = case
    txt, shp, lab = dev(*hr.retrieval_float_inputs(Nq, Ns, D))
    idx0, sim0, hit0 = ops.retrieval_topk(txt, shp, lab, k=k)
    idx, sim, hit = ops.retrieval_gallery(txt, shp, lab, k=k)
    print(f"GALLERY {case} idx_mismatch={int((idx != idx0).sum())} sim_mismatch={int((sim.view(torch.int64) != sim0.view(torch.int64)).sum())} "
          f"hit_mismatch={int((hit != hit0).sum())}")
    assert torch.equal(idx, idx0) and same_bytes(sim, sim0) and torch.equal(hit, hit0)
    idx1, sim1, hit1 = ops.retrieval_gallery(txt, shp, None, k=k)
    assert hit1 is None and torch.equal(idx1, idx) and same_bytes(sim1, sim)
    idx2, sim2, hit2 = ops.retrieval_gallery(txt, shp, lab, k=k)
    assert torch.equal(idx2, idx) and same_bytes(sim2, sim) and torch.equal(hit2, hit)


def test_gallery_rejections():
    """tri_retrieval_gallery's argument checks: 1 <= k <= min(Ns, 64), D <= 4096, first_hit only with label; no queries is no work."""
    txt, shp, lab = dev(*hr.retrieval_int_inputs(4, 70, 68))
    for k in (0, 71):
        with pytest.raises(RuntimeError, match="1 <= k <= number of shapes"):
            ops.retrieval_gallery(txt, shp, lab, k=k)
    with pytest.raises(RuntimeError, match="TRI_GALLERY_MAX_K"):
        ops.retrieval_gallery(txt, shp, lab, k=65)
    with pytest.raises(RuntimeError, match="D > 4096"):
        ops.retrieval_gallery(torch.zeros(2, 4097, device=DEV), torch.zeros(9, 4097, device=DEV), None, k=5)
    idx, sim, hit = torch.empty(4, 5, dtype=torch.int32, device=DEV), torch.empty(4, 5, dtype=torch.float64, device=DEV), torch.empty(4, dtype=torch.int32, device=DEV)
    rc = ops.lib().tri_retrieval_gallery(ops.ptr(txt), ops.ptr(shp), None, 4, 70, 68, 5, ops.ptr(idx), ops.ptr(sim), ops.ptr(hit), ops.stream())
    assert rc == -1 and b"first_hit needs label" in ops.lib().tri_last_error()
    idx, sim, hit = ops.retrieval_gallery(txt[:0], shp, lab[:0], k=5)
    assert idx.shape == (0, 5) and sim.shape == (0, 5) and hit.shape == (0,)


def test_gallery_inside_guard_bands():
    """test_retrieval_topk of tests/test_gpu_guard_bands.py on the new entry point: Nq = 3, Ns = 37, D = 64, k = 5 with an exact tie,
    every operand and output between poisoned bands, under 0xFF and 0x00 fills with identical bytes."""
    rng = np.random.default_rng(3)
    shp = rng.standard_normal((37, 64)).astype(np.float32)
    shp[20] = shp[7]                                                 # an exact tie
    txt = shp[[7, 36, 0]] + 0.01 * rng.standard_normal((3, 64)).astype(np.float32)
    lab = np.array([7, 36, 5], dtype=np.int32)
    runs = []
    for fill in (POISON, ZERO):
        with guarded_ops(fill) as g:
            idx, sim, hit = ops.retrieval_gallery(g.put(torch.from_numpy(txt)), g.put(torch.from_numpy(shp)), g.put(torch.from_numpy(lab)), k=5)
            out = dict(idx=idx.cpu(), sim=sim.cpu(), hit=hit.cpu())
        assert g.launched == ["tri_retrieval_gallery"]
        runs.append(out)
    for name in runs[0]:
        assert same_bytes(runs[0][name], runs[1][name]), f"{name} depends on memory outside the operands"
    got = runs[0]
    top, top_sims, first_hit, _ = hr.retrieval_reference(txt, shp, lab, 5)
    np.testing.assert_array_equal(got["idx"].numpy(), top)
    np.testing.assert_array_equal(got["hit"].numpy(), first_hit)
    np.testing.assert_allclose(got["sim"].numpy(), top_sims, rtol=1e-13, atol=1e-13)
    assert 20 in top[0, :2] and 7 in top[0, :2] and list(top[0, :2]) == [20, 7]       # the tie: higher index first


def test_compute_metrics_past_the_old_limit():
    """compute_metrics over 19,200 distinct integer-valued shape rows of width 64 (Ns + D = 19264: tri_retrieval_topk refuses, the parent
    commit raised) returns, and matches retrieval_reference.  A shape enters compute_metrics with a caption tuple, so there are 19,200
    tuples: 40 of them (spread over the file, first and last included) carry a real caption - a shape row plus noise -, the others a zero
    text embedding, whose ranking is known in closed form (every similarity 0: higher index first, first_hit = Ns - 1 - label), which is
    what retrieval_reference gives for them without a 19,200 x 19,200 sort."""
    from tricolo_amd.evaluation.eval_retrieval import compute_metrics, compute_pr_at_k, nearest_neighbors_hip
    Ns, D, k = 19200, 64, 5
    rng = np.random.default_rng(11)
    shp = rng.integers(-2, 3, (Ns, D)).astype(np.float32)
    assert len(np.unique(shp, axis=0)) == Ns
    real = np.unique(np.concatenate([[0, Ns - 1], rng.integers(0, Ns, 38)]))
    while len(real) < 40:
        real = np.unique(np.concatenate([real, rng.integers(0, Ns, 40 - len(real))]))
    txt = np.zeros((Ns, D), dtype=np.float32)
    txt[real] = shp[real] + rng.integers(-1, 2, (40, D))
    lab = np.arange(Ns)
    top, top_sims, first_hit, _ = hr.retrieval_reference(txt[real], shp, lab[real], k)
    # what compute_metrics calls, on the 40 captions alone
    dist, idx, hit = nearest_neighbors_hip(shp, txt[real], lab[real], k)
    np.testing.assert_array_equal(idx, top)
    np.testing.assert_array_equal(dist, top_sims)
    np.testing.assert_array_equal(hit, first_hit)
    # the whole call
    tuples = [(None, "cat", f"m{i:05d}", txt[i], shp[i]) for i in range(Ns)]
    r = compute_metrics("Text2Shape", {"caption_embedding_tuples": tuples})
    want_idx = np.tile(np.arange(Ns - 1, Ns - 1 - k, -1), (Ns, 1))
    want_hit = Ns - 1 - lab
    want_idx[real], want_hit[real] = top, first_hit
    np.testing.assert_array_equal(r["indices"], want_idx)
    want = compute_pr_at_k(want_idx, want_hit, lab, k, Ns, np.arange(Ns))
    for name in ("precision", "recall", "recall_rate", "ndcg"):
        np.testing.assert_array_equal(r[name], want[name])
    assert r["mrr"] == want["mrr"]
