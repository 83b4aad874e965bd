"""CPU: tests/head_reference.py against torch autograd in float64, and the conditions that make the GPU assertions of
tests/test_gpu_head_paths.py mean something - each NT-Xent tolerance sees the defect its shape is there for by a factor of ten, every
integer retrieval case really has ties inside its top k + 1, and the integer cases are exact in fp32."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import head_reference as hr

NTX_SHAPES = hr.NTX_TILED + hr.NTX_WIDE + [hr.NTX_ZERO_ROW]


def ntx_case(B, D, norm=True):
    za, zb = hr.ntx_inputs(B, D)
    if (B, D) == hr.NTX_ZERO_ROW:
        za[hr.NTX_ZERO_ROW_INDEX] = 0
    if not norm:
        za, zb = hr.normalise_rows_f64_to_f32(za), hr.normalise_rows_f64_to_f32(zb)
    return za, zb


def nonzero_rows(B, D):
    keep = np.ones(B, bool)
    if (B, D) == hr.NTX_ZERO_ROW:
        keep[hr.NTX_ZERO_ROW_INDEX] = False
    return keep


@pytest.mark.parametrize("B,D", NTX_SHAPES)
def test_nt_xent_restatement_is_the_oracle_and_autograd(B, D):
    from oracle.modules import nt_xent_numpy
    za, zb = ntx_case(B, D)
    keep = nonzero_rows(B, D)
    loss, da, db = hr.nt_xent_f64(za.numpy(), zb.numpy())
    l_or, da_or, db_or = nt_xent_numpy(za.numpy(), zb.numpy(), hr.T, hr.ALPHA)
    assert abs(loss - l_or) < 1e-14
    np.testing.assert_allclose(da, da_or, rtol=1e-13, atol=1e-16)
    np.testing.assert_allclose(db, db_or, rtol=1e-13, atol=1e-16)
    l_ag, da_ag, db_ag = hr.nt_xent_torch(za, zb, dtype=torch.float64)
    assert abs(loss - l_ag) < 1e-12
    np.testing.assert_allclose(da[keep], da_ag[keep], rtol=1e-9, atol=1e-13)
    np.testing.assert_allclose(db, db_ag, rtol=1e-9, atol=1e-13)
    if not keep.all():
        # the all-zero row: a_hat = 0, so the gradient is da_hat / eps - O(1 / eps), finite, and what F.normalize's clamp gives
        row = hr.NTX_ZERO_ROW_INDEX
        assert np.isfinite(loss) and np.isfinite(da[row]).all() and np.abs(da[row]).min() > 1e9
        np.testing.assert_allclose(da[row], da_ag[row], rtol=1e-9)


def test_nt_xent_restatement_without_the_normalise_step():
    B, D = hr.NTX_TILED[0]
    za, zb = ntx_case(B, D, norm=False)
    assert abs(float(za.double().norm(dim=1).max()) - 1) < 1e-7                   # unit rows: the logits keep the normalised scale
    loss, da, db = hr.nt_xent_f64(za.numpy(), zb.numpy(), norm=False)
    l_ag, da_ag, db_ag = hr.nt_xent_torch(za, zb, norm=False, dtype=torch.float64)
    assert abs(loss - l_ag) < 1e-12
    np.testing.assert_allclose(da, da_ag, rtol=1e-9, atol=1e-13)
    np.testing.assert_allclose(db, db_ag, rtol=1e-9, atol=1e-13)
    l_n, _, _ = hr.nt_xent_f64(*[z.numpy() for z in ntx_case(B, D)])
    assert abs(loss - l_n) < 1e-6                                                 # same loss as the normalised case, up to the fp32 rounding of the rows


@pytest.mark.parametrize("B,D,norm", [(B, D, True) for B, D in NTX_SHAPES] + [hr.NTX_TILED[0] + (False,)])
def test_nt_xent_tolerances_see_each_shapes_defect(B, D, norm):
    """A float64 reference with the defect planted moves the loss or one gradient element (outside the all-zero row, which is compared
    relatively) by at least 10 x the tolerance asserted on the GPU; and the fp32 restatement itself is 10 x inside the tolerances, so
    they ask nothing of the kernel that fp32 arithmetic cannot give."""
    za, zb = ntx_case(B, D, norm)
    keep = nonzero_rows(B, D)
    loss, da, db = hr.nt_xent_f64(za.numpy(), zb.numpy(), norm=norm)
    defects = hr.ntx_defects(B, D)
    assert defects, "a shape that catches nothing"
    assert ("drop_last_col" in defects) == (D % 16 != 0) and ("lse_skip_last" in defects) == (B % 64 != 0) and ("zero_wide" in defects) == (D > 1024)
    for name in defects:
        l_d, da_d, db_d = hr.nt_xent_f64(za.numpy(), zb.numpy(), norm=norm, defect=name)
        moved_loss = abs(l_d - loss)
        moved_grad = max(np.abs(da_d - da)[keep].max(), np.abs(db_d - db).max())
        assert moved_loss >= 10 * hr.NTX_LOSS_TOL or moved_grad >= 10 * hr.NTX_GRAD_ATOL, (name, moved_loss, moved_grad)
    l32, da32, db32 = hr.nt_xent_torch(za, zb, norm=norm)
    assert abs(l32 - loss) <= hr.NTX_LOSS_TOL / 10
    assert max(np.abs(da32 - da)[keep].max(), np.abs(db32 - db).max()) <= hr.NTX_GRAD_ATOL / 10
    if not keep.all():
        row = hr.NTX_ZERO_ROW_INDEX
        assert (np.abs(da32[row] - da[row]) <= 1e-5 * np.abs(da[row])).all()


def test_nt_xent_multi_reference_is_the_sum_over_pairs():
    """The all-pairs gradient at dtotal = 1 is the plain sum of the pair gradients: autograd through the summed float64 losses."""
    from itertools import combinations
    B, D = 9, 20
    zs = hr.ntx_inputs(B, D, M=3)
    acc = [np.zeros((B, D)) for _ in range(3)]
    for a, b in combinations(range(3), 2):
        _, da, db = hr.nt_xent_f64(zs[a].numpy(), zs[b].numpy())
        acc[a] += da
        acc[b] += db
    zr = [z.double().requires_grad_() for z in zs]
    total = 0
    for a, b in combinations(range(3), 2):
        S = F.normalize(zr[a], dim=1) @ F.normalize(zr[b], dim=1).t() / hr.T
        lab = torch.arange(B)
        total = total + hr.ALPHA * F.cross_entropy(S, lab) + (1 - hr.ALPHA) * F.cross_entropy(S.t(), lab)
    total.backward()
    for m in range(3):
        np.testing.assert_allclose(acc[m], zr[m].grad.numpy(), rtol=1e-9, atol=1e-13)


# ------------------------------------------------------------------------------------------------ retrieval
@pytest.mark.parametrize("case", hr.RETRIEVAL_INT + [hr.RETRIEVAL_LIMIT], ids=str)
def test_retrieval_integer_cases_are_exact_and_tied(case):
    Nq, Ns, D, k = case
    txt, shp, lab = hr.retrieval_int_inputs(Nq, Ns, D)
    assert txt.shape == (Nq, D) and shp.shape == (Ns, D) and lab.shape == (Nq,)
    assert np.abs(shp).max() <= 2 and np.abs(txt).max() <= 3 and 6 * D < 2 ** 24          # |sim| <= 6 D: an exact integer in fp32 and fp64
    top, top_sims, hit, sims = hr.retrieval_reference(txt, shp, lab, k)
    assert np.array_equal((txt @ shp.T).astype(np.float64), sims) and np.array_equal(sims, np.rint(sims))
    assert hr.tie_share(sims, k) >= 0.5
    # the labels reach both ends of the index range and (with four or more queries) both copies of a repeated row
    assert lab[0] == 0 and lab[1] == Ns - 1
    if Nq >= 4:
        assert lab[2] != lab[3] and np.array_equal(shp[lab[2]], shp[lab[3]])
    # the reference is the ranking rule stated outright: larger similarity first, equal similarities with the higher index first
    for q in range(min(Nq, 4)):
        ranked = sorted(range(Ns), key=lambda s: (-sims[q, s], -s))
        assert ranked[:k] == list(top[q]) and ranked.index(lab[q]) == hit[q]
    assert Ns + D <= hr.RETRIEVAL_LDS_LIMIT


def test_retrieval_float_case_is_well_separated():
    Nq, Ns, D, k = hr.RETRIEVAL_FLOAT
    txt, shp, lab = hr.retrieval_float_inputs(Nq, Ns, D)
    _, _, _, sims = hr.retrieval_reference(txt, shp, lab, k)
    gaps = np.diff(np.sort(sims, axis=1), axis=1)
    assert gaps.min() > 1e-6 and np.abs(sims).max() < 1e3           # 1e-13 relative on a similarity cannot reorder anything


# ------------------------------------------------------------------------------------------------ embedding
@pytest.mark.parametrize("case", hr.EMBEDDING_CASES, ids=str)
def test_embedding_cases_hold_what_they_are_there_for(case):
    B, L, V, D = case
    tok, w, dout = hr.embedding_inputs(B, L, V, D)
    counts = torch.bincount(tok.flatten().long(), minlength=V)
    assert counts[0] > B * L // 4 and counts[V - 1] == 0 and (counts[1: V - 1] > 0).all()
    assert 3 * int(counts.max()) < 2 ** 24                          # integer gradients: every partial sum is exact in fp32
    out, dw = hr.embedding_reference(tok, w, dout)
    assert out.shape == (L, B, D) and torch.equal(out[5, 3], w[tok[3, 5].long()])
    assert torch.count_nonzero(dw[0]) == 0 and torch.count_nonzero(dw[V - 1]) == 0
    v = int(tok[0, 0]) or int(tok[tok > 0][0])
    assert torch.equal(dw[v], dout[(tok.t() == v)].sum(0))
    tokens = B * L
    assert {(24, 96, 50, 256): 2048 < tokens <= 4096 and tokens % 2048,        # second, ragged trip of the 2048-token scan
            (172, 96, 16, 8): tokens > 16384,                                  # more than 256 mask words
            (7, 96, 50, 300): 256 < D < 512}[case]                             # second, ragged trip of the column loop


# ------------------------------------------------------------------------------------------------ linear_small
def test_linear_integer_cases_are_exact():
    assert 3 * 2 * 512 + 2 < 2 ** 24                                # forward: |x w| <= 6 per term, K = 512 terms, plus the bias
    assert 3 * 2 * 128 < 2 ** 24 and 3 * 3 * 63 < 2 ** 24           # dx over N = 128, dW / db over at most 63 rows
    for M, K, N in [(m, 512, 128) for m in hr.LINEAR_FWD_ROWS] + hr.LINEAR_BWD_CASES:
        x, w, b, dout = hr.linear_int_inputs(M, K, N)
        for t, bound in ((x, 3), (w, 2), (b, 2), (dout, 3)):
            assert float(t.abs().max()) <= bound and torch.equal(t, t.to(torch.bfloat16).float())       # exact as bf16 operands
        y = x @ w.t() + b
        assert torch.equal(y.double(), x.double() @ w.double().t() + b.double())
        for act in (0, 1):
            out = torch.relu(y) if act else y
            dx, dw, db = hr.linear_bwd_reference(x, w, out, dout, act)
            dx64, dw64, db64 = hr.linear_bwd_reference(x.double(), w.double(), out.double(), dout.double(), act)
            assert torch.equal(dx.double(), dx64) and torch.equal(dw.double(), dw64) and torch.equal(db.double(), db64)


@pytest.mark.parametrize("act", [0, 1, 2])
def test_linear_backward_restatement_is_autograd(act):
    M, K, N = hr.LINEAR_TANH
    x, w, b, dout = [t.double() for t in hr.linear_real_inputs(M, K, N)]
    xr, wr, br = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
    f = {0: lambda v: v, 1: torch.relu, 2: torch.tanh}[act]
    out = f(xr @ wr.t() + br)
    out.backward(dout)
    dx, dw, db = hr.linear_bwd_reference(x, w, out.detach(), dout, act)
    np.testing.assert_allclose(dx.numpy(), xr.grad.numpy(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(dw.numpy(), wr.grad.numpy(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(db.numpy(), br.grad.numpy(), rtol=1e-12, atol=1e-14)


# ------------------------------------------------------------------------------------------------ row normalise, column sum
@pytest.mark.parametrize("rows,D", hr.L2NORM_CASES)
def test_l2norm_restatement_is_autograd(rows, D):
    x, dz = hr.l2norm_inputs(rows, D)
    z, dx = hr.l2norm_reference(x.numpy(), dz.numpy())
    xr = x.double().requires_grad_()
    zr = F.normalize(xr, dim=1)
    zr.backward(dz.double())
    np.testing.assert_allclose(z, zr.detach().numpy(), rtol=1e-14, atol=0)
    np.testing.assert_allclose(dx, xr.grad.numpy(), rtol=1e-9, atol=1e-15)
    if rows > 1:
        assert not x[1].any() and not z[1].any()
        np.testing.assert_allclose(dx[1], dz[1].double().numpy() / hr.L2_EPS, rtol=1e-15)        # the all-zero row: dz / eps


def test_colsum_cases_are_exact():
    for M, C in hr.COLSUM_CASES:
        m = hr.ints((M, C), -3, 3, 11)
        assert 3 * M < 2 ** 24 and torch.equal(m.sum(0).double(), m.double().sum(0))
