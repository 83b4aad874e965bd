"""GPU: the branches of the loss, head, embedding and ranking kernels that no other test launches (csrc/ntxent.hip, retrieval.hip,
linear_small.hip and the embedding / row kernels of misc.hip), called through the tricolo_amd.ops wrappers so that the branch named in
each docstring is the one that runs.  References, inputs and case lists: tests/head_reference.py; what makes the assertions mean
something (defect sensitivity, tie share, integer exactness): tests/test_head_reference_cpu.py; measured figures:
profiles/r19/NOTES_head_paths.md (every test prints its figures as a `HEADPATH` line before it asserts)."""
from itertools import combinations

import numpy as np
import pytest
import torch

from tests import head_reference as hr

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tricolo_amd import ops

DEV = "cuda"
T, ALPHA = hr.T, hr.ALPHA


def report(case, **figures):
    print("HEADPATH " + case + " " + " ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in figures.items()))


def amax(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def check_ntxent(case, loss, dza, dzb, ref, restated=None, skip_row=None):
    """loss within 2e-5 and gradients within atol 1e-6 of float64 (the tolerances of test_ntxent_large_batch_against_float64)."""
    l64, da, db = ref
    dza, dzb = dza.cpu().numpy(), dzb.cpu().numpy()
    keep = np.ones(da.shape[0], bool)
    if skip_row is not None:
        keep[skip_row] = False
    fig = dict(loss_err=abs(float(loss) - l64), grad_err=max(amax(dza[keep], da[keep]), amax(dzb, db)),
               grad_max=float(max(np.abs(da[keep]).max(), np.abs(db).max())))
    if restated is not None:
        fig.update(fp32_loss_err=abs(restated[0] - l64), fp32_grad_err=max(amax(restated[1][keep], da[keep]), amax(restated[2], db)))
    report(case, **fig)
    assert abs(float(loss) - l64) < hr.NTX_LOSS_TOL
    np.testing.assert_allclose(dza[keep], da[keep], rtol=0, atol=hr.NTX_GRAD_ATOL)
    np.testing.assert_allclose(dzb, db, rtol=0, atol=hr.NTX_GRAD_ATOL)


# ------------------------------------------------------------------------------------------------ NT-Xent
@pytest.mark.parametrize("B,D", hr.NTX_TILED)
def test_ntxent_tiled_similarity_kernel(B, D):
    """ntx_sim_kernel, the 64 x 64 LDS-tiled similarity (B > 512 or D % 4 != 0): (70, 18) has a ragged tile on both axes and a ragged
    second K chunk, (130, 6) three tiles per axis and one short K chunk, (513, 8) selects it on B alone with a last tile of one row."""
    from oracle.modules import nt_xent_numpy
    assert B > 512 or D % 4
    za, zb = hr.ntx_inputs(B, D)
    loss, dza, dzb = ops.ntxent_fwd_bwd(za.to(DEV), zb.to(DEV), T, ALPHA)
    check_ntxent(f"ntxent_tiled_{B}x{D}", loss.item(), dza, dzb, nt_xent_numpy(za.numpy(), zb.numpy(), T, ALPHA), hr.nt_xent_torch(za, zb))


def test_ntxent_tiled_similarity_kernel_without_normalise():
    """ntx_sim_kernel reading za / zb themselves (norm=False: no ntxm_l2norm_kernel, ntxm_grad_kernel without the Jacobian) at (70, 18),
    on rows normalised in float64 on the host so that the logits keep their scale."""
    B, D = hr.NTX_TILED[0]
    za, zb = [hr.normalise_rows_f64_to_f32(z) for z in hr.ntx_inputs(B, D)]
    loss, dza, dzb = ops.ntxent_fwd_bwd(za.to(DEV), zb.to(DEV), T, ALPHA, norm=False)
    check_ntxent(f"ntxent_tiled_nonorm_{B}x{D}", loss.item(), dza, dzb, hr.nt_xent_f64(za.numpy(), zb.numpy(), norm=False),
                 hr.nt_xent_torch(za, zb, norm=False))


@pytest.mark.parametrize("B,D", hr.NTX_WIDE)
def test_ntxent_wide_rows(B, D):
    """ntxm_grad_kernel register slots g[2..7] with one pair: D = 2048 fills all eight (the limit), D = 1284 leaves slot 5 ragged and
    6, 7 empty.  (ntxm_sim_rows_kernel computes the similarities: B <= 512, D % 4 == 0.)"""
    from oracle.modules import nt_xent_numpy
    za, zb = hr.ntx_inputs(B, D)
    loss, dza, dzb = ops.ntxent_fwd_bwd(za.to(DEV), zb.to(DEV), T, ALPHA)
    check_ntxent(f"ntxent_wide_{B}x{D}", loss.item(), dza, dzb, nt_xent_numpy(za.numpy(), zb.numpy(), T, ALPHA), hr.nt_xent_torch(za, zb))


@pytest.mark.parametrize("B,D", hr.NTX_WIDE)
def test_ntxent_all_pairs_wide_rows(B, D):
    """ntxm_grad_kernel register slots g[2..7] (and ntxm_sim_rows_kernel's second trip of the k += 1024 row fill at D = 2048), M = 3 with
    dtotal = 1: every embedding's gradient is the sum of the float64 gradients of its two pairs."""
    from oracle.modules import nt_xent_numpy
    assert ops.ntxent_multi_supported(B, D, 3)
    zs = hr.ntx_inputs(B, D, M=3)
    zd = [z.to(DEV) for z in zs]
    losses, ws = ops.ntxent_multi_fwd(zd, T, ALPHA)
    dzs = ops.ntxent_multi_bwd(zd, ws, T, ALPHA, dtotal=torch.ones((), dtype=torch.float32, device=DEV))
    acc, l64 = [np.zeros((B, D)) for _ in range(3)], []
    for a, b in combinations(range(3), 2):
        l, da, db = nt_xent_numpy(zs[a].numpy(), zs[b].numpy(), T, ALPHA)
        l64.append(l)
        acc[a] += da
        acc[b] += db
    losses = losses.cpu().numpy().astype(np.float64)
    report(f"ntxent_multi_wide_{B}x{D}", loss_err=float(np.abs(losses[:3] - l64).max()), total_err=abs(losses[3] - sum(l64)),
           grad_err=max(amax(dzs[m].cpu().numpy(), acc[m]) for m in range(3)), grad_max=float(max(np.abs(a).max() for a in acc)))
    for q in range(3):
        assert abs(losses[q] - l64[q]) < hr.NTX_LOSS_TOL
    assert abs(losses[3] - sum(l64)) < 3 * hr.NTX_LOSS_TOL                         # three pair losses, each within the pair tolerance
    for m in range(3):
        np.testing.assert_allclose(dzs[m].cpu().numpy(), acc[m], rtol=0, atol=hr.NTX_GRAD_ATOL)


def test_ntxent_at_the_batch_limit():
    """(8192, 4), the single-pair limit on B: ntxm_grad_kernel's B coefficients are 32 KiB of LDS, the one shape at which its request
    is near the 64 KiB a launch gets (two pairs' worth would not launch); ntx_sim_kernel computes the similarities."""
    from oracle.modules import nt_xent_numpy
    B, D = hr.NTX_BATCH_LIMIT
    za, zb = hr.ntx_inputs(B, D)
    loss, dza, dzb = ops.ntxent_fwd_bwd(za.to(DEV), zb.to(DEV), T, ALPHA)
    check_ntxent(f"ntxent_limit_{B}x{D}", loss.item(), dza, dzb, nt_xent_numpy(za.numpy(), zb.numpy(), T, ALPHA))


def test_ntxent_split_forward_backward_on_the_tiled_path():
    """ops.ntxent_fwd then ops.ntxent_bwd at (70, 18): ntx_sim_kernel fills the workspace, tri_ntxent_bwd reads S, the lse vectors, the
    normalised rows and the norms back from it and ntxm_grad_kernel folds dloss = 0.5 into its coefficients."""
    from oracle.modules import nt_xent_numpy
    B, D = hr.NTX_TILED[0]
    za, zb = hr.ntx_inputs(B, D)
    zad, zbd = za.to(DEV), zb.to(DEV)
    loss, ws = ops.ntxent_fwd(zad, zbd, T, ALPHA)
    dza, dzb = ops.ntxent_bwd(zad, zbd, ws, T, ALPHA, dloss=torch.full((), 0.5, dtype=torch.float32, device=DEV))
    l64, da, db = nt_xent_numpy(za.numpy(), zb.numpy(), T, ALPHA)
    check_ntxent(f"ntxent_split_{B}x{D}", loss.item(), dza, dzb, (l64, 0.5 * da, 0.5 * db))


def test_ntxent_all_zero_row():
    """(6, 20) with row 2 of za zero, norm=True: ntxm_l2norm_kernel's max(|x|, eps) clamp and ntxm_grad_kernel's 1 / max(norm, eps).  The
    loss is finite; row 2's gradient is da_hat / eps, O(1e11), compared relatively."""
    from oracle.modules import nt_xent_numpy
    B, D = hr.NTX_ZERO_ROW
    row = hr.NTX_ZERO_ROW_INDEX
    za, zb = hr.ntx_inputs(B, D)
    za[row] = 0
    loss, dza, dzb = ops.ntxent_fwd_bwd(za.to(DEV), zb.to(DEV), T, ALPHA)
    ref = nt_xent_numpy(za.numpy(), zb.numpy(), T, ALPHA)
    got = dza.cpu().numpy()[row].astype(np.float64)
    report("ntxent_zero_row", row_rel_err=float((np.abs(got - ref[1][row]) / np.abs(ref[1][row])).max()), row_min=float(np.abs(ref[1][row]).min()))
    assert np.isfinite(loss.item())
    check_ntxent("ntxent_zero_row_others", loss.item(), dza, dzb, ref, hr.nt_xent_torch(za, zb), skip_row=row)
    np.testing.assert_allclose(got, ref[1][row], rtol=1e-5, atol=0)


def test_ntxent_rejections():
    """The single-pair argument check (1 <= B <= 8192, 1 <= D <= 2048: ntxm_grad_kernel holds a row in eight register slots and
    B coefficients per pair in LDS), in tri_ntxent_fwd_bwd and in tri_ntxent_bwd, and the all-pairs range."""
    for B, D in [(4, 2052), (4, 0), (8193, 4)]:
        za, zb = torch.zeros(B, D, device=DEV), torch.zeros(B, D, device=DEV)
        with pytest.raises(RuntimeError, match="tri_ntxent"):
            ops.ntxent_fwd_bwd(za, zb, T, ALPHA)
        with pytest.raises(RuntimeError, match="tri_ntxent"):
            ops.ntxent_fwd(za, zb, T, ALPHA)
        ws = torch.empty(ops.lib().tri_ntxent_workspace(B, D), dtype=torch.uint8, device=DEV)
        with pytest.raises(RuntimeError, match="tri_ntxent"):
            ops.ntxent_bwd(za, zb, ws, T, ALPHA)
    assert not ops.ntxent_multi_supported(8, 2, 3)
    assert not ops.ntxent_multi_supported(8, 2052, 3)
    assert not ops.ntxent_multi_supported(513, 512, 3)
    for B, D in [(8, 2), (8, 2052), (513, 8)]:                                      # ... and the library agrees with the Python predicate
        with pytest.raises(RuntimeError, match="tri_ntxent_multi"):
            ops.ntxent_multi_fwd([torch.zeros(B, D, device=DEV) for _ in range(3)], T, ALPHA)


# ------------------------------------------------------------------------------------------------ retrieval ranking
def check_retrieval(txt, shp, lab, k, exact):
    idx, sim, hit = ops.retrieval_topk(torch.from_numpy(txt).to(DEV), torch.from_numpy(shp).to(DEV), torch.from_numpy(lab).to(DEV), k=k)
    top, top_sims, first_hit, _ = hr.retrieval_reference(txt, shp, lab, k)
    np.testing.assert_array_equal(idx.cpu().numpy(), top)
    np.testing.assert_array_equal(hit.cpu().numpy(), first_hit)
    if exact:
        np.testing.assert_array_equal(sim.cpu().numpy(), top_sims)
    else:
        np.testing.assert_allclose(sim.cpu().numpy(), top_sims, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("case", hr.RETRIEVAL_INT, ids=str)
def test_retrieval_ranking_integer_exact(case):
    """retrieval_topk_kernel: (64, 400, 80, 5) and (32, 686, 520, 5) take the second / third trip of every `s += 256` loop, the latter also
    the query fill's `d += 256` trips and D % 64 != 0; (8, 257, 4, 1) is k == 1 with one shape in the second trip and D < 64;
    (4, 7, 68, 7) is k == Ns, every shape retired.  Integer similarities: indices, similarities and first_hit must be EQUAL."""
    Nq, Ns, D, k = case
    check_retrieval(*hr.retrieval_int_inputs(Nq, Ns, D), k, exact=True)


def test_retrieval_ranking_float_at_the_evaluation_width():
    """retrieval_topk_kernel at D = 512 (the real evaluation's width: two trips of the query fill, eight of the dot product) with
    Ns = 300 real-valued, well-separated similarities."""
    Nq, Ns, D, k = hr.RETRIEVAL_FLOAT
    check_retrieval(*hr.retrieval_float_inputs(Nq, Ns, D), k, exact=False)


def test_retrieval_ranking_at_the_lds_limit():
    """tri_retrieval_topk at exactly Ns + D = 19200 (150 KiB of dynamic LDS per workgroup, granted through hipFuncSetAttribute, whose
    result the wrapper checks): Nq = 2, Ns = 19136, D = 64, integer inputs, must rank correctly."""
    Nq, Ns, D, k = hr.RETRIEVAL_LIMIT
    assert Ns + D == hr.RETRIEVAL_LDS_LIMIT
    check_retrieval(*hr.retrieval_int_inputs(Nq, Ns, D), k, exact=True)


def test_retrieval_rejections():
    """tri_retrieval_topk's argument checks: 1 <= k <= Ns and Ns + D <= 19200."""
    txt, shp, lab = [torch.from_numpy(a).to(DEV) for a in hr.retrieval_int_inputs(4, 7, 68)]
    for k in (0, 8):
        with pytest.raises(RuntimeError, match="1 <= k <= number of shapes"):
            ops.retrieval_topk(txt, shp, lab, k=k)
    with pytest.raises(RuntimeError, match="19200"):
        ops.retrieval_topk(torch.zeros(2, 64, device=DEV), torch.zeros(19137, 64, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV), k=5)


# ------------------------------------------------------------------------------------------------ embedding
@pytest.mark.parametrize("case", hr.EMBEDDING_CASES, ids=str)
def test_embedding_weight_gradient_and_lookup(case):
    """embedding_bwd_kernel: (24, 96, 50, 256) has 2304 tokens - a second, ragged trip of the `base += 2048` scan; (172, 96, 16, 8) has
    16512 tokens - 258 mask words, a second trip of the `w += 256` clear; (7, 96, 50, 300) takes a second, ragged trip of the
    `d += 256` column loop.  Integer dout: EQUAL to F.embedding's autograd; the padding row and the unused entry V - 1 stay zero."""
    B, L, V, D = case
    tok, w, dout = hr.embedding_inputs(B, L, V, D)
    out_ref, dw_ref = hr.embedding_reference(tok, w, dout)
    assert torch.equal(ops.embedding_fwd(tok.to(DEV), w.to(DEV)).cpu(), out_ref)
    dw = ops.embedding_bwd(tok.to(DEV), dout.to(DEV), V).cpu()
    assert torch.equal(dw, dw_ref)
    assert torch.count_nonzero(dw[0]) == 0 and torch.count_nonzero(dw[V - 1]) == 0


def test_embedding_lookup_rejects_rows_it_cannot_read_as_float4():
    """tri_embedding_fwd: D % 4 != 0."""
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.embedding_fwd(torch.zeros(2, 3, dtype=torch.int32, device=DEV), torch.zeros(5, 6, device=DEV))


# ------------------------------------------------------------------------------------------------ linear_small
@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("M", hr.LINEAR_FWD_ROWS)
def test_linear_small_forward_fast_path_ragged_rows(M, act, precision):
    """linear_small_fwd_kernel's `MT <= 2 && K == 512` path (all loads first; rows past M read row 0 and are masked by `ok`) at ragged
    row counts: one tile ragged (1, 5), full (16), a second tile of 1 and of 15 rows (17, 31).  Integer inputs: EQUAL."""
    K, N = 512, 128
    assert ops.linear_small_supported(M, K, N)
    x, w, b, _ = hr.linear_int_inputs(M, K, N)
    ref = x @ w.t() + b
    out = ops.linear_small_fwd(x.to(DEV), w.to(DEV), b.to(DEV), act, precision)
    assert torch.equal(out.cpu(), torch.relu(ref) if act else ref)


@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("M,K,N", hr.LINEAR_BWD_CASES)
def test_linear_small_backward_ragged_rows(M, K, N, act, precision):
    """linear_small_bwd_kernel / linear_small_wgrad_kernel: 33 <= M <= 63 makes the SECOND 32-row contraction step of the weight gradient
    ragged (and the data gradient's third / fourth row tile), M = 5, 17 the first, behind the K = 512 forward.  Integer inputs, the ReLU
    mask from the kernel's own (exact) forward output: dx, dw, db EQUAL; need_dx=False gives the same dw, db bit for bit."""
    x, w, b, dout = hr.linear_int_inputs(M, K, N)
    xd, wd, dd = x.to(DEV), w.to(DEV), dout.to(DEV)
    out = ops.linear_small_fwd(xd, wd, b.to(DEV), act, precision)
    ref = x @ w.t() + b
    assert torch.equal(out.cpu(), torch.relu(ref) if act else ref)
    dx, dw, db = ops.linear_small_bwd(xd, wd, out, dd, act, precision)
    rx, rw, rb = hr.linear_bwd_reference(x, w, out.cpu(), dout, act)
    assert torch.equal(dx.cpu(), rx) and torch.equal(dw.cpu(), rw) and torch.equal(db.cpu(), rb)
    none, dw1, db1 = ops.linear_small_bwd(xd, wd, out, dd, act, precision, need_dx=False)
    assert none is None and torch.equal(dw1, dw) and torch.equal(db1, db)


@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
def test_linear_small_tanh_head_ragged_rows(precision):
    """act = 2 (tanh and its 1 - y^2 derivative) on the K = 512 forward fast path at M = 17, real inputs against float64 with the
    tolerances of test_linear_small_matches_torch (2e-5 bf16x3, 3e-2 bf16; x 20 on dw, x 4 on db)."""
    M, K, N = hr.LINEAR_TANH
    x, w, b, dout = hr.linear_real_inputs(M, K, N)
    xd, wd, dd = x.to(DEV), w.to(DEV), dout.to(DEV)
    out = ops.linear_small_fwd(xd, wd, b.to(DEV), 2, precision)
    dx, dw, db = ops.linear_small_bwd(xd, wd, out, dd, 2, precision)
    ref = torch.tanh(x.double() @ w.double().t() + b.double())
    o = out.cpu().double()                                          # derivative from the kernel's own forward output, as the kernel takes it
    rx, rw, rb = hr.linear_bwd_reference(x.double(), w.double(), o, dout.double(), 2)
    out32 = torch.tanh(x @ w.t() + b)                               # the fp32 restatement's own error, each side with its own forward output
    f32, f64 = hr.linear_bwd_reference(x, w, out32, dout, 2), hr.linear_bwd_reference(x.double(), w.double(), ref, dout.double(), 2)
    report(f"linear_tanh_{precision}", out_err=amax(out.cpu(), ref), dx_err=amax(dx.cpu(), rx), dw_err=amax(dw.cpu(), rw), db_err=amax(db.cpu(), rb),
           fp32_out_err=amax(out32, ref), fp32_dx_err=amax(f32[0], f64[0]), fp32_dw_err=amax(f32[1], f64[1]), fp32_db_err=amax(f32[2], f64[2]))
    tol = hr.LINEAR_TOL[precision]
    np.testing.assert_allclose(out.cpu().numpy(), ref.numpy(), atol=tol, rtol=tol)
    np.testing.assert_allclose(dx.cpu().numpy(), rx.numpy(), atol=tol, rtol=tol)
    np.testing.assert_allclose(dw.cpu().numpy(), rw.numpy(), atol=tol * 20, rtol=tol)
    np.testing.assert_allclose(db.cpu().numpy(), rb.numpy(), atol=tol * 4, rtol=tol)


@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
def test_linear_small_without_bias_and_bias_gradient(precision):
    """linear_small_fwd_kernel with bias == nullptr and the weight-gradient body with db == nullptr (one-launch backward and the
    weight-gradient entry point alone): the biased results minus the bias, the need_db=True results minus db."""
    M, K, N = 17, 512, 128
    x, w, b, dout = hr.linear_int_inputs(M, K, N)
    xd, wd, dd = x.to(DEV), w.to(DEV), dout.to(DEV)
    for act in (0, 1):
        ref = x @ w.t()
        out = ops.linear_small_fwd(xd, wd, None, act, precision)
        assert torch.equal(out.cpu(), torch.relu(ref) if act else ref)
        if act == 0:
            assert torch.equal(out.cpu(), ops.linear_small_fwd(xd, wd, b.to(DEV), 0, precision).cpu() - b)
        dx, dw, db = ops.linear_small_bwd(xd, wd, out, dd, act, precision)
        dx0, dw0, db0 = ops.linear_small_bwd(xd, wd, out, dd, act, precision, need_db=False)
        assert db0 is None and torch.equal(dx0, dx) and torch.equal(dw0, dw)
        none, dw1, db1 = ops.linear_small_bwd(xd, wd, out, dd, act, precision, need_dx=False, need_db=False)
        assert none is None and db1 is None and torch.equal(dw1, dw)
        rx, rw, rb = hr.linear_bwd_reference(x, w, out.cpu(), dout, act)
        assert torch.equal(dx.cpu(), rx) and torch.equal(dw.cpu(), rw) and torch.equal(db.cpu(), rb)


def test_linear_small_declines_what_it_cannot_tile():
    """tri_linear_small_supported: rows <= 64, K % 128 == 0, N % 128 == 0."""
    assert ops.linear_small_supported(64, 512, 128)
    assert not ops.linear_small_supported(65, 512, 128)
    assert not ops.linear_small_supported(32, 192, 128)
    assert not ops.linear_small_supported(32, 512, 64)
    with pytest.raises(RuntimeError, match="linear_small"):
        ops.linear_small_fwd(torch.zeros(65, 512, device=DEV), torch.zeros(128, 512, device=DEV), None, 0, "bf16x3")


# ------------------------------------------------------------------------------------------------ row normalise, column sum
@pytest.mark.parametrize("rows,D", hr.L2NORM_CASES)
def test_l2norm_ragged_rows_and_widths(rows, D):
    """l2norm_fwd_kernel / l2norm_bwd_kernel, one wave per row, four rows per workgroup: (1, 4) is D < 64 with three idle waves, (5, 70)
    D % 64 != 0 with rows % 4 != 0 (a second workgroup of one row), (6, 512) the unrolled full-width loop with a ragged second
    workgroup.  Row 1 of the last two is all zero: z = 0 and dx = dz / eps."""
    x, dz = hr.l2norm_inputs(rows, D)
    z64, dx64 = hr.l2norm_reference(x.numpy(), dz.numpy())
    z, norm = ops.l2norm_fwd(x.to(DEV))
    dx = ops.l2norm_bwd(z, norm, dz.to(DEV)).cpu().numpy()
    live = np.ones(rows, bool)
    if rows > 1:
        live[1] = False
    report(f"l2norm_{rows}x{D}", fwd_err=amax(z.cpu(), z64), bwd_err=amax(dx[live], dx64[live]), norm_err=amax(norm.cpu(), np.linalg.norm(x.double().numpy(), axis=1)))
    np.testing.assert_allclose(z.cpu().numpy(), z64, rtol=0, atol=1e-7)
    np.testing.assert_allclose(norm.cpu().numpy(), np.linalg.norm(x.double().numpy(), axis=1), rtol=1e-6, atol=0)
    np.testing.assert_allclose(dx[live], dx64[live], rtol=1e-4, atol=1e-6)
    if rows > 1:
        assert float(norm[1]) == 0.0 and not z[1].any()
        np.testing.assert_allclose(dx[1], dx64[1], rtol=1e-4, atol=0)


@pytest.mark.parametrize("M,C", hr.COLSUM_CASES)
def test_colsum_ragged(M, C):
    """colsum_kernel, 64 columns per workgroup, four row phases: (3, 1) is M < 4 and C < 64, (1, 130) one row over three workgroups,
    the last with two columns, (1031, 70) M % 4 != 0 with a ragged second workgroup.  Integer inputs: EQUAL."""
    m = hr.ints((M, C), -3, 3, 11)
    assert torch.equal(ops.colsum(m.to(DEV)).cpu(), m.sum(0))
