"""float64 numpy restatements of the small kernels behind the loss, the MLP heads, the token embedding and the retrieval metric, with
the inputs and case lists that tests/test_head_reference_cpu.py (CPU) and tests/test_gpu_head_paths.py (GPU) share.  TEST INFRASTRUCTURE.

Every case is there for one branch of a kernel's dispatch that the suite did not launch before (profiles/r19/NOTES_head_paths.md names
them).  Wherever the kernel's arithmetic is exact on integers the inputs are integer-valued and the GPU assertion is equality; the rest
carries the tolerances of the project's existing tests of the same kernels, and the CPU file proves on float64 references with a
planted defect that those tolerances still see the defect each shape is there for.
"""
import numpy as np
import torch

T, ALPHA = 0.1, 0.25
NTX_LOSS_TOL, NTX_GRAD_ATOL = 2e-5, 1e-6          # test_ntxent_large_batch_against_float64
NTX_EPS = 1e-12

# (B, D): ntx_sim_kernel (64 x 64 LDS tiles, K chunks of 16) runs when B > 512 or D % 4 != 0
NTX_TILED = [(70, 18), (130, 6), (513, 8)]
# (B, D): ntxm_grad_kernel register slots g[2..7] (D > 512), with one pair and with three
NTX_WIDE = [(5, 2048), (9, 1284)]
NTX_BATCH_LIMIT = (8192, 4)                       # the single-pair limit on B: ntxm_grad_kernel's coefficients fill 32 KiB of LDS
NTX_ZERO_ROW = (6, 20)
NTX_ZERO_ROW_INDEX = 2


# ------------------------------------------------------------------------------------------------ NT-Xent
def ntx_inputs(B, D, seed=None, M=2):
    """randn embeddings with the first half of modality 1 pulled towards modality 0 (test_ntxent_large_batch_against_float64)."""
    g = torch.Generator().manual_seed(1000 * B + D if seed is None else seed)
    zs = [torch.randn(B, D, generator=g) for _ in range(M)]
    zs[1][: B // 2] += zs[0][: B // 2] * 2
    return zs


def normalise_rows_f64_to_f32(z):
    """Rows normalised on the host in float64, rounded to fp32: what the norm=False cases feed, so that the logits keep the scale of
    the normalised cases."""
    z64 = z.double()
    return (z64 / z64.norm(dim=1, keepdim=True).clamp_min(NTX_EPS)).float()


def _lse(x, axis):
    m = x.max(axis=axis, keepdims=True)
    return (m + np.log(np.exp(x - m).sum(axis=axis, keepdims=True))).squeeze(axis)


def nt_xent_f64(za, zb, temperature=T, alpha=ALPHA, norm=True, defect=None):
    """loss, d loss / d za, d loss / d zb in float64.  norm=True is oracle.modules.nt_xent_numpy (the CPU test compares the two);
    norm=False takes the rows as they are: the gradient is da_hat, with no normalise Jacobian.

    defect plants what a wrong kernel branch would compute (CPU sensitivity test only):
      "drop_last_col"  the last feature column is missing from the similarity (a ragged last K chunk read short)
      "lse_skip_last"  the last row and the last column are missing from every log-sum-exp (a ragged last tile left unwritten)
      "zero_wide"      the contraction's columns >= 1024 come out zero (register slots g[4..7] never filled)"""
    za, zb = np.asarray(za, np.float64), np.asarray(zb, np.float64)
    B = za.shape[0]
    if norm:
        na = np.maximum(np.linalg.norm(za, axis=1, keepdims=True), NTX_EPS)
        nb = np.maximum(np.linalg.norm(zb, axis=1, keepdims=True), NTX_EPS)
        a, b = za / na, zb / nb
    else:
        a, b = za, zb
    S = (a[:, :-1] @ b[:, :-1].T if defect == "drop_last_col" else a @ b.T) / temperature
    if defect == "lse_skip_last":
        row, col = _lse(S[:, :-1], 1), _lse(S[:-1, :], 0)
    else:
        row, col = _lse(S, 1), _lse(S, 0)
    d = np.diag(S)
    loss = alpha * (-(d - row).mean()) + (1 - alpha) * (-(d - col).mean())
    P_row, P_col = np.exp(S - row[:, None]), np.exp(S - col[None, :])
    dS = (alpha * (P_row - np.eye(B)) + (1 - alpha) * (P_col - np.eye(B))) / B
    da_hat, db_hat = dS @ b / temperature, dS.T @ a / temperature
    if defect == "zero_wide":
        da_hat[:, 1024:] = 0.0
        db_hat[:, 1024:] = 0.0
    if not norm:
        return loss, da_hat, db_hat
    da = (da_hat - a * (da_hat * a).sum(1, keepdims=True)) / na
    db = (db_hat - b * (db_hat * b).sum(1, keepdims=True)) / nb
    return loss, da, db


def nt_xent_torch(za, zb, temperature=T, alpha=ALPHA, norm=True, dtype=torch.float32):
    """The loss as the model states it (F.normalize, two cross entropies) through torch autograd on the CPU in `dtype`: float64 checks
    nt_xent_f64, float32 is the 'restatement error' column of the notes."""
    a0, b0 = za.to(dtype).clone().requires_grad_(), zb.to(dtype).clone().requires_grad_()
    a, b = (torch.nn.functional.normalize(a0, dim=1), torch.nn.functional.normalize(b0, dim=1)) if norm else (a0, b0)
    S = a @ b.t() / temperature
    labels = torch.arange(S.shape[0])
    loss = alpha * torch.nn.functional.cross_entropy(S, labels) + (1 - alpha) * torch.nn.functional.cross_entropy(S.t(), labels)
    loss.backward()
    return float(loss.detach()), a0.grad.double().numpy(), b0.grad.double().numpy()


def ntx_defects(B, D):
    """The defects the shape (B, D) is there to catch."""
    out = []
    if D % 16:
        out.append("drop_last_col")
    if B % 64:
        out.append("lse_skip_last")
    if D > 1024:
        out.append("zero_wide")
    return out


# ------------------------------------------------------------------------------------------------ retrieval
# (Nq, Ns, D, k), integer-valued
RETRIEVAL_INT = [(64, 400, 80, 5), (32, 686, 520, 5), (8, 257, 4, 1), (4, 7, 68, 7)]
RETRIEVAL_FLOAT = (16, 300, 512, 5)
RETRIEVAL_LIMIT = (2, 19136, 64, 5)               # Ns + D == 19200: the documented limit of the per-query LDS ranking
RETRIEVAL_LDS_LIMIT = 19200


def retrieval_int_inputs(Nq, Ns, D, seed=None):
    """Shape rows from {-2..2}, a third of them repeated under new indices at the end; queries = a shape row + noise from {-1..1}.
    Every similarity is an integer below 2^24: exact in fp32 and fp64 in any summation order, so ties are exact on both sides.
    labels: index 0, index Ns - 1 (itself a copy), an original and its copy, then random."""
    rng = np.random.default_rng(7919 * Ns + D if seed is None else seed)
    nbase = (3 * Ns + 3) // 4
    base = rng.integers(-2, 3, (nbase, D))
    src = rng.permutation(nbase)[: Ns - nbase]                    # the copy at index nbase + i repeats row src[i]
    shp = np.concatenate([base, base[src]]).astype(np.float32)
    pick = np.concatenate([src[rng.integers(0, len(src), Nq // 2)], rng.integers(0, Ns, Nq - Nq // 2)])
    txt = (shp[pick] + rng.integers(-1, 2, (Nq, D))).astype(np.float32)
    lab = rng.integers(0, Ns, Nq)
    fixed = [0, Ns - 1, int(src[0]), nbase]
    lab[: min(Nq, 4)] = fixed[: min(Nq, 4)]
    return txt, shp, lab.astype(np.int32)


def retrieval_float_inputs(Nq, Ns, D, seed=3):
    rng = np.random.default_rng(seed)
    shp = rng.standard_normal((Ns, D)).astype(np.float32)
    txt = (shp[rng.integers(0, Ns, Nq)] + 0.25 * rng.standard_normal((Nq, D))).astype(np.float32)
    lab = rng.integers(0, Ns, Nq)
    lab[:2] = (0, Ns - 1)
    return txt, shp, lab.astype(np.int32)


def retrieval_reference(txt, shp, lab, k):
    """(top-k indices, their float64 similarities, first_hit, the full similarity matrix): a stable ascending argsort, flipped -
    larger similarity first, equal similarities with the HIGHER index first."""
    sims = txt.astype(np.float64) @ shp.astype(np.float64).T
    order = np.flip(np.argsort(sims, axis=1, kind="stable"), 1)
    top = order[:, :k]
    return top, np.take_along_axis(sims, top, 1), np.argmax(order == lab[:, None], axis=1), sims


def tie_share(sims, k):
    """Fraction of the queries with two equal similarities among their top k + 1."""
    srt = -np.sort(-sims, axis=1)[:, : k + 1]
    return float((np.diff(srt, axis=1) == 0).any(axis=1).mean())


# ------------------------------------------------------------------------------------------------ embedding
# (B, L, V, D)
EMBEDDING_CASES = [(24, 96, 50, 256), (172, 96, 16, 8), (7, 96, 50, 300)]


def embedding_inputs(B, L, V, D, seed=23):
    """tokens with many pads (token 0, a third of all positions) and one vocabulary entry (V - 1) that never occurs; integer-valued dout
    in time-major [L, B, D] so that any summation order is exact."""
    g = torch.Generator().manual_seed(seed + B)
    tok = torch.randint(0, V, (B, L), generator=g, dtype=torch.int32)
    tok[torch.rand(B, L, generator=g) < 1 / 3] = 0
    tok[tok == V - 1] = 1
    w = torch.randn(V, D, generator=g)
    w[0] = 0
    dout = torch.randint(-3, 4, (L, B, D), generator=g).to(torch.float32)
    return tok, w, dout


def embedding_reference(tok, w, dout):
    wr = w.clone().requires_grad_()
    out = torch.nn.functional.embedding(tok.t().contiguous().long(), wr, padding_idx=0)
    out.backward(dout)
    return out.detach(), wr.grad


# ------------------------------------------------------------------------------------------------ linear_small
LINEAR_FWD_ROWS = [1, 5, 16, 17, 31]              # K = 512, N = 128: the all-loads-first forward path, ragged row tiles
LINEAR_BWD_CASES = [(33, 256, 128), (47, 256, 128), (63, 256, 128), (5, 512, 128), (17, 512, 128)]
LINEAR_TANH = (17, 512, 128)
LINEAR_TOL = {"bf16x3": 2e-5, "bf16": 3e-2}       # test_linear_small_matches_torch


def ints(shape, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).to(torch.float32)


def linear_int_inputs(M, K, N):
    """x in [-3, 3], w in [-2, 2], b in [-2, 2], dout in [-3, 3]: every product and sum is a small integer, exact in bf16 operands
    with fp32 accumulation."""
    return ints((M, K), -3, 3, 1), ints((N, K), -2, 2, 2), ints((N,), -2, 2, 3), ints((M, N), -3, 3, 4)


def linear_real_inputs(M, K, N, seed=5):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / np.sqrt(K), torch.randn(N, generator=g),
            torch.randn(M, N, generator=g))


def linear_bwd_reference(x, w, out, dout, act):
    """(dx, dw, db) in the dtype of the inputs, the activation derivative taken from the forward output `out`."""
    dpre = dout * {0: torch.ones_like(out), 1: (out > 0).to(out.dtype), 2: 1 - out * out}[act]
    return dpre @ w, dpre.t() @ x, dpre.sum(0)


# ------------------------------------------------------------------------------------------------ row normalise, column sum
L2NORM_CASES = [(1, 4), (5, 70), (6, 512)]        # (rows, D); every case with more than one row has an all-zero row (row 1)
COLSUM_CASES = [(3, 1), (1, 130), (1031, 70)]     # (M, C)
L2_EPS = 1e-12


def l2norm_inputs(rows, D, seed=1):
    g = torch.Generator().manual_seed(seed + rows)
    x, dz = torch.randn(rows, D, generator=g), torch.randn(rows, D, generator=g)
    if rows > 1:
        x[1] = 0
    return x, dz


def l2norm_reference(x, dz, eps=L2_EPS):
    """z, dx in float64: z = x / max(|x|, eps); dx = (dz - z <dz, z>) / max(|x|, eps) - for x = 0 that is dz / eps, what the clamp in
    F.normalize gives."""
    x, dz = np.asarray(x, np.float64), np.asarray(dz, np.float64)
    n = np.maximum(np.linalg.norm(x, axis=1, keepdims=True), eps)
    z = x / n
    return z, (dz - z * (dz * z).sum(1, keepdims=True)) / n
