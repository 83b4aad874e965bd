"""float64 numpy restatement of NT-Xent with a learnable temperature (CLIP's logit scale), shared by tests/test_ntxent_temperature_cpu.py
and tests/test_gpu_ntxent_temperature.py.  TEST INFRASTRUCTURE.

s = clamp(logit_scale, 0, max_logit_scale) is taken in fp32, as the kernels take it; 1 / T = exp(float64(s)).  With S = exp(s) C the
gradient is d loss / d logit_scale = [0 <= logit_scale <= max] * sum_ij G_ij S_ij, G = d loss / d S; the clamp's boundaries pass it, as
torch.clamp's backward does.
"""
import math
from itertools import combinations

import numpy as np
import torch

from tests import head_reference as hr

MAX_LOGIT_SCALE = math.log(100.0)                 # CLIP's clamp
LS_T01 = math.log(10.0)                           # T = 0.1, the temperature of every existing NT-Xent test

# (B, D) of the GPU cases: the row similarity kernel, the tiled one, the all-pairs forms
ROW_CASES = [(1, 4), (5, 4), (37, 260), (300, 64), (16, 2048)]
TILED_CASES = [(70, 18), (513, 8)]
MULTI_CASES = [(37, 260), (300, 64)]
PAIR_UPSTREAMS = (0.5, -1.25, 2.0)                # per-pair upstreams of different values (first P of them)


def clamp_f32(logit_scale, max_logit_scale=MAX_LOGIT_SCALE):
    """(s, gate): the clamped scale as the fp32 number the kernels see, and whether the clamp passes the gradient."""
    ls, mx = np.float32(logit_scale), np.float32(max_logit_scale)
    s = np.float32(min(max(ls, np.float32(0.0)), mx))
    return s, bool(np.float32(0.0) <= ls <= mx)


def inv_temperature(logit_scale, max_logit_scale=MAX_LOGIT_SCALE):
    s, _ = clamp_f32(logit_scale, max_logit_scale)
    return float(np.exp(np.float64(s)))


def _pair_terms(za, zb, inv_T, alpha, norm):
    """loss, dza, dzb, sum G * S of one pair at upstream 1, and (G, S) themselves."""
    za, zb = np.asarray(za, np.float64), np.asarray(zb, np.float64)
    B = za.shape[0]
    if norm:
        na = np.maximum(np.linalg.norm(za, axis=1, keepdims=True), hr.NTX_EPS)
        nb = np.maximum(np.linalg.norm(zb, axis=1, keepdims=True), hr.NTX_EPS)
        a, b = za / na, zb / nb
    else:
        a, b = za, zb
    S = a @ b.T * inv_T
    row, col = hr._lse(S, 1), hr._lse(S, 0)
    d = np.diag(S)
    loss = alpha * (-(d - row).mean()) + (1 - alpha) * (-(d - col).mean())
    G = (alpha * (np.exp(S - row[:, None]) - np.eye(B)) + (1 - alpha) * (np.exp(S - col[None, :]) - np.eye(B))) / B
    da, db = G @ b * inv_T, G.T @ a * inv_T
    if norm:
        da = (da - a * (da * a).sum(1, keepdims=True)) / na
        db = (db - b * (db * b).sum(1, keepdims=True)) / nb
    return loss, da, db, float((G * S).sum()), G, S


def nt_xent_ls_f64(za, zb, logit_scale, max_logit_scale=MAX_LOGIT_SCALE, alpha=hr.ALPHA, norm=True):
    """(loss, dza, dzb, dlogit_scale) of one pair in float64."""
    _, gate = clamp_f32(logit_scale, max_logit_scale)
    loss, da, db, gs, _, _ = _pair_terms(za, zb, inv_temperature(logit_scale, max_logit_scale), alpha, norm)
    return loss, da, db, (gs if gate else 0.0)


def nt_xent_ls_all_pairs_f64(zs, logit_scale, max_logit_scale=MAX_LOGIT_SCALE, alpha=hr.ALPHA, norm=True, dpairs=None, dtotal=1.0):
    """M = 2 / 3 embeddings: (pair losses in combination order, total, [dz_m], dlogit_scale) with upstream dtotal on the total and
    dpairs[q] (None: zeros) on pair q - the earlier modality of a pair is the alpha side."""
    M = len(zs)
    pairs = list(combinations(range(M), 2))
    dpairs = [0.0] * len(pairs) if dpairs is None else list(dpairs)
    inv_T = inv_temperature(logit_scale, max_logit_scale)
    _, gate = clamp_f32(logit_scale, max_logit_scale)
    losses, dls = [], 0.0
    dzs = [np.zeros(np.asarray(z).shape, np.float64) for z in zs]
    for q, (a, b) in enumerate(pairs):
        loss, da, db, gs, _, _ = _pair_terms(zs[a], zs[b], inv_T, alpha, norm)
        up = dtotal + dpairs[q]
        losses.append(loss)
        dzs[a] += up * da
        dzs[b] += up * db
        dls += up * gs
    return losses, float(sum(losses)), dzs, (dls if gate else 0.0)


def nt_xent_ls_torch(zs, logit_scale, max_logit_scale=MAX_LOGIT_SCALE, alpha=hr.ALPHA, norm=True, dpairs=None, dtotal=1.0, dtype=torch.float64):
    """The reference's formula (F.normalize, matmul / temperature, two cross entropies) with temperature = exp(-clamp(logit_scale)), through
    torch autograd on the CPU in `dtype`, over every pair of `zs`: (pair losses, [dz_m], dlogit_scale).  float64 checks the restatement;
    float32 is the 'plain fp32 evaluation' whose error sets the bound on dlogit_scale."""
    F = torch.nn.functional
    ls = torch.tensor(float(np.float32(logit_scale)), dtype=dtype, requires_grad=True)
    z0 = [z.to(dtype).clone().requires_grad_() for z in zs]
    zn = [F.normalize(z, dim=1) for z in z0] if norm else z0
    temperature = torch.exp(-torch.clamp(ls, 0.0, float(np.float32(max_logit_scale))))
    pairs = list(combinations(range(len(zs)), 2))
    dpairs = [0.0] * len(pairs) if dpairs is None else list(dpairs)
    labels = torch.arange(zs[0].shape[0])
    losses, root = [], 0.0
    for q, (a, b) in enumerate(pairs):
        S = zn[a] @ zn[b].t() / temperature
        loss = alpha * F.cross_entropy(S, labels) + (1 - alpha) * F.cross_entropy(S.t(), labels)
        losses.append(float(loss.detach()))
        root = root + (dtotal + dpairs[q]) * loss
    root.backward()
    return losses, [z.grad.double().numpy() for z in z0], float(ls.grad)


def adam_f64(p, grads, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    """torch.optim.Adam (L2 weight decay folded into the gradient, bias-corrected) on one float64 scalar over the gradients `grads`:
    (p, m, v) after the last step."""
    m = v = 0.0
    for t, g in enumerate(grads, 1):
        g = g + weight_decay * p
        m = betas[0] * m + (1 - betas[0]) * g
        v = betas[1] * v + (1 - betas[1]) * g * g
        p = p - lr * (m / (1 - betas[0] ** t)) / (math.sqrt(v / (1 - betas[1] ** t)) + eps)
    return p, m, v


def dls_mass(zs, logit_scale, max_logit_scale=MAX_LOGIT_SCALE, alpha=hr.ALPHA, norm=True, dpairs=None, dtotal=1.0):
    """sum_q |up_q| sum_ij |G^q_ij S^q_ij|: the size of the terms d loss / d logit_scale sums (the sum itself cancels to a fraction of it).
    The scale an fp32 evaluation's rounding error grows with, so the scale the bound on dlogit_scale is relative to."""
    inv_T = inv_temperature(logit_scale, max_logit_scale)
    mass = 0.0
    for q, (a, b) in enumerate(combinations(range(len(zs)), 2)):
        _, _, _, _, G, S = _pair_terms(zs[a], zs[b], inv_T, alpha, norm)
        mass += abs(dtotal + (dpairs[q] if dpairs is not None else 0.0)) * float(np.abs(G * S).sum())
    return mass


def gpu_cases():
    """(M, B, D, norm, dpairs) of every case tests/test_gpu_ntxent_temperature.py holds to the dlogit_scale bound."""
    cases = [(2, B, D, True, None) for B, D in ROW_CASES + TILED_CASES] + [(2, 70, 18, False, None)]
    for B, D in MULTI_CASES:
        for M in (2, 3):
            cases += [(M, B, D, True, None), (M, B, D, True, list(PAIR_UPSTREAMS[:M * (M - 1) // 2]))]
    return cases


def fp32_autograd_errors(scales=(("ln 10", LS_T01), ("0", 0.0), ("ln 100", MAX_LOGIT_SCALE))):
    """[(scale name, case, float64 dlogit_scale, |fp32 torch autograd on the CPU - float64|, mass)] over gpu_cases() at the scale of the
    cases and at both clamp boundaries: the measurement behind the GPU test's DLS_BOUND (4 x the largest error / mass)."""
    rows = []
    for name, ls in scales:
        for M, B, D, norm, dp in gpu_cases():
            zs = hr.ntx_inputs(B, D, M=M)
            if not norm:
                zs = [hr.normalise_rows_f64_to_f32(z) for z in zs]
            ref = nt_xent_ls_all_pairs_f64(zs, ls, norm=norm, dpairs=dp)[3]
            got = nt_xent_ls_torch(zs, ls, norm=norm, dpairs=dp, dtype=torch.float32)[2]
            rows.append((name, (M, B, D, norm, dp is not None), ref, abs(got - ref), dls_mass(zs, ls, norm=norm, dpairs=dp)))
    return rows


if __name__ == "__main__":
    worst = 0.0
    for name, case, ref, err, mass in fp32_autograd_errors():
        rel = err / mass if mass else 0.0
        worst = max(worst, rel)
        print(f"logit_scale = {name:6s} (M, B, D, norm, dpairs) = {case}: dlogit_scale {ref:+.6e}  fp32 error {err:.3e}  mass {mass:.4e}  error / mass {rel:.3e}")
    print(f"largest error / mass {worst:.4e}; four times that {4 * worst:.4e}")
