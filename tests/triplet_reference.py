"""Float64 numpy restatement of the reference's TripletLoss (tricolo/loss/triplet.py) with its gradients in closed form.

tests/test_triplet_golden.py pins it to the REAL class on every case of tests/golden/triplet.npz (loss, both gradients, set sizes);
the GPU tests then use it as the comparator for inputs the fixture does not hold.  Importable without a GPU.

    sq[i][j] = |zls[j]|^2 - 2 <zls[i], zis[j]> + |zis[i]|^2        (the reference's swapped norms, kept)
    d = sqrt(max(sq, 0)), gradient 0 where sq <= 0
    S = {(i, j), j != i : d[i][i] < d[i][j] < d[i][i] + margin},  H = {(i, j), j != i : d[i][j] < d[i][i]}
    loss = mean over S (over H when S is empty) of d[i][i] - d[i][j] + margin;  NaN, with NaN gradients, when both are empty
"""
from types import SimpleNamespace

import numpy as np


def make_inputs(kind, B, D, r, s, seed, normalise=True):
    """The fixture's input recipes as fp32 torch tensors (the fixture stores seeds, not arrays).  clustered: a rank-r latent shared by the two modalities plus independent noise; separated: a full-rank latent and little noise;
    duplicates: a fixed integer-valued pair with repeated rows, so that sq is exactly 0 at some entries (see below)."""
    import torch
    g = torch.Generator().manual_seed(int(seed))
    rn = lambda *shape: torch.randn(*shape, generator=g).double().numpy()       # noqa: E731
    # Only the generator's draws come from torch; the arithmetic is elementwise float64 numpy in a fixed order (no BLAS call, whose
    # summation order depends on the CPU), so that every machine rebuilds the same fp32 arrays - the fixture records their SHA-256.
    if kind in ("clustered", "separated"):
        if kind == "clustered":
            u, v = rn(B, r), rn(r, D) / D ** 0.5
            c = np.zeros((B, D))
            for k in range(r):
                c = c + u[:, k:k + 1] * v[k:k + 1, :]
        else:                                 # matched rows close, different samples far apart: what a trained net emits
            c = rn(B, D) / D ** 0.5
        a = c + s * rn(B, D) / D ** 0.5
        b = c + s * rn(B, D) / D ** 0.5
    elif kind == "duplicates":
        # B = 6, D = 8, entries in {-1, 0, 1}: every product, sum and sq is exact in fp32 and fp64 alike.  Rows 1 / 3 of zis copy
        # rows 0 / 2; zls = zis except one extra 1 in rows 0 and 2, so d[0][0] = d[2][2] = 1, the other d[i][i] are exactly 0,
        # d[0][1] = d[2][3] = 0 off the diagonal (hard negatives) and d[0][3] = d[0][4] = d[2][1] = d[2][4] = sqrt(2).
        a = torch.zeros(6, 8)
        a[0, 0] = a[1, 0] = a[2, 1] = a[3, 1] = 1.0
        a[4, :3] = 1.0
        a[5, 5], a[5, 6] = 1.0, -1.0
        b = a.clone()
        b[0, 3] += 1.0
        b[2, 4] += 1.0
        return a, b
    else:
        raise ValueError(kind)
    if normalise:
        a, b = a / np.sqrt((a * a).sum(1, keepdims=True)), b / np.sqrt((b * b).sum(1, keepdims=True))
    return torch.from_numpy(a.astype(np.float32)), torch.from_numpy(b.astype(np.float32))

def triplet(zis, zls, margin, upstream=1.0):
    """loss, dzis, dzls (times `upstream`), |S|, |H|, the branch taken and `gap`: the smallest distance of any candidate
    d[i][j] - d[i][i] to either threshold (0 and margin).  Everything in float64 from the values given."""
    zis, zls = np.asarray(zis, dtype=np.float64), np.asarray(zls, dtype=np.float64)
    B = zis.shape[0]
    dot = zls @ zis.T
    sq = ((zls * zls).sum(1)[None, :] - 2.0 * dot) + (zis * zis).sum(1)[:, None]
    pos = sq > 0
    d = np.where(pos, np.sqrt(np.where(pos, sq, 1.0)), 0.0)
    dii = np.diag(d)[:, None]
    off = ~np.eye(B, dtype=bool)
    semi = off & (dii < d) & (d < dii + margin)
    hard = off & (d < dii)
    diff = (d - dii)[off]
    gap = float(min(np.abs(diff).min(), np.abs(diff - margin).min()))
    sel = semi if semi.any() else hard
    n = int(sel.sum())
    out = SimpleNamespace(n_semi=int(semi.sum()), n_hard=int(hard.sum()), branch=0 if semi.any() else 1, gap=gap, d=d)
    if n == 0:
        out.loss = float("nan")
        out.dzis, out.dzls = np.full_like(zis, np.nan), np.full_like(zls, np.nan)
        return out
    out.loss = float(((dii - d + margin) * sel).sum() / n)
    inv2d = np.where(pos, 0.5 / np.where(pos, d, 1.0), 0.0)       # d d / d sq, cut where sq <= 0
    c = -(upstream / n) * sel * inv2d                             # d loss / d sq
    c[np.arange(B), np.arange(B)] += (upstream / n) * sel.sum(1) * np.diag(inv2d)
    out.dzls = -2.0 * c @ zis + 2.0 * c.sum(0)[:, None] * zls
    out.dzis = -2.0 * c.T @ zls + 2.0 * c.sum(1)[:, None] * zis
    return out


def rel_l2(x, ref):
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    den = np.linalg.norm(ref)
    return float(np.linalg.norm(x - ref) / den) if den > 0 else float(np.linalg.norm(x - ref))
