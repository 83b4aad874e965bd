"""Generate tests/golden/triplet.npz from the REAL reference class tricolo.loss.triplet.TripletLoss.  TEST INFRASTRUCTURE.

Runs only where the reference checkout is present (oracle.make_golden.REF); the fixture travels, the reference does not.

    python tools/make_triplet_golden.py

Per case: the inputs' recipe (tests/triplet_reference.make_inputs: kind, B, D, r, s, seed, normalise) and the SHA-256 of the fp32
arrays it yields; the reference's loss and both gradients computed in float64 (the fp32 inputs converted) and again in float32;
how far the float32 run is from the float64 one (relative on the loss, relative L2 on each gradient: the GPU tests' bound is
4 x the largest of these over all cases); the sizes of the semi-hard set S and the hard set H; and `gap`, the smallest float64
distance of any candidate d[i][j] - d[i][i] to either threshold (0 and margin).  A seed whose gap is below GAP_MIN is rejected and the
next one is taken (at most TRIES per case; the generator fails otherwise): a case is usable only if no candidate sits on a threshold.
Gradients are stored in full up to B x D = 32 x 512 and, above (a committed file stays under 1 MiB), as their L2 norm, the L2 norm
of every row and SAMPLE_ROWS whole rows.
"""
import hashlib
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import make_golden as mg            # noqa: E402
from tests import triplet_reference as tr      # noqa: E402

GAP_MIN, TRIES, FULL_ELEMS, SAMPLE_ROWS = 1e-5, 8, 32 * 512, 4

# tag, kind, B, D, r, s, margin, normalise, first seed
CASES = [
    ("semi_b32", "clustered", 32, 512, 3, 0.3, 0.025, True, 1),
    ("semi_b64", "clustered", 64, 512, 3, 0.3, 0.025, True, 1),
    ("dense_b48", "clustered", 48, 512, 2, 0.2, 0.025, True, 1),
    ("hard_b64", "clustered", 64, 512, 3, 0.3, 1e-6, True, 1),
    ("raw_b64", "clustered", 64, 512, 3, 0.3, 0.025, False, 3),
    ("raw_hard_b64", "clustered", 64, 512, 3, 0.3, 0.025, False, 9),
    ("tiny_b5", "clustered", 5, 64, 2, 0.3, 0.1, True, 2),
    ("tiny_b2", "clustered", 2, 512, 3, 2.0, 0.025, True, 1),
    ("tiny_b2_empty", "clustered", 2, 512, 3, 0.3, 0.025, True, 1),
    ("empty_b64", "separated", 64, 512, 0, 0.05, 0.025, True, 1),
    ("dup_semi", "duplicates", 6, 8, 0, 0.0, 0.5, False, 1),
    ("dup_hard", "duplicates", 6, 8, 0, 0.0, 0.25, False, 1),
    ("big_b200", "clustered", 200, 512, 3, 0.3, 0.025, True, 1),
    ("big_b512", "clustered", 512, 512, 3, 0.3, 0.025, True, 4),
]


def run_reference(cls, a, b, margin, dtype):
    zis, zls = a.clone().to(dtype).requires_grad_(), b.clone().to(dtype).requires_grad_()
    try:
        loss = cls(margin)(zis, zls)
    except ZeroDivisionError:                    # both sets empty: sum([]) / 0
        return None
    loss.backward()
    return float(loss.item()), zis.grad.double().numpy(), zls.grad.double().numpy()


def sample_rows(g):
    """SAMPLE_ROWS fixed rows: the first half rows that carry a gradient, the rest evenly spaced."""
    B = g.shape[0]
    nz = np.flatnonzero(np.abs(g).sum(1) > 0)[:SAMPLE_ROWS // 2]
    even = np.linspace(0, B - 1, SAMPLE_ROWS - len(nz)).astype(np.int64)
    return np.concatenate([nz, even]).astype(np.int64)


def main():
    mg.install_shims()
    from tricolo.loss.triplet import TripletLoss
    out, tags = {}, []
    for tag, kind, B, D, r, s, margin, normalise, seed0 in CASES:
        for seed in range(seed0, seed0 + TRIES):
            a, b = tr.make_inputs(kind, B, D, r, s, seed, normalise)
            mine = tr.triplet(a.numpy(), b.numpy(), margin)
            if mine.gap >= GAP_MIN:
                break
            print(f"{tag}: seed {seed} rejected, gap {mine.gap:.2e}")
        else:
            raise SystemExit(f"{tag}: no seed in {seed0}..{seed0 + TRIES - 1} keeps every candidate {GAP_MIN} off the thresholds")
        r64 = run_reference(TripletLoss, a, b, margin, torch.float64)
        r32 = run_reference(TripletLoss, a, b, margin, torch.float32)
        rec = {"kind": np.array(kind), "B": np.int64(B), "D": np.int64(D), "r": np.int64(r), "s": np.float64(s), "seed": np.int64(seed),
               "margin": np.float64(margin), "normalise": np.bool_(normalise),
               "sha256": np.array(hashlib.sha256(a.numpy().tobytes() + b.numpy().tobytes()).hexdigest()),
               "n_semi": np.int64(mine.n_semi), "n_hard": np.int64(mine.n_hard), "gap": np.float64(mine.gap)}
        if r64 is None:
            assert r32 is None and mine.n_semi == 0 and mine.n_hard == 0, tag
            rec["loss64"] = np.float64("nan")
        else:
            # the set sizes come from the restatement's masks; the reference's own sets show in its loss, which must agree
            assert abs(r64[0] - mine.loss) <= 1e-9 * abs(r64[0]), (tag, r64[0], mine.loss)
            rec.update({"loss64": np.float64(r64[0]), "loss32": np.float32(r32[0]),
                        "err_loss32": np.float64(abs(r32[0] - r64[0]) / abs(r64[0])),
                        "err_dzis32": np.float64(tr.rel_l2(r32[1], r64[1])), "err_dzls32": np.float64(tr.rel_l2(r32[2], r64[2]))})
            for name, g64, g32 in (("dzis", r64[1], r32[1]), ("dzls", r64[2], r32[2])):
                if B * D <= FULL_ELEMS:
                    rec[name + "64"], rec[name + "32"] = g64, g32.astype(np.float32)
                else:
                    rows = sample_rows(g64)
                    rec.update({name + "_rows": rows, name + "64_rows": g64[rows], name + "32_rows": g32[rows].astype(np.float32),
                                name + "64_norm": np.float64(np.linalg.norm(g64)), name + "32_norm": np.float64(np.linalg.norm(g32)),
                                name + "64_rownorms": np.linalg.norm(g64, axis=1)})
        print(f"{tag}: seed {seed} |S| {mine.n_semi} |H| {mine.n_hard} gap {mine.gap:.2e} loss64 {rec['loss64']:.9g} "
              + (f"fp32-vs-fp64 loss {rec['err_loss32']:.2e} dzis {rec['err_dzis32']:.2e} dzls {rec['err_dzls32']:.2e}" if r64 else "(both empty)"))
        out.update({f"{tag}/{k}": v for k, v in rec.items()})
        tags.append(tag)
    out["cases"] = np.array(tags)
    errs = {k: max(float(out[f"{t}/err_{k}32"]) for t in tags if f"{t}/err_{k}32" in out) for k in ("loss", "dzis", "dzls")}
    out["max_err_loss32"], out["max_err_grad32"] = np.float64(errs["loss"]), np.float64(max(errs["dzis"], errs["dzls"]))
    print(f"reference fp32 against fp64, largest over the cases: loss {errs['loss']:.3e}, gradient {max(errs['dzis'], errs['dzls']):.3e}")
    path = os.path.join(mg.GOLD, "triplet.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
