"""Generate tests/golden/shape_f1.npz from the REAL reference function calculate_f1._compute_sampling_metrics.  TEST INFRASTRUCTURE.

Runs only where the reference checkout is present (oracle.make_golden.REF); the fixture travels, the reference does not.

    python tools/make_shape_f1_golden.py

calculate_f1.py imports pytorch3d, jsonlines and tqdm and opens a dataset file when it is imported.  None of that is needed for the
function: the module is loaded with stub modules - pytorch3d.ops.knn_points is an exact float64 brute-force K = 1 search that returns
fp32 `dists` like the real one, the other names are empty stubs - from a temporary working directory that holds an empty val_map.json.

Per pair: its recipe (tests/shape_f1_reference.make_pair: kind, sizes, seed) and the SHA-256 of the fp32 clouds it yields; the
reference's F1 at every threshold; the float64 counts of decidable points below each threshold and of undecidable ones, per direction;
the float64 chamfer distance; and the float64 d2 of SAMPLE evenly spaced points per direction.  A seed with more than MAX_UNDECIDABLE
undecidable points (both directions together) at any threshold is rejected and the next one is taken, at most TRIES times.
"""
import importlib.util
import os
import sys
import tempfile
import types
from collections import namedtuple

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import make_golden as mg            # noqa: E402
from tests import shape_f1_reference as sr     # noqa: E402

TRIES, SAMPLE = 8, 512

# tag, kind, S_pred, S_gt, first seed
CASES = [
    ("unrelated_a", "unrelated", 10000, 10000, 11),
    ("unrelated_b", "unrelated", 10000, 10000, 12),
    ("near_a", "near", 10000, 10000, 21),
    ("near_b", "near", 10000, 10000, 22),
    ("identical", "identical", 10000, 10000, 31),
    ("small_unrelated", "unrelated", 2000, 1500, 41),
    ("small_near", "near", 1200, 2000, 51),
    ("small_identical", "identical", 777, 777, 61),
]


_SEEN = {}


def nn_bruteforce(p, q, chunk=256):
    """Exact float64 K = 1 search by exhaustion: d2 [S1] float64 (kept per input pair: the reference function is called per threshold)."""
    key = sr.sha256(p, q)
    if key not in _SEEN:
        _SEEN.clear()
        _SEEN[key] = _nn_bruteforce(p, q, chunk)
    return _SEEN[key]


def _nn_bruteforce(p, q, chunk):
    p64, q64 = p.astype(np.float64), q.astype(np.float64)
    out = np.empty(p64.shape[0])
    for i0 in range(0, p64.shape[0], chunk):
        diff = p64[i0:i0 + chunk, None, :] - q64[None, :, :]
        out[i0:i0 + chunk] = (diff * diff).sum(axis=2).min(axis=1)
    return out


def knn_points_stub(p1, p2, lengths1=None, lengths2=None, K=1):
    assert K == 1 and p1.shape[0] == p2.shape[0]
    d = np.stack([nn_bruteforce(a, b) for a, b in zip(p1.numpy(), p2.numpy())])
    return namedtuple("KNN", "dists idx knn")(torch.from_numpy(d.astype(np.float32))[..., None], None, None)


def load_reference_function():
    stubs = {"pytorch3d": {}, "pytorch3d.ops": {"knn_points": knn_points_stub, "sample_points_from_meshes": None},
             "pytorch3d.structures": {"Meshes": None}, "pytorch3d.io": {"load_obj": None}, "jsonlines": {},
             "tqdm": {"tqdm": None}, "tqdm.contrib": {}, "tqdm.contrib.concurrent": {"process_map": None}}
    for name, attrs in stubs.items():
        mod = types.ModuleType(name)
        mod.__dict__.update(attrs)
        sys.modules[name] = mod
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        d = os.path.join(tmp, "data", "text2shape-data", "shapenet", "preprocessed", "exp_data")
        os.makedirs(d)
        with open(os.path.join(d, "val_map.json"), "w") as f:
            f.write("[]")
        os.chdir(tmp)
        try:
            spec = importlib.util.spec_from_file_location("reference_calculate_f1", os.path.join(mg.REF, "calculate_f1.py"))
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
        finally:
            os.chdir(cwd)
    return mod._compute_sampling_metrics


def main():
    ref_fn = load_reference_function()
    out, tags = {}, []
    for tag, kind, S_pred, S_gt, seed0 in CASES:
        for seed in range(seed0, seed0 + TRIES):
            pred, gt = sr.make_pair(kind, S_pred, S_gt, seed)
            d2p, _ = sr.nn_exact(pred, gt)
            d2g, _ = sr.nn_exact(gt, pred)
            cp = [sr.threshold_counts(d2p, t) for t in sr.THRESHOLDS]
            cg = [sr.threshold_counts(d2g, t) for t in sr.THRESHOLDS]
            worst = max(a.undecidable + b.undecidable for a, b in zip(cp, cg))
            if worst <= sr.MAX_UNDECIDABLE:
                break
            print(f"{tag}: seed {seed} rejected, {worst} undecidable points at one threshold")
        else:
            raise SystemExit(f"{tag}: no seed in {seed0}..{seed0 + TRIES - 1} has at most {sr.MAX_UNDECIDABLE} undecidable points per threshold")
        # the kd-tree restatement against the exhaustive search the reference function is given
        bp, bg = nn_bruteforce(pred, gt), nn_bruteforce(gt, pred)
        assert np.allclose(bp, d2p, rtol=1e-14, atol=0) and np.allclose(bg, d2g, rtol=1e-14, atol=0), tag
        tp, tg = torch.from_numpy(pred)[None], torch.from_numpy(gt)[None]
        ref_f1 = np.array([float(ref_fn(tp, tg, thresholds=[t])[0]) for t in sr.THRESHOLDS], dtype=np.float32)
        # where the count is pinned, the restatement's fp32 expression must reproduce the reference bit for bit
        for k, t in enumerate(sr.THRESHOLDS):
            if cp[k].undecidable == 0 and cg[k].undecidable == 0:
                mine = sr.f1_fp32(cp[k].below, S_pred, cg[k].below, S_gt)[2]
                assert mine.tobytes() == ref_f1[k].tobytes(), (tag, t, mine, ref_f1[k])
        rows_p = np.linspace(0, S_pred - 1, min(SAMPLE, S_pred)).astype(np.int64)
        rows_g = np.linspace(0, S_gt - 1, min(SAMPLE, S_gt)).astype(np.int64)
        rec = {"kind": np.array(kind), "S_pred": np.int64(S_pred), "S_gt": np.int64(S_gt), "seed": np.int64(seed),
               "sha256": np.array(sr.sha256(pred, gt)), "ref_f1": ref_f1,
               "below_pred": np.array([c.below for c in cp], dtype=np.int64), "undecidable_pred": np.array([c.undecidable for c in cp], dtype=np.int64),
               "below_gt": np.array([c.below for c in cg], dtype=np.int64), "undecidable_gt": np.array([c.undecidable for c in cg], dtype=np.int64),
               "chamfer64": np.float64(d2p.mean() + d2g.mean()),
               "rows_pred": rows_p, "d2_pred": d2p[rows_p], "rows_gt": rows_g, "d2_gt": d2g[rows_g]}
        print(f"{tag}: seed {seed} F1 {ref_f1.tolist()} undecidable {[a.undecidable + b.undecidable for a, b in zip(cp, cg)]} "
              f"chamfer {float(rec['chamfer64']):.6g}")
        out.update({f"{tag}/{k}": v for k, v in rec.items()})
        tags.append(tag)
    out["cases"] = np.array(tags)
    out["thresholds"] = np.array(sr.THRESHOLDS, dtype=np.float64)
    path = os.path.join(mg.GOLD, "shape_f1.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
