#!/usr/bin/env python
"""tri_retrieval_topk against tri_retrieval_gallery at the chair/table val shape (7,424 captions x 1,486 shapes x 512), alternating in one
process under device events, and tri_retrieval_gallery alone against a 40,000-shape gallery (past the old kernel's limit):
python tools/gallery_bench.py [--rounds 5] [--reps 10].  Prints one line per measurement (profiles/r20/NOTES_gallery.md keeps them)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tricolo_amd import ops  # noqa: E402


def inputs(Nq, Ns, D, seed=0):
    rng = np.random.default_rng(seed)
    shape = rng.standard_normal((Ns, D)).astype(np.float32)
    shape /= np.linalg.norm(shape, axis=1, keepdims=True)
    pick = rng.integers(0, Ns, Nq)
    text = shape[pick] + 0.05 * rng.standard_normal((Nq, D)).astype(np.float32)
    return [torch.from_numpy(a).cuda() for a in (text, shape, pick.astype(np.int32))]


def timed(fn, args, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        out = fn(*args, 5)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gallery_bench.py needs an MI355X"
    Nq, Ns, D = 7424, 1486, 512
    args = inputs(Nq, Ns, D)
    for fn in (ops.retrieval_topk, ops.retrieval_gallery):
        timed(fn, args, 3)
    old, new = [], []
    for _ in range(a.rounds):                                       # alternating: both see the same neighbours on the machine
        ms, o = timed(ops.retrieval_topk, args, a.reps)
        old.append(ms)
        ms, n = timed(ops.retrieval_gallery, args, a.reps)
        new.append(ms)
    same = torch.equal(o[0], n[0]) and torch.equal(o[1].view(torch.int64), n[1].view(torch.int64)) and torch.equal(o[2], n[2])
    qt = 8
    print(f"val shape {Nq} x {Ns} x {D}, k = 5, {a.rounds} alternating rounds of {a.reps} calls; outputs bit-identical: {same}")
    print(f"  tri_retrieval_topk     ms/call min {min(old):.3f} median {sorted(old)[len(old) // 2]:.3f} max {max(old):.3f}   "
          f"shape bytes from L2: {Nq * Ns * D * 4 / 1e9:.2f} GB")
    print(f"  tri_retrieval_gallery  ms/call min {min(new):.3f} median {sorted(new)[len(new) // 2]:.3f} max {max(new):.3f}   "
          f"shape bytes from L2: {Nq * Ns * D * 4 / qt / 1e9:.2f} GB (QT = {qt})")
    Ns2 = 40000
    big = inputs(Nq, Ns2, D, seed=1)
    timed(ops.retrieval_gallery, big, 1)
    t = [timed(ops.retrieval_gallery, big, 3)[0] for _ in range(a.rounds)]
    print(f"gallery {Nq} x {Ns2} x {D}, k = 5: tri_retrieval_gallery ms/call min {min(t):.3f} median {sorted(t)[len(t) // 2]:.3f} max {max(t):.3f}   "
          f"shape bytes from L2: {Nq * Ns2 * D * 4 / qt / 1e9:.2f} GB; float64 FMAs {Nq * Ns2 * D / 1e9:.1f} G")


if __name__ == "__main__":
    main()
