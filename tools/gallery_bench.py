#!/usr/bin/env python
"""tri_retrieval_topk against tri_retrieval_gallery at the chair/table val shape (7,424 captions x 1,486 shapes x 512), alternating in one
process under device events, and tri_retrieval_gallery alone against a 40,000-shape gallery (past the old kernel's limit):
python tools/gallery_bench.py [--rounds 5] [--reps 10].  Prints one line per measurement (profiles/r20/NOTES_gallery.md keeps them).
--s2t measures the other direction instead: 1,486 shapes ask 7,424 captions (tri_retrieval_classes, CSR built once outside the timed
window) against tri_retrieval_gallery on the same swapped operands without labels - the same dot products, no pass over the classes -
alternating, with the spread of each (profiles/r22/NOTES_s2t.md)."""
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


def stats(t):
    return f"min {min(t):.3f} median {sorted(t)[len(t) // 2]:.3f} max {max(t):.3f} spread {(max(t) - min(t)) / sorted(t)[len(t) // 2] * 100:.1f}%"


def s2t(a):
    """Shape -> text at the val split's size: every shape asks, a caption's class is the shape it was made from."""
    Nt, Ns, D = 7424, 1486, 512
    text, shape, pick = inputs(Nt, Ns, D)
    qc = torch.arange(Ns, dtype=torch.int32, device="cuda")
    off, rows, ncls = ops.class_csr(pick, Ns)
    base = lambda q, c, k: ops.retrieval_gallery(q, c, None, k)                              # noqa: E731
    new = lambda q, c, k: ops.retrieval_classes_csr(q, c, qc, off, rows, ncls, k)            # noqa: E731
    whole = lambda q, c, k: ops.retrieval_classes(q, c, qc, pick, k, ncls=Ns)                # noqa: E731  (with the CSR build)
    for fn in (base, new, whole):
        timed(fn, (shape, text), 3)
    tb, tn, tw = [], [], []
    for _ in range(a.rounds):                                       # alternating: all see the same neighbours on the machine
        for fn, t in ((base, tb), (new, tn), (whole, tw)):
            ms, out = timed(fn, (shape, text), a.reps)
            t.append(ms)
            if fn is base:
                o = out
            elif fn is new:
                n = out
    same = torch.equal(o[0], n[0]) and torch.equal(o[1].view(torch.int64), n[1].view(torch.int64))
    sizes = torch.bincount(pick.long(), minlength=Ns)
    print(f"s2t {Ns} shapes x {Nt} captions x {D}, k = 5, {a.rounds} alternating rounds of {a.reps} calls; top k bit-identical: {same}; "
          f"captions per shape 0..{int(sizes.max())}, first_hit -1 for {int((n[2] < 0).sum())} shapes")
    print(f"  tri_retrieval_gallery, no labels   ms/call {stats(tb)}")
    print(f"  tri_retrieval_classes              ms/call {stats(tn)}   (+{Nt} dot products of the class pass on {Ns * Nt})")
    print(f"  ops.retrieval_classes (CSR + call) ms/call {stats(tw)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--s2t", action="store_true", help="measure the shape -> text direction instead")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gallery_bench.py needs an MI355X"
    if a.s2t:
        return s2t(a)
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
