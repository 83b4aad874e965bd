"""Timing of the multi-view renderer on the GPU (DESIGN.md "Multi-view rendering"): ops.render_views for a batch of 8 meshes in 12
views at 224 x 224 - the procedural mesh of tests/raster_reference.py (a sphere on a table of boxes) at about 20 k and about 200 k
faces - HIP events, warmed; milliseconds per call and per model, every window reported.  --samples 1 4 times the one-sample and the
four-sample call alternately, window by window, in one process.  One JSON line per size.

    python tools/raster_bench.py [--rings 100 317] [--batch 8] [--iters 20] [--windows 1] [--samples 1 4] [--trace-only RINGS]
    (--trace-only: three warmed calls for rocprofv3 --kernel-trace --stats, which gives the queue kernel's share of the time)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import raster_reference as rr                      # noqa: E402
from tricolo_amd import ops                                  # noqa: E402
from tricolo_amd.data import render as R                     # noqa: E402
from tricolo_amd.meshes import MeshBatch                     # noqa: E402

VIEWS, SIZE = 12, 224


def batch(rings, n, dev):
    pv, pf, pm, pk = rr.procedural_mesh(rings)
    packed = MeshBatch.pack([pv] * n, [pf] * n, [pm] * n, [pk] * n, dev)
    return pf.shape[0], (*packed.tensors, R.pack_cameras(R.box_centers(packed.boxes), VIEWS, dev), SIZE, SIZE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rings", type=int, nargs="+", default=[100, 317])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--samples", type=int, nargs="+", choices=(1, 4), default=[1], help="coverage samples per pixel; several: they alternate "
                    "window by window in one process")
    ap.add_argument("--windows", type=int, default=1)
    ap.add_argument("--trace-only", type=int, default=None, metavar="RINGS")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    for rings in ([a.trace_only] if a.trace_only else a.rings):
        faces, args = batch(rings, a.batch, dev)
        img = {}
        for s in a.samples:
            for _ in range(3):
                img[s] = ops.render_views(*args, samples=s)
        torch.cuda.synchronize()
        if a.trace_only:
            print(json.dumps({"faces_per_mesh": faces, "batch": a.batch, "covered": {s: float((i != 255).any(dim=2).float().mean()) for s, i in img.items()}}))
            return
        ms = {s: [] for s in a.samples}
        for _ in range(a.windows):
            for s in a.samples:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    ops.render_views(*args, samples=s)
                e1.record()
                torch.cuda.synchronize()
                ms[s].append(round(e0.elapsed_time(e1) / a.iters, 4))
        med = {s: float(np.median(v)) for s, v in ms.items()}
        print(json.dumps({"faces_per_mesh": faces, "batch": a.batch, "views": VIEWS, "size": SIZE, "iters": a.iters, "windows": a.windows,
                          "ms_per_call": ms, "median_ms_per_call": med, "median_ms_per_model": {s: round(m / a.batch, 4) for s, m in med.items()},
                          "pixels_changed_by_four_samples": float((img[1] != img[4]).any(dim=2).float().mean()) if len(img) == 2 else None}),
              flush=True)


if __name__ == "__main__":
    main()
