"""Timing of the multi-view renderer on the GPU (DESIGN.md "Multi-view rendering"): ops.render_views for a batch of 8 meshes in 12
views at 224 x 224 - the procedural mesh of tests/raster_reference.py (a sphere on a table of boxes) at about 20 k and about 200 k
faces - HIP events, warmed; milliseconds per model.  One JSON line per size.

    python tools/raster_bench.py [--rings 100 317] [--batch 8] [--trace-only RINGS]
    (--trace-only: three warmed calls for rocprofv3 --kernel-trace --stats, which gives the queue kernel's share of the time)
"""
import argparse
import json
import os
import sys

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
    ap.add_argument("--trace-only", type=int, default=None, metavar="RINGS")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    for rings in ([a.trace_only] if a.trace_only else a.rings):
        faces, args = batch(rings, a.batch, dev)
        for _ in range(3):
            img = ops.render_views(*args)
        torch.cuda.synchronize()
        if a.trace_only:
            print(json.dumps({"faces_per_mesh": faces, "batch": a.batch, "covered": float((img != 255).any(dim=2).float().mean())}))
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            ops.render_views(*args)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / a.iters
        print(json.dumps({"faces_per_mesh": faces, "batch": a.batch, "views": VIEWS, "size": SIZE, "iters": a.iters, "ms_per_call": round(ms, 3),
                          "ms_per_model": round(ms / a.batch, 3)}), flush=True)


if __name__ == "__main__":
    main()
