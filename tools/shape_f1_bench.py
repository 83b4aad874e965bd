"""Timing of the shape F1 path on the GPU (profiles/r8/NOTES_shape_f1.md): one direction of the nearest-neighbour kernel at
10,000 x 10,000 points for N = 1, 64, 512 pairs, compute_sampling_metrics end to end, and the chunked torch expression a user
would otherwise write, in the same process.  One JSON line per N.

    python tools/shape_f1_bench.py [--n 1 64 512] [--trace-only N]    (--trace-only: one warmed call for rocprofv3 --kernel-trace)
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tricolo_amd.evaluation import shape_f1 as sf      # noqa: E402

S = 10000
FLOOR_US_PER_DIRECTION = 1e8 * 7 / (256 * 4 * 16 * 2.4e9) * 1e6      # 7 fp32 VALU operations per pair, unpacked: 17.8 us per 10^8 pairs


def torch_nn(p, q, rows=2500):
    """The expression a user would write, chunked so that the [rows, S, 3] temporaries fit."""
    out = torch.empty(p.shape[:2], device=p.device)
    for n in range(p.shape[0]):
        for i0 in range(0, p.shape[1], rows):
            out[n, i0:i0 + rows] = ((p[n, i0:i0 + rows, None] - q[n, None]) ** 2).sum(-1).min(-1).values
    return out


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters                                                   # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1, 64, 512])
    ap.add_argument("--trace-only", type=int, default=0)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    if a.trace_only:
        p, q = (3.0 * torch.randn((a.trace_only, S, 3), device=dev, generator=gen) for _ in range(2))
        for _ in range(3):
            m = sf.compute_sampling_metrics(p, q, thresholds=(0.1,))
        torch.cuda.synchronize()
        print(json.dumps({"N": a.trace_only, "mean_f1": float(m["F1@0.100000"].mean())}))
        return
    for N in a.n:
        p, q = (3.0 * torch.randn((N, S, 3), device=dev, generator=gen) for _ in range(2))
        iters = max(3, min(200, 20000 // N))
        kernel = timed(lambda: sf.nn_dist2(p, q), iters)
        kernel_idx = timed(lambda: sf.nn_dist2(p, q, return_idx=True), iters)
        e2e = timed(lambda: sf.compute_sampling_metrics(p, q, thresholds=(0.1,)), iters)
        base = timed(lambda: torch_nn(p, q), 3 if N <= 64 else 1)
        same = bool(((sf.nn_dist2(p[:1], q[:1]) - torch_nn(p[:1], q[:1])).abs() <= 2.0 ** -21 * sf.nn_dist2(p[:1], q[:1])).all())
        print(json.dumps({"N": N, "S": S, "iters": iters, "nn_dist2_us": round(kernel, 1), "nn_dist2_idx_us": round(kernel_idx, 1),
                          "compute_sampling_metrics_us": round(e2e, 1), "torch_expression_us": round(base, 1),
                          "torch_over_kernel": round(base / kernel, 2), "floor_us": round(FLOOR_US_PER_DIRECTION * N, 1),
                          "floor_fraction": round(FLOOR_US_PER_DIRECTION * N / kernel, 3), "agrees_with_torch": same}), flush=True)


if __name__ == "__main__":
    main()
