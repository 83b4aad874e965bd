"""Timing of the bicubic antialiased u8 resize (csrc/resize.hip through ops.resize_bicubic_aa_u8) at the loader's shape: a chunk of
256 shapes x 6 views, u8 [1536, 3, 224, 224] -> 128 x 128, HIP events, warmed; effective GB/s of u8 read + written against the
6.3 TB/s HBM figure of SURVEY 8d; and the torch-CPU expression (the op's host path, what the reference's loader runs per shape) on
16 threads on a slice of the same input.  One JSON line.  Run it under a time limit.

    timeout -k 10 300 python tools/resize_bench.py [--shapes 256] [--views 6] [--iters 20] [--cpu-images 96]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tricolo_amd import ops                                  # noqa: E402

HBM_TBPS = 6.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=int, default=256)
    ap.add_argument("--views", type=int, default=6)
    ap.add_argument("--src", type=int, default=224)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cpu-images", type=int, default=96, help="images of the same input the torch-CPU expression is timed on")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    n = a.shapes * a.views
    gen = torch.Generator().manual_seed(0)
    x_host = torch.randint(0, 256, (n, 3, a.src, a.src), dtype=torch.uint8, generator=gen)
    x = x_host.to(dev)
    y = ops.resize_bicubic_aa_u8(x, a.size)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        y = ops.resize_bicubic_aa_u8(x, a.size)
    e1.record()
    torch.cuda.synchronize()
    gpu_ms = e0.elapsed_time(e1) / a.iters
    nbytes = x.numel() + y.numel()
    t0 = time.perf_counter()
    x.copy_(x_host)
    torch.cuda.synchronize()
    upload_ms = (time.perf_counter() - t0) * 1e3
    torch.set_num_threads(16)
    m = min(a.cpu_images, n)
    ops.resize_bicubic_aa_u8(x_host[:8], a.size)
    t0 = time.perf_counter()
    y_cpu = ops.resize_bicubic_aa_u8(x_host[:m], a.size)
    cpu_ms = (time.perf_counter() - t0) * 1e3 * n / m
    same = float((y[:m].cpu() == y_cpu).float().mean())
    print(json.dumps({"images": n, "src": a.src, "size": a.size, "iters": a.iters, "gpu_ms": round(gpu_ms, 3),
                      "gpu_images_per_s": round(n / gpu_ms * 1e3), "effective_GBps": round(nbytes / gpu_ms / 1e6, 1),
                      "fraction_of_hbm": round(nbytes / gpu_ms / 1e6 / (HBM_TBPS * 1e3), 3), "pageable_upload_ms": round(upload_ms, 1),
                      "torch_cpu_16_threads_ms": round(cpu_ms, 1), "cpu_images_timed": m, "cpu_over_gpu": round(cpu_ms / gpu_ms, 1),
                      "pixels_equal_to_cpu": round(same, 6)}), flush=True)


if __name__ == "__main__":
    main()
