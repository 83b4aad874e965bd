"""Time the two losses side by side on one GPU: the all-pairs launches alone (forward + backward, M = 3, D = 512, B = 32 and 64)
and the trimodal default-configuration training step (bench.py's config 4, its default precision) with loss.name = NTXentLoss and
TripletLoss.  Everything is a replayed HIP graph after warm-up; a figure is the median of three windows.

    python tools/triplet_timing.py [--reps 200] [--steps 20] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench                                                     # noqa: E402
from tricolo_amd import config as tcfg, ops, parallel            # noqa: E402
from tricolo_amd.data import synthetic as syn                    # noqa: E402
from tricolo_amd.loss.nt_xent import NTXentLoss                  # noqa: E402
from tricolo_amd.loss.triplet import TripletLoss                 # noqa: E402
from tricolo_amd.model.tricolo_net import TriCoLoNet             # noqa: E402

DEV = "cuda"


def windows(graph, reps):
    out = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            graph.replay()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / reps)
    return sorted(out)


def clustered(B, D, seed):
    g = torch.Generator().manual_seed(seed)
    c = torch.randn(B, 3, generator=g) @ (torch.randn(3, D, generator=g) / D ** 0.5)
    z = [c + 0.3 * torch.randn(B, D, generator=g) / D ** 0.5 for _ in range(3)]
    return [torch.nn.functional.normalize(x).to(DEV).requires_grad_() for x in z]


def time_loss(loss_fn, B, reps):
    zs = clustered(B, 512, B)
    one = ops.one(DEV)

    def run():
        _, total = loss_fn.all_pairs(zs)
        return torch.autograd.grad(total, zs, grad_outputs=one)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            run()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = run()                                             # noqa: F841
    for _ in range(50):
        graph.replay()
    return windows(graph, reps)


def time_step(loss_name, steps):
    a = bench.parse_args([])
    ops.set_default_precision(a.precision)
    cfg = tcfg.compose(overrides=["data=synthetic", f"model.text_encoder={a.text}", f"model.image_encoder={a.image}",
                                  f"model.voxel_encoder={a.voxel}", f"data.voxel_size={a.voxel_size}", f"data.num_views={a.num_views}",
                                  f"data.image_size={a.image_size}", f"loss.name={loss_name}", "experiment_name=timing"])
    torch.manual_seed(cfg.train_seed)
    net = TriCoLoNet(cfg).to(DEV)
    opt = net.configure_optimizers()
    opt.prepare()
    batch = bench.make_batches(a, 0, DEV, 1)[0]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            parallel.dp_training_step(net, batch, opt)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        losses = parallel.dp_training_step(net, batch, opt)
    for _ in range(a.preroll):
        graph.replay()
    w = windows(graph, steps)
    info = {"loss": float(losses["train_loss/total_loss"].item()), "skipped_steps": opt.skipped_steps()}
    counts = getattr(net.loss_fn, "last_counts", None)
    if counts is not None:
        info["counts"] = counts.tolist()
    return w, info, a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0)}
    for B in (32, 64):
        for name, fn in (("ntxent_multi", NTXentLoss(0.1, 0.25)), ("triplet_multi", TripletLoss(0.025))):
            w = time_loss(fn, B, args.reps)
            res[f"{name}_fwd_bwd_B{B}_us"] = {"median": w[1] * 1e6, "min": w[0] * 1e6, "max": w[2] * 1e6}
            print(f"{name} fwd+bwd B={B} D=512 M=3: median {w[1] * 1e6:.2f} us (min {w[0] * 1e6:.2f}, max {w[2] * 1e6:.2f})", flush=True)
    for loss_name in ("NTXentLoss", "TripletLoss", "NTXentLoss", "TripletLoss"):             # alternating, two runs each
        w, info, a = time_step(loss_name, args.steps)
        res.setdefault(f"step_{loss_name}_ms", []).append({"median": w[1] * 1e3, "min": w[0] * 1e3, "max": w[2] * 1e3, **info})
        print(f"step config {a.config} {a.precision} B={a.per_gpu_batch} {loss_name}: median {w[1] * 1e3:.4f} ms "
              f"(min {w[0] * 1e3:.4f}, max {w[2] * 1e3:.4f}) {info}", flush=True)
        torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
