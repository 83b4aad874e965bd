"""Timing of the mesh surface sampler on the GPU (profiles/r9/NOTES_mesh_sample.md): the CDF launches (tri_mesh_face_cdf) and the
sampling launch (tri_mesh_sample_points) for N = 1, 64, 512 meshes x 10,000 samples at 2,000 and 200,000 faces per mesh, HIP events,
warmed, beside the plain torch expression a user would otherwise write on the same GPU in the same process (areas -> cumsum in
float64 -> searchsorted -> gather -> barycentric, one mesh after the other as its CDF is per mesh).  One JSON line per batch.

    python tools/mesh_sample_bench.py [--n 1 64 512] [--faces 2000 200000] [--trace-only N F]
    (--trace-only: three warmed calls of sample_points_from_meshes for rocprofv3 --kernel-trace --stats)
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tricolo_amd import ops                                  # noqa: E402
from tricolo_amd.evaluation import mesh as M                 # noqa: E402

S = 10000


def grid_mesh(faces, gen, dev):
    """A bumpy height field of about `faces` triangles (uneven areas)."""
    side = max(2, int(round((faces / 2) ** 0.5)) + 1)
    x, y = torch.meshgrid(torch.linspace(0, 1, side, device=dev), torch.linspace(0, 1, side, device=dev), indexing="ij")
    z = 0.2 * torch.rand((side, side), device=dev, generator=gen)
    v = torch.stack([x * x, y, z], -1).reshape(-1, 3).contiguous()
    i, j = torch.meshgrid(torch.arange(side - 1, device=dev), torch.arange(side - 1, device=dev), indexing="ij")
    a, b, c, d = i * side + j, (i + 1) * side + j, (i + 1) * side + j + 1, i * side + j + 1
    f = torch.cat([torch.stack([a, b, c], -1).reshape(-1, 3), torch.stack([a, c, d], -1).reshape(-1, 3)])
    return v, f[torch.randperm(f.shape[0], device=dev, generator=gen)].contiguous()


def torch_expression(verts_list, faces_list, gen):
    out = []
    for v, f in zip(verts_list, faces_list):
        a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
        cdf = torch.cumsum(0.5 * torch.linalg.cross(b - a, c - a).norm(dim=1).double(), 0)
        u = torch.rand((3, S), device=v.device, generator=gen)
        pick = torch.searchsorted(cdf, u[0].double() * cdf[-1], right=True).clamp(max=f.shape[0] - 1)
        r = u[1].sqrt()
        out.append((1 - r)[:, None] * a[pick] + (r * (1 - u[2]))[:, None] * b[pick] + (r * u[2])[:, None] * c[pick])
    return torch.stack(out)


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
    ap.add_argument("--faces", type=int, nargs="+", default=[2000, 200000])
    ap.add_argument("--trace-only", type=int, nargs=2, default=None, metavar=("N", "FACES"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    if a.trace_only:
        N, F = a.trace_only
        v, f = grid_mesh(F, gen, dev)
        for _ in range(3):
            p = M.sample_points_from_meshes([v] * N, [f] * N, S, 0, "gt-10")
        torch.cuda.synchronize()
        print(json.dumps({"N": N, "faces": f.shape[0], "mean": float(p.mean())}))
        return
    for F in a.faces:
        base_mesh = [grid_mesh(F, gen, dev) for _ in range(4)]                                 # four distinct meshes, repeated
        for N in a.n:
            vl, fl = [base_mesh[k % 4][0] for k in range(N)], [base_mesh[k % 4][1] for k in range(N)]
            verts, faces, voff, foff, mf = M.pack_meshes(vl, fl, dev)
            scale = M.resolve_scale("gt-10", verts, voff)
            cdf, total = ops.mesh_face_cdf(verts, faces, voff, foff, scale, mf)
            iters = max(5, min(200, 20000 // N))
            t_bbox = timed(lambda: ops.mesh_bbox(verts, voff), iters)
            t_cdf = timed(lambda: ops.mesh_face_cdf(verts, faces, voff, foff, scale, mf), iters)
            t_smp = timed(lambda: ops.mesh_sample_points(verts, faces, voff, foff, cdf, total, S, 0, scale), iters)
            t_idx = timed(lambda: ops.mesh_sample_points(verts, faces, voff, foff, cdf, total, S, 0, scale, True), iters)
            t_e2e = timed(lambda: M.sample_points_from_meshes(vl, fl, S, 0, "gt-10"), max(3, iters // 10))
            t_torch = timed(lambda: torch_expression(vl, fl, gen), 3 if N <= 64 else 1)
            # bytes the algorithm has to move: faces + their vertices once, the CDF out; samples: three vertices in, a point out
            cdf_bytes = faces.shape[0] * (12 + 36 + 8)
            print(json.dumps({"N": N, "faces_per_mesh": fl[0].shape[0], "S": S, "iters": iters, "bbox_us": round(t_bbox, 1),
                              "face_cdf_us": round(t_cdf, 1), "sample_us": round(t_smp, 1), "sample_idx_us": round(t_idx, 1),
                              "cdf_plus_sample_us": round(t_cdf + t_smp, 1), "sample_points_from_meshes_us": round(t_e2e, 1),
                              "torch_expression_us": round(t_torch, 1), "torch_over_kernels": round(t_torch / (t_cdf + t_smp), 2),
                              "face_cdf_GBps": round(cdf_bytes / t_cdf / 1e3, 1), "samples_per_us": round(N * S / t_smp, 1)}), flush=True)


if __name__ == "__main__":
    main()
