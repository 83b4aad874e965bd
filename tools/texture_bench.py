"""Timing of the textured renderer on the GPU (DESIGN.md "Textures"): ops.render_views_textured against ops.render_views on the scene
of tools/raster_bench.py - a batch of 8 procedural meshes (a sphere on a table of boxes, about 20 k and about 200 k faces) in 12
views at 224 x 224 - and ops.mesh_face_colours on the same batch.  Two of the three materials carry a 256 x 256 random-noise texture
(the parser's largest size; noise is the worst case for the texel loads), the third has none, and every face has random UVs in
[-2, 3]: textured and untextured pixels meet in the same waves.  HIP events, warmed; the two renderers alternate window by window in
one process, and every window is reported, so the spread is on the page.  One JSON line per size.  --mip adds the mip-mapped call
(ops.render_views_textured(..., mips=), with --samples 1 4 in both sample counts) and ops.texture_mips, the pyramid build for the
batch's 256 x 256 textures, to the alternation.  --normals adds the smooth-shaded calls (normals= of both renderers, the batch's
computed vertex normals, in every sample count asked for) and ops.mesh_vertex_normals itself.  --brdf adds the metallic-roughness
partner (brdf= of both renderers; metallic 1 with two roughnesses, and the default (0.2, 0.8)) of every render call in the alternation.

    python tools/texture_bench.py [--rings 100 317] [--batch 8] [--iters 20] [--windows 5] [--samples 1 4] [--mip] [--normals] [--brdf] [--trace-only RINGS]
    (--trace-only: three warmed calls of each for rocprofv3 --kernel-trace --stats, which gives the resolve kernels' own times)
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

VIEWS, SIZE, TEXTURE = 12, 224, 256


def batch(rings, n, dev):
    pv, pf, pm, pk = rr.procedural_mesh(rings)
    g = np.random.default_rng(1)
    uv = torch.from_numpy(g.uniform(-2.0, 3.0, (pf.shape[0], 3, 2)).astype(np.float32))
    texs = [np.concatenate([g.integers(0, 256, (TEXTURE, TEXTURE, 3), dtype=np.uint8), np.full((TEXTURE, TEXTURE, 1), 255, np.uint8)], 2) for _ in range(2)]
    mt = torch.tensor([-1, 0, 1], dtype=torch.int32)
    packed = MeshBatch.pack([pv] * n, [pf] * n, [pm] * n, [pk] * n, dev, face_uv_list=[uv] * n, mat_tex_list=[mt] * n, textures_list=[texs] * n)
    return pf.shape[0], packed, (R.pack_cameras(R.box_centers(packed.boxes), VIEWS, dev), SIZE, SIZE)


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rings", type=int, nargs="+", default=[100, 317])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--samples", type=int, nargs="+", choices=(1, 4), default=[1], help="coverage samples per pixel of the two renderers; with "
                    "1 4 the four-sample calls (render_views_4, render_views_textured_4) join the alternation")
    ap.add_argument("--mip", action="store_true", help="time the mip-mapped call (render_views_mip, render_views_mip_4) and the pyramid build "
                    "(texture_mips) beside the others")
    ap.add_argument("--normals", action="store_true", help="time the smooth-shaded calls (render_views_smooth, render_views_textured_smooth and their "
                    "_4 partners) and the vertex normals (mesh_vertex_normals) beside the others")
    ap.add_argument("--brdf", action="store_true", help="time the metallic-roughness partner (its name with _brdf) of every render call beside the others")
    ap.add_argument("--trace-only", type=int, default=None, metavar="RINGS")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    for rings in ([a.trace_only] if a.trace_only else a.rings):
        faces, packed, tail = batch(rings, a.batch, dev)
        calls = {"render_views": lambda: ops.render_views(*packed.tensors, *tail),
                 "render_views_textured": lambda: ops.render_views_textured(*packed.tensors, *packed.texture_tensors, *tail),
                 "mesh_face_colours": lambda: ops.mesh_face_colours(packed)}
        if 4 in a.samples:
            calls["render_views_4"] = lambda: ops.render_views(*packed.tensors, *tail, samples=4)
            calls["render_views_textured_4"] = lambda: ops.render_views_textured(*packed.tensors, *packed.texture_tensors, *tail, samples=4)
        if a.mip:
            mips = ops.texture_mips(*packed.texture_tensors[2:])
            calls["texture_mips"] = lambda: ops.texture_mips(*packed.texture_tensors[2:])
            calls["render_views_mip"] = lambda: ops.render_views_textured(*packed.tensors, *packed.texture_tensors, *tail, mips=mips)
            if 4 in a.samples:
                calls["render_views_mip_4"] = lambda: ops.render_views_textured(*packed.tensors, *packed.texture_tensors, *tail, samples=4, mips=mips)
        if a.normals:
            geometry = (packed.verts, packed.faces, packed.vert_off, packed.face_off)
            vn = ops.mesh_vertex_normals(*geometry)
            calls["mesh_vertex_normals"] = lambda: ops.mesh_vertex_normals(*geometry)
            for smp in a.samples:
                tag = "_4" if smp == 4 else ""
                calls["render_views_smooth" + tag] = lambda smp=smp: ops.render_views(*packed.tensors, *tail, samples=smp, normals=vn)
                calls["render_views_textured_smooth" + tag] = lambda smp=smp: ops.render_views_textured(*packed.tensors, *packed.texture_tensors, *tail,
                                                                                                         samples=smp, normals=vn)
        if a.brdf:
            pbr = torch.tensor([[0.2, 0.8], [1.0, 0.76], [1.0, 0.5]] * a.batch, device=dev)
            renders = {"render_views": (False, None, None), "render_views_textured": (True, None, None)}
            if a.mip:
                renders["render_views_mip"] = (True, mips, None)
            if a.normals:
                renders["render_views_smooth"], renders["render_views_textured_smooth"] = (False, None, vn), (True, None, vn)
            for name, (textured, pyramid, normals) in renders.items():
                for smp in a.samples:
                    if textured:
                        fn = lambda smp=smp, pyramid=pyramid, normals=normals: ops.render_views_textured(    # noqa: E731
                            *packed.tensors, *packed.texture_tensors, *tail, samples=smp, mips=pyramid, normals=normals, brdf=pbr)
                    else:
                        fn = lambda smp=smp, normals=normals: ops.render_views(*packed.tensors, *tail, samples=smp, normals=normals, brdf=pbr)  # noqa: E731
                    calls[name + ("_4" if smp == 4 else "") + "_brdf"] = fn
        if 1 not in a.samples:
            calls.pop("render_views_mip", None)
            del calls["render_views"], calls["render_views_textured"]
        for fn in calls.values():
            for _ in range(3):
                out = fn()
            out = out[0] if isinstance(out, tuple) else out
        torch.cuda.synchronize()
        if a.trace_only:
            print(json.dumps({"faces_per_mesh": faces, "batch": a.batch, "finite": bool(torch.isfinite(out).all())}))
            return
        plain, tex = ops.render_views(*packed.tensors, *tail), ops.render_views_textured(*packed.tensors, *packed.texture_tensors, *tail)
        ms = {k: [] for k in calls}
        for _ in range(a.windows):
            for k, fn in calls.items():
                ms[k].append(round(window(fn, a.iters), 4))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        ratios = {"textured_over_plain": ("render_views_textured", "render_views"), "textured_4_over_plain_4": ("render_views_textured_4", "render_views_4"),
                  "textured_4_over_textured": ("render_views_textured_4", "render_views_textured"),
                  "mip_over_textured": ("render_views_mip", "render_views_textured"), "mip_4_over_textured_4": ("render_views_mip_4", "render_views_textured_4"),
                  "smooth_over_plain": ("render_views_smooth", "render_views"), "smooth_4_over_plain_4": ("render_views_smooth_4", "render_views_4"),
                  "textured_smooth_over_textured": ("render_views_textured_smooth", "render_views_textured"),
                  "textured_smooth_4_over_textured_4": ("render_views_textured_smooth_4", "render_views_textured_4")}
        print(json.dumps({"faces_per_mesh": faces, "batch": a.batch, "views": VIEWS, "size": SIZE, "texture": TEXTURE, "iters": a.iters, "ms_per_call": ms,
                          "median_ms_per_call": med, **{k: round(med[x] / med[y], 4) for k, (x, y) in ratios.items() if x in med and y in med},
                          "pixels_changed_by_textures": float((plain != tex).any(dim=2).float().mean()),
                          **({"pixels_changed_by_mips": float((calls["render_views_mip"]() != tex).any(dim=2).float().mean())}
                             if "render_views_mip" in calls else {}),
                          **({"pixels_changed_by_normals": float((calls["render_views_smooth"]() != plain).any(dim=2).float().mean())}
                             if "render_views_smooth" in calls else {}),
                          **{k + "_over_lambert": round(med[k] / med[k[:-5]], 4) for k in med if k.endswith("_brdf") and k[:-5] in med},
                          **({"pixels_changed_by_brdf": float((calls["render_views_brdf"]() != plain).any(dim=2).float().mean()),
                              "drawn_pixels_changed_by_brdf": float(((calls["render_views_brdf"]() != plain).any(dim=2) & (plain != 255).any(dim=2)).sum()
                                                                    / (plain != 255).any(dim=2).sum())}
                             if "render_views_brdf" in calls else {})}), flush=True)


if __name__ == "__main__":
    main()
