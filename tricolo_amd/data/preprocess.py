"""Preprocessing of the Text2Shape data on the GPU: what the reference's data/preprocess_all_data.py:109-155 does for the three
splits, without pyrender, trimesh, pynrrd, Hydra or Lightning.

    python -m tricolo_amd.data.preprocess data=text2shape_chair_table data.dataset_root_path=/path/to/data \\
        [--batch-meshes 8] [--jpeg-roundtrip] [--device cuda] [--voxels nrrd|mesh|auto] [--textures off|on|mip] [--antialias off|4x] \\
        [--shading flat|smooth] [--brdf lambert|gltf] [--metallic 1.0]

It writes the files tricolo_amd.data.dataset.PackedDataset (and the reference's own loader) read: `{split}_map.json` at
cfg.data.{split}_lang_data_path - the list of {model_id, category, caption, tokens} from processed_captions_{split}.p and
shapenet.json; for Text2ShapeC13 the existing map file is read instead - and `<exp_data_root_path>/<category>/<model_id>.npz`
with voxel32 / voxel64 / voxel128 (uint8 [4, V, V, V]) and images (uint8 [cfg.data.num_views, 3, 224, 224]).  The images are rendered from
`<dirname(dataset_path)>/ShapeNetCore.v2/<category>/<model_id>/models/model_normalized.obj` by ops.render_views (csrc/raster.hip), a
batch of meshes per call.  data/render.py says what that renderer restates of the reference's pyrender scene, what it deliberately
does differently (Lambert shading and flat normals unless asked otherwise, no culling, textures only on request) and that no pixel has
been compared with pyrender's.

--textures on (the default is off: a textured material renders with its bare Kd) reads the `vt` coordinates and the map_Kd images
of the models (data/materials.py load_obj_textured; textures above 256 texels on a side are reduced) and renders through
ops.render_views_textured: Kd x texel, repeat wrap, bilinear, no mip-maps.  Voxels made from the meshes (--voxels mesh | auto) then
take one colour per face, ops.mesh_face_colours: Kd times the mean of four texture samples of the face.  The summary names the
models with at least one loaded texture and the map_Kd files that could not be loaded (such a material keeps its Kd).

--textures mip is --textures on with mip-mapped texture lookups in the renderings: ops.texture_mips builds the pyramid of every
texture once per packed batch (exact integer box means of the texture itself), and ops.render_views_textured(..., mips=) blends the
two levels around the footprint of a pixel - with --antialias 4x, of a sample - in the texture, so that a face much smaller on
screen than its texture shows the texture's mean colour, not four texels picked at random.  A magnified texture renders exactly as
under --textures on.  The voxel colours are those of --textures on (ops.mesh_face_colours does not read the pyramid).  The level
rule is a definition of our own (data/render.py, head of csrc/raster.hip): no pixel of it has been compared with pyrender's.

--antialias 4x (the default is off: visibility is decided at the pixel centre alone) renders with four coverage samples per pixel,
ops.render_views(..., samples=4): the 4x rotated grid, every sample covered, depth-tested and coloured by the one-sample rules, the
pixel their rounded integer mean.  It works with --textures on (each sample takes the texture at its own (u, v)) and with --device
cpu.  data/render.py says what it rests on - our unverified reading that pyrender's off-screen passes are 4x multisampled.

--shading smooth (the default is flat: a pixel is lit by the normal of its face) reads the `vn` normals of the models beside whatever
else is loaded (data/materials.py load_obj_normals), computes vertex normals for the faces that have none (ops.mesh_vertex_normals,
once per packed batch: area-weighted, by vertex index) and renders with normals=: the corner normals are interpolated across the
face, at the pixel centre or with --antialias 4x at every sample, turned toward the eye and lit as before.  It works with every
--textures and --antialias choice and with --device cpu, and leaves the voxels alone.  The summary then counts the faces that came
with vn and the faces that took computed normals.  It rests on our unverified readings, from memory, that pyrender shades trimesh
meshes smoothly by default and that trimesh keeps a file's vn; the area weighting (trimesh: angle weighting) and the turn toward
the eye at every position are our own (data/render.py).

--brdf gltf (the default is lambert: Kd (0.1 + 3/pi max(n . l, 0))) colours every pixel - with --antialias 4x, every sample - with
the glTF 2.0 metallic-roughness BRDF, ops.render_views(..., brdf=): the materials' roughness comes from their `Ns`
(data/materials.py load_obj_pbr: (2 / (Ns + 2))^(1/4), Ns = 1 without a usable one), their metallic factor is --metallic (default
1.0; only meaningful with gltf), the default grey material takes (0.2, 0.8).  It works with every --textures, --antialias and
--shading choice and with --device cpu, and leaves the voxels and the .npz layout alone.  It rests on our unverified readings, from
memory, of how pyrender converts a trimesh SimpleMaterial and of its fragment shader (data/render.py); the metallic factor is the
least certain part, hence --metallic.  No pixel has been compared with pyrender's.

--voxels says where the grids come from.  nrrd (the default): Text2Shape's nrrd_256_filter_div_{V}_solid/<id>/<id>.nrrd downloads
(data/nrrd.py), which exist for chairs and tables only.  mesh: ops.voxelize_meshes (csrc/voxelize.hip) voxelises the meshes already
loaded for the renderer, one call per size for the whole batch, so that Text2ShapeC13 or one's own meshes get their grids too.
auto: the NRRD files where all three exist for a model, the mesh otherwise.  The voxeliser is a definition of our own - surface
voxels by an exact box / triangle overlap, the mean Kd of all overlapping faces, interiors carved along the six axis rays;
data/voxelize.py spells it out - and NO GRID OF IT HAS BEEN COMPARED WITH TEXT2SHAPE'S: not the occupancy, not the orientation of
the grid axes relative to the v2 meshes, not the colour of interior voxels.  The .npz layout is the same either way.

Every .npz is written under a temporary name and renamed; a file that exists is skipped, so an interrupted run resumes.
--jpeg-roundtrip passes every view through an in-memory JPEG at PIL's default quality, as the reference's img.save("<i>.jpg")
followed by Image.open does.
"""
from __future__ import annotations

import argparse
import io
import json
import os
import pickle
import sys

import numpy as np
import torch

from .. import config as tcfg
from ..meshes import MeshBatch
from . import render, voxelize
from .materials import load_obj_materials, load_obj_normals, load_obj_pbr, load_obj_textured
from .nrrd import read_nrrd

VOXEL_SIZES = (32, 64, 128)
SPLITS = ("train", "val", "test")
VOXEL_SOURCES = ("nrrd", "mesh", "auto")
TEXTURE_MODES = ("off", "on", "mip")
ANTIALIAS_MODES = {"off": 1, "4x": 4}                # --antialias -> samples per pixel
SHADING_MODES = render.SHADING_MODES                 # ("flat", "smooth")
BRDF_MODES = render.BRDF_MODES                       # ("lambert", "gltf")


def create_model_id_caption_mapping(caption_file_path, id_word_file_path, output_json_path, ignored_models):
    """preprocess_all_data.py:16-41: -> ((category, model_id), ...) in order of first occurrence; writes the list of
    {model_id, category, caption, tokens} to output_json_path.  Words are joined up to the first pad id 0, newlines removed."""
    with open(caption_file_path, "rb") as f:
        caption_tuples = pickle.load(f)["caption_tuples"]
    with open(id_word_file_path, "r") as f:
        idx_to_word = json.load(f)["idx_to_word"]
    ignored = set(ignored_models or ())
    samples, seen = [], {}
    for inds, category, nrrd_name in caption_tuples:
        inds = np.asarray(inds)
        text = []
        for ind in inds.tolist():
            if ind == 0:
                break
            text.append(idx_to_word[str(ind)])
        model_id = nrrd_name.split(".")[0]
        if f"{category}/{model_id}" in ignored:
            continue
        samples.append({"model_id": model_id, "category": category, "caption": " ".join(text).replace("\n", ""), "tokens": inds.tolist()})
        seen.setdefault((category, model_id), True)
    os.makedirs(os.path.dirname(os.path.abspath(output_json_path)), exist_ok=True)
    with open(output_json_path, "w") as f:
        json.dump(samples, f, indent=2)
    return tuple(seen)


def read_model_ids(map_json_path):
    """preprocess_all_data.py:130-137: the (category, model_id) pairs of an existing map file, in order of first occurrence."""
    with open(map_json_path, "r") as f:
        return tuple(dict.fromkeys((it["category"], it["model_id"]) for it in json.load(f)))


def jpeg_roundtrip(images):
    """uint8 [n, 3, H, W] -> the same views after PIL's JPEG encoder (default quality) and decoder."""
    from PIL import Image
    out = np.empty_like(images)
    for i, view in enumerate(images):
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(view.transpose(1, 2, 0))).save(buf, format="JPEG")
        buf.seek(0)
        out[i] = np.asarray(Image.open(buf).convert("RGB")).transpose(2, 0, 1)
    return out


def nrrd_path(data_root, mid, v):
    return os.path.join(data_root, f"nrrd_256_filter_div_{v}_solid", mid, f"{mid}.nrrd")


def pack_batch(meshes, device, textures=False, face_vn_list=None, pbr_list=None):
    """MeshBatch.pack of load_obj_materials' (or, with textures, load_obj_textured's) tuples; with textures the voxeliser's batch too.
    textures="mip": the packed batch carries the mip pyramid of its textures, built here, once per batch.  face_vn_list
    (load_obj_normals of the same files): the renderer's batch carries them, completed by computed vertex normals once per batch; the
    voxeliser's batch is what it is without them.  pbr_list (load_obj_pbr of the same files): the renderer's batch carries the
    materials' (metallic, roughness); the voxeliser does not read them."""
    from dataclasses import replace
    if not textures:
        packed = MeshBatch.pack(*zip(*(m[:4] for m in meshes)), device=device, face_vn_list=face_vn_list, pbr_list=pbr_list)
        solid = packed if face_vn_list is None else replace(packed, face_vn=None)
    else:
        from .. import ops
        packed = MeshBatch.pack(*zip(*(m[:4] for m in meshes)), device=device, face_uv_list=[m[5] for m in meshes],
                                mat_tex_list=[m[6] for m in meshes], textures_list=[m[7] for m in meshes], face_vn_list=face_vn_list,
                                pbr_list=pbr_list)
        solid = packed.with_face_colours(ops.mesh_face_colours(packed))
        if textures == "mip":
            packed = packed.with_texture_mips()
    if face_vn_list is not None:
        packed = packed.with_vertex_normals(fill="missing")
    return packed, solid


def pack_models(keys, obj_root, data_root, out_root, num_views, device, batch_meshes=8, roundtrip=False, log=print, voxels="nrrd",
                textures=False, texture_stats=None, samples=1, shading="flat", normal_stats=None, brdf="lambert", metallic=1.0):
    """Render and pack every (category, model_id) of `keys` that has no .npz yet -> (written, skipped).  voxels: where the grids
    come from - "nrrd" (the downloaded files), "mesh" (ops.voxelize_meshes) or "auto" (the files where all three exist).
    textures: read and render map_Kd textures, and colour mesh voxels from them ("mip": render them mip-mapped); texture_stats, a dict, then gains the number of
    "textured_models" (at least one texture loaded) and of "texture_failures" (map_Kd files that could not be loaded).
    samples: coverage samples per pixel, 1 or 4 (render.render_batch).  shading="smooth": read the `vn` normals, complete them with
    computed vertex normals and render smooth-shaded; normal_stats, a dict, then gains the number of "faces_with_vn" (rendered with
    the file's normals) and of "faces_with_computed_normals".  brdf="gltf": read the materials' Ns (load_obj_pbr, with `metallic` as
    their metallic factor) and render with the metallic-roughness BRDF."""
    if shading not in SHADING_MODES:
        raise ValueError(f"shading must be one of {SHADING_MODES}, got {shading!r}")
    if brdf not in BRDF_MODES:
        raise ValueError(f"brdf must be one of {BRDF_MODES}, got {brdf!r}")
    todo = [k for k in keys if not os.path.exists(os.path.join(out_root, k[0], f"{k[1]}.npz"))]
    load = load_obj_textured if textures else load_obj_materials
    for i in range(0, len(todo), batch_meshes):
        batch = todo[i:i + batch_meshes]
        meshes = [load(os.path.join(obj_root, cat, mid, "models", "model_normalized.obj")) for cat, mid in batch]
        if textures and texture_stats is not None:
            texture_stats["textured_models"] = texture_stats.get("textured_models", 0) + sum(1 for m in meshes if len(m[7]))
            texture_stats["texture_failures"] = texture_stats.get("texture_failures", 0) + sum(len(m[8]) for m in meshes)
        normals = None
        if shading == "smooth":
            normals = [load_obj_normals(os.path.join(obj_root, cat, mid, "models", "model_normalized.obj")) for cat, mid in batch]
        pbr = None
        if brdf == "gltf":
            pbr = [load_obj_pbr(os.path.join(obj_root, cat, mid, "models", "model_normalized.obj"), metallic) for cat, mid in batch]
        packed, solid = pack_batch(meshes, device, textures, normals, pbr)
        if normals is not None and normal_stats is not None:
            given = sum(int((~torch.isnan(vn[:, 0, 0])).sum()) for vn in normals)
            normal_stats["faces_with_vn"] = normal_stats.get("faces_with_vn", 0) + given
            normal_stats["faces_with_computed_normals"] = (normal_stats.get("faces_with_computed_normals", 0)
                                                           + int((~torch.isnan(packed.face_vn[:, 0, 0])).sum()) - given)
        images = render.render_batch(packed, num_views, render.IMAGE_SIZE, textures=textures, samples=samples, shading=shading,
                                     brdf=brdf).cpu().numpy()
        from_mesh = [k for k, (_, mid) in enumerate(batch) if voxels == "mesh" or
                     (voxels == "auto" and not all(os.path.exists(nrrd_path(data_root, mid, v)) for v in VOXEL_SIZES))]
        if 0 < len(from_mesh) < len(batch):                  # only some models lack their NRRD files: that subset, packed once for the three sizes
            solid = pack_batch([meshes[k] for k in from_mesh], device, bool(textures))[1]
        made = {f"voxel{v}": voxelize.voxelize_batch(solid, v, fill="carve").cpu().numpy() for v in VOXEL_SIZES} if from_mesh else {}
        for k, ((cat, mid), views) in enumerate(zip(batch, images)):
            if k in from_mesh:
                grids = {name: g[from_mesh.index(k)] for name, g in made.items()}
            else:
                grids = {f"voxel{v}": read_nrrd(nrrd_path(data_root, mid, v), v) for v in VOXEL_SIZES}
            os.makedirs(os.path.join(out_root, cat), exist_ok=True)
            path = os.path.join(out_root, cat, f"{mid}.npz")
            tmp = f"{path}.{os.getpid()}.tmp"
            with open(tmp, "wb") as f:
                np.savez_compressed(f, images=jpeg_roundtrip(views) if roundtrip else views, **grids)
            os.replace(tmp, path)
        log(f"  packed {min(i + batch_meshes, len(todo))} / {len(todo)}")
    return len(todo), len(keys) - len(todo)


def main(argv=None, log=print):
    """-> {split: {"models", "written", "skipped"}}, with --textures on | mip also "textured_models" and "texture_failures", with
    --shading smooth also "faces_with_vn" and "faces_with_computed_normals"."""
    ap = argparse.ArgumentParser(prog="python -m tricolo_amd.data.preprocess", description=__doc__.split("\n\n")[0])
    ap.add_argument("overrides", nargs="*", help="config overrides, e.g. data=text2shape_chair_table data.dataset_root_path=...")
    ap.add_argument("--batch-meshes", type=int, default=8, help="meshes rendered per call")
    ap.add_argument("--jpeg-roundtrip", action="store_true", help="pass every view through an in-memory JPEG, as the reference's .jpg files do")
    ap.add_argument("--device", default="cuda", help="cuda (csrc/raster.hip, csrc/voxelize.hip) or cpu (the untuned torch restatements)")
    ap.add_argument("--voxels", choices=VOXEL_SOURCES, default="nrrd", help="the grids: the nrrd_256_filter_div_{V}_solid downloads, voxelised "
                    "from the meshes, or auto (the downloads where all three sizes exist for a model)")
    ap.add_argument("--textures", choices=TEXTURE_MODES, default="off", help="on: render map_Kd textures (ops.render_views_textured) and colour "
                    "mesh voxels from them; mip: the same with mip-mapped lookups in the renderings (ops.texture_mips); off: a textured "
                    "material renders with its bare Kd")
    ap.add_argument("--antialias", choices=tuple(ANTIALIAS_MODES), default="off", help="4x: four coverage samples per pixel (the 4x rotated grid), "
                    "the pixel their rounded mean; off: visibility at the pixel centre alone")
    ap.add_argument("--shading", choices=SHADING_MODES, default="flat", help="smooth: interpolate the models' vn normals, and computed vertex "
                    "normals where a face has none (ops.mesh_vertex_normals), across every face; flat: the normal of the face")
    ap.add_argument("--brdf", choices=BRDF_MODES, default="lambert", help="gltf: the glTF metallic-roughness BRDF, roughness from the materials' "
                    "Ns (ops.render_views(..., brdf=)); lambert: Kd (0.1 + 3/pi max(n . l, 0))")
    ap.add_argument("--metallic", type=float, default=1.0, help="the metallic factor of every parsed material under --brdf gltf")
    args = ap.parse_args(sys.argv[1:] if argv is None else argv)
    if args.batch_meshes < 1:
        ap.error("--batch-meshes must be positive")
    cfg = tcfg.compose(overrides=args.overrides)
    data = cfg.data
    obj_root = os.path.join(os.path.dirname(data.dataset_path), "ShapeNetCore.v2")
    stats = {}
    for split in SPLITS:
        log(f"==> {split} split")
        map_path = getattr(data, f"{split}_lang_data_path")
        if data.dataset == "Text2ShapeChairTable":
            keys = create_model_id_caption_mapping(os.path.join(data.dataset_path, f"processed_captions_{split}.p"),
                                                   os.path.join(data.dataset_path, "shapenet.json"), map_path, data.ignored_models)
        else:
            keys = read_model_ids(map_path)
        tex = {"textured_models": 0, "texture_failures": 0} if args.textures != "off" else {}
        nrm = {"faces_with_vn": 0, "faces_with_computed_normals": 0} if args.shading == "smooth" else {}
        written, skipped = pack_models(keys, obj_root, data.dataset_path, data.exp_data_root_path, int(data.num_views), args.device,
                                       args.batch_meshes, args.jpeg_roundtrip, log, args.voxels, {"off": False, "on": True, "mip": "mip"}[args.textures], tex,
                                       ANTIALIAS_MODES[args.antialias], args.shading, nrm, args.brdf, args.metallic)
        stats[split] = {"models": len(keys), "written": written, "skipped": skipped, **tex, **nrm}
        log(f"  {len(keys)} models: {written} written, {skipped} already there")
        if tex:
            log(f"  {tex['textured_models']} of the written models have a texture, {tex['texture_failures']} map_Kd files could not be loaded")
        if nrm:
            log(f"  {nrm['faces_with_vn']} faces rendered with the normals of their file, {nrm['faces_with_computed_normals']} with computed ones")
    return stats


if __name__ == "__main__":
    main()
