"""Per-face diffuse colours of a Wavefront OBJ: the `usemtl` groups of the file and the `Kd` of the `mtllib` files next to it,
as far as the renderer of data/render.py uses them.  load_obj_materials ignores map_Kd textures (and every other MTL statement);
load_obj_textured also reads the `vt` texture coordinates and decodes the map_Kd images for ops.render_views_textured;
load_obj_normals reads the `vn` normals of the face corners for the smooth shading of ops.render_views(..., normals=);
load_obj_pbr reads the `Ns` of the materials for the metallic-roughness BRDF of ops.render_views(..., brdf=)."""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from ..meshes import load_obj

DEFAULT_KD = (0.4, 0.4, 0.4)
DEFAULT_PBR = (0.2, 0.8)                            # (metallic, roughness) of material 0, the default grey
DEFAULT_NS = 1.0                                    # the specular exponent of a material without a usable Ns


def load_mtl(path):
    """-> {name: (r, g, b)} in file order; a material without a (complete) Kd line keeps the default grey."""
    out = {}
    name = None
    with open(path, "rb") as f:
        for ln in f.read().replace(b"\r", b"").split(b"\n"):
            tok = ln.split()
            if len(tok) >= 2 and tok[0] == b"newmtl":
                name = b" ".join(tok[1:]).decode(errors="replace")
                out.setdefault(name, DEFAULT_KD)
            elif len(tok) >= 4 and tok[0] == b"Kd" and name is not None:
                try:
                    out[name] = tuple(float(t) for t in tok[1:4])
                except ValueError:
                    pass
    return out


def load_obj_materials(path):
    """-> (verts float32 [V, 3], faces int64 [F, 3], face_material int32 [F], Kd float32 [M, 3], names): verts and faces are
    meshes.load_obj's; a k-gon under a `usemtl` yields k - 2 faces of that material.  Material 0 is a default grey
    (0.4, 0.4, 0.4) named None: it covers faces before any usemtl, names no mtllib file defines, and missing MTL files.  The other
    materials follow in the order the mtllib files define them.  CRLF is tolerated."""
    verts, faces = load_obj(path)
    with open(path, "rb") as f:
        lines = [ln.strip() for ln in f.read().replace(b"\r", b"").split(b"\n")]
    names, kd, index = [None], [DEFAULT_KD], {}
    here = os.path.dirname(os.path.abspath(path))
    for ln in lines:
        if ln[:7] in (b"mtllib ", b"mtllib\t"):
            for lib in ln.split()[1:]:
                lib_path = os.path.join(here, lib.decode(errors="replace"))
                if os.path.isfile(lib_path):
                    for name, colour in load_mtl(lib_path).items():
                        if name not in index:
                            index[name] = len(names)
                            names.append(name)
                            kd.append(colour)
    current, mats = 0, []
    for ln in lines:
        head = ln[:2]
        if head == b"f " or head == b"f\t":
            mats += [current] * (len(ln.split()) - 3)
        elif ln[:7] in (b"usemtl ", b"usemtl\t"):
            current = index.get(b" ".join(ln.split()[1:]).decode(errors="replace"), 0)
    face_material = torch.tensor(mats, dtype=torch.int32)
    if face_material.shape[0] != faces.shape[0]:
        raise ValueError(f"{path}: {face_material.shape[0]} material entries for {faces.shape[0]} faces")
    return verts, faces, face_material, torch.from_numpy(np.asarray(kd, dtype=np.float32).reshape(-1, 3)), names


def load_obj_normals(path):
    """-> face_vn float32 [F, 3, 3]: the `vn x y z` of every face corner in the order of meshes.load_obj's faces (the third index of
    tokens i/j/k and i//k; 1-based, negative = counted back from the vn lines read so far; polygons fan like their vertices,
    (0, k, k + 1)).  All nine values are NaN for a face with a corner that has no vn index (tokens i and i/j), an index outside the
    file's vn lines, a vn line that cannot be parsed, or a value that is not finite: such a face is shaded flat, or takes computed
    normals (MeshBatch.with_vertex_normals).  The normals are taken as they stand, not normalised.  CRLF is tolerated."""
    _, faces = load_obj(path)
    with open(path, "rb") as f:
        lines = [ln.strip() for ln in f.read().replace(b"\r", b"").split(b"\n")]
    vn, rows = [], []
    nan = (math.nan, math.nan, math.nan)
    for ln in lines:
        head = ln[:3]
        if head in (b"vn ", b"vn\t"):
            tok = ln.split()
            try:
                value = (float(tok[1]), float(tok[2]), float(tok[3]))
            except (IndexError, ValueError):
                value = nan
            vn.append(value if all(math.isfinite(x) for x in value) else nan)
        elif head[:2] in (b"f ", b"f\t"):
            corner = []
            for tok in ln.split()[1:]:
                part = tok.split(b"/")
                try:
                    j = int(part[2]) if len(part) >= 3 and part[2] else 0
                except ValueError:
                    j = 0
                j = j - 1 if j > 0 else len(vn) + j if j < 0 else -1
                corner.append(vn[j] if 0 <= j < len(vn) else nan)
            for k in range(1, len(corner) - 1):
                tri = (corner[0], corner[k], corner[k + 1])
                rows.append(tri if all(c[0] == c[0] for c in tri) else (nan, nan, nan))
    face_vn = torch.from_numpy(np.asarray(rows, dtype=np.float64).astype(np.float32).reshape(-1, 3, 3))
    face_vn[~torch.isfinite(face_vn).all(dim=2).all(dim=1)] = math.nan           # a value that overflows fp32 is not finite either
    if face_vn.shape[0] != faces.shape[0]:
        raise ValueError(f"{path}: {face_vn.shape[0]} normal rows for {faces.shape[0]} faces")
    return face_vn


def load_mtl_ns(path):
    """-> {name: Ns} in file order: the specular exponent of every material, DEFAULT_NS for one without a usable `Ns` line - absent,
    unparsable, negative or not finite.  As for Kd, the lines of a material's first `newmtl` and of its later ones both count, the last
    usable one wins."""
    out = {}
    name = None
    with open(path, "rb") as f:
        for ln in f.read().replace(b"\r", b"").split(b"\n"):
            tok = ln.split()
            if len(tok) >= 2 and tok[0] == b"newmtl":
                name = b" ".join(tok[1:]).decode(errors="replace")
                out.setdefault(name, DEFAULT_NS)
            elif len(tok) >= 2 and tok[0] == b"Ns" and name is not None:
                try:
                    ns = float(tok[1])
                except ValueError:
                    continue
                if math.isfinite(ns) and ns >= 0.0:
                    out[name] = ns
    return out


def ns_to_roughness(ns):
    """(2 / (Ns + 2)) ^ (1 / 4) in float64, as two square roots, rounded to fp32: the roughness a specular exponent stands for."""
    return float(np.float32(math.sqrt(math.sqrt(2.0 / (float(ns) + 2.0)))))


def load_obj_pbr(path, metallic=1.0):
    """-> pbr float32 [M, 2] = (metallic, roughness) of the materials of load_obj_materials(path), in its order: what
    MeshBatch.pack(..., pbr_list=) takes for the BRDF of ops.render_views(..., brdf=).  roughness = ns_to_roughness(Ns) with the Ns of
    the material's MTL definition (the first mtllib file that defines the name counts, as for Kd), Ns = 1 without a usable one;
    metallic is one number for all parsed materials.  Material 0, the default grey named None, is DEFAULT_PBR = (0.2, 0.8).  This is
    what pyrender is believed - from memory, checked by nobody - to make of a trimesh SimpleMaterial (data/render.py)."""
    names = load_obj_materials(path)[4]
    with open(path, "rb") as f:
        lines = [ln.strip() for ln in f.read().replace(b"\r", b"").split(b"\n")]
    here = os.path.dirname(os.path.abspath(path))
    ns = {}
    for ln in lines:
        if ln[:7] in (b"mtllib ", b"mtllib\t"):
            for lib in ln.split()[1:]:
                lib_path = os.path.join(here, lib.decode(errors="replace"))
                if os.path.isfile(lib_path):
                    for name, value in load_mtl_ns(lib_path).items():
                        ns.setdefault(name, value)
    rows = [DEFAULT_PBR] + [(float(metallic), ns_to_roughness(ns.get(name, DEFAULT_NS))) for name in names[1:]]
    return torch.from_numpy(np.asarray(rows, dtype=np.float32).reshape(-1, 2))


def load_mtl_textures(path):
    """-> {name: map_Kd file name or None} in file order.  The file name is the LAST token of the map_Kd line (options such as
    `-s 1 1 1` are skipped), with backslashes turned into slashes."""
    out = {}
    name = None
    with open(path, "rb") as f:
        for ln in f.read().replace(b"\r", b"").split(b"\n"):
            tok = ln.split()
            if len(tok) >= 2 and tok[0] == b"newmtl":
                name = b" ".join(tok[1:]).decode(errors="replace")
                out.setdefault(name, None)
            elif len(tok) >= 2 and tok[0] == b"map_Kd" and name is not None:
                out[name] = tok[-1].decode(errors="replace").replace("\\", "/")
    return out


def load_texture(path, max_texture_size=256):
    """An image file -> uint8 [H, W, 4] RGBA (alpha 255), row 0 the top row: decoded with PIL, converted to RGB (from greyscale,
    palette or RGBA), and reduced by the smallest integer box factor (PIL's Image.reduce) that brings both sides to at most
    max_texture_size - the renderer has no mip-maps, this bounds its minification.  Raises what PIL raises."""
    from PIL import Image
    with Image.open(path) as img:
        img = img.convert("RGB")
        factor = int(math.ceil(max(img.size) / float(max_texture_size)))
        if factor > 1:
            img = img.reduce(factor)
        rgb = np.asarray(img, dtype=np.uint8)
    return np.concatenate([rgb, np.full(rgb.shape[:2] + (1,), 255, np.uint8)], axis=2)


def load_obj_textured(path, max_texture_size=256):
    """load_obj_materials plus textures -> (verts, faces, face_material, Kd, names, face_uv, mat_tex, textures, warnings):
    face_uv float32 [F, 3, 2], the `vt u v [w]` of every face corner in the order of `faces` (tokens i/j and i/j/k; 1-based, negative
    = counted back from the vt lines read so far; polygons fan like their vertices) - all six values NaN for a face with a corner
    that has no vt (tokens i and i//k, or an index outside the file's vt lines); mat_tex int32 [M], per material an index into
    textures or -1; textures, a list of uint8 [H, W, 4] arrays (load_texture) of the map_Kd files, looked up relative to the MTL file
    that names them, one entry per distinct file; warnings, a list of strings, one per map_Kd that could not be loaded (a missing
    or unreadable file, no PIL) - such a material stays untextured, nothing is raised."""
    verts, faces, face_material, kd, names = load_obj_materials(path)
    with open(path, "rb") as f:
        lines = [ln.strip() for ln in f.read().replace(b"\r", b"").split(b"\n")]
    here = os.path.dirname(os.path.abspath(path))
    mat_tex = np.full((len(names),), -1, np.int32)
    textures, loaded, warnings, seen = [], {}, [], set()
    for ln in lines:
        if ln[:7] not in (b"mtllib ", b"mtllib\t"):
            continue
        for lib in ln.split()[1:]:
            lib_path = os.path.join(here, lib.decode(errors="replace"))
            if not os.path.isfile(lib_path):
                continue
            for name, file_name in load_mtl_textures(lib_path).items():
                if name in seen or name not in names:
                    continue
                seen.add(name)                                                           # the first definition counts, as for Kd
                if file_name is None:
                    continue
                tex_path = os.path.normpath(os.path.join(os.path.dirname(lib_path), file_name))
                if tex_path not in loaded:
                    try:
                        textures.append(load_texture(tex_path, max_texture_size))
                        loaded[tex_path] = len(textures) - 1
                    except Exception as e:                                               # never raises: the material stays untextured
                        loaded[tex_path] = -1
                        warnings.append(f"{tex_path}: {type(e).__name__}: {e}")
                mat_tex[names.index(name)] = loaded[tex_path]
    vt, uv = [], []
    nan = (math.nan, math.nan)
    for ln in lines:
        head = ln[:3]
        if head in (b"vt ", b"vt\t"):
            tok = ln.split()
            try:
                vt.append((float(tok[1]), float(tok[2])))
            except (IndexError, ValueError):
                vt.append(nan)
        elif head[:2] in (b"f ", b"f\t"):
            corner = []
            for tok in ln.split()[1:]:
                part = tok.split(b"/")
                try:
                    j = int(part[1]) if len(part) >= 2 and part[1] else 0
                except ValueError:
                    j = 0
                j = j - 1 if j > 0 else len(vt) + j if j < 0 else -1
                corner.append(vt[j] if 0 <= j < len(vt) else nan)
            for k in range(1, len(corner) - 1):
                tri = (corner[0], corner[k], corner[k + 1])
                uv.append(tri if all(c[0] == c[0] and c[1] == c[1] for c in tri) else (nan, nan, nan))
    face_uv = torch.from_numpy(np.asarray(uv, dtype=np.float64).astype(np.float32).reshape(-1, 3, 2))
    if face_uv.shape[0] != faces.shape[0]:
        raise ValueError(f"{path}: {face_uv.shape[0]} texture coordinate rows for {faces.shape[0]} faces")
    return verts, faces, face_material, kd, names, face_uv, torch.from_numpy(mat_tex), textures, warnings
