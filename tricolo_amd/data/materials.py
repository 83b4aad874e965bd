"""Per-face diffuse colours of a Wavefront OBJ: the `usemtl` groups of the file and the `Kd` of the `mtllib` files next to it,
as far as the renderer of data/render.py uses them (map_Kd textures and every other MTL statement are ignored)."""
from __future__ import annotations

import os

import numpy as np
import torch

from ..meshes import load_obj

DEFAULT_KD = (0.4, 0.4, 0.4)


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
