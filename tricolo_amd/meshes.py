"""The packed batch of triangle meshes that the sampler, the renderer and the voxeliser share (csrc/mesh_batch.h lays it out): reading
OBJ files, validating and packing lists of meshes on the host, the float64 bounding boxes the cameras and voxel frames come from, and
the three conventions of the kernels that the torch restatements in evaluation/mesh.py, data/render.py and data/voxelize.py have in
common - the unsigned clamp of a bad index, the diffuse colour of a face, the fp32 cross product."""
from __future__ import annotations

import re
from dataclasses import dataclass

import numpy as np
import torch


# ------------------------------------------------------------------------------------------------ OBJ
def load_obj(path):
    """-> (verts float32 [V, 3], faces int64 [F, 3]), what pytorch3d's load_obj(path, load_textures=False) gives calculate_f1.py as
    verts and faces.verts_idx.  `v x y z` lines (further values - vertex colours - ignored); `f` lines with tokens i, i/j, i/j/k, i//k:
    1-based, negative = counted back from the vertices read so far, polygons split as a fan (0, k, k + 1).  Every other line is
    ignored; CRLF is tolerated.  An index outside the file's vertices raises ValueError naming the line."""
    with open(path, "rb") as f:
        lines = [ln.strip() for ln in f.read().replace(b"\r", b"").split(b"\n")]
    head = [ln[:2] for ln in lines]
    is_v = np.fromiter((h == b"v " or h == b"v\t" for h in head), dtype=bool, count=len(lines))
    is_f = np.fromiter((h == b"f " or h == b"f\t" for h in head), dtype=bool, count=len(lines))
    v_lines, f_lines = np.flatnonzero(is_v), np.flatnonzero(is_f)
    vtoks = [lines[i].split()[1:4] for i in v_lines]
    for i, t in zip(v_lines, vtoks):
        if len(t) != 3:
            raise ValueError(f"{path}: line {i + 1}: a vertex needs three coordinates")
    verts = np.array(vtoks, dtype="S").astype(np.float64).astype(np.float32).reshape(-1, 3)
    V = verts.shape[0]
    if f_lines.size == 0:
        return torch.from_numpy(verts), torch.zeros((0, 3), dtype=torch.int64)
    ftoks = [lines[i].split()[1:] for i in f_lines]
    counts = np.fromiter((len(t) for t in ftoks), dtype=np.int64, count=len(ftoks))
    if (counts < 3).any():
        raise ValueError(f"{path}: line {f_lines[np.argmax(counts < 3)] + 1}: a face needs at least three vertices")
    body = re.sub(rb"/\S*", b"", b" ".join(b" ".join(t) for t in ftoks))            # i/j/k -> i
    raw = np.array(body.split(), dtype="S").astype(np.int64)
    tok_line = np.repeat(np.arange(len(ftoks)), counts)
    seen = np.cumsum(is_v)[f_lines][tok_line]                                       # vertices read before the token's line
    idx = np.where(raw > 0, raw - 1, np.where(raw < 0, seen + raw, -1))
    bad = (idx < 0) | (idx >= V)
    if bad.any():
        k = int(np.argmax(bad))
        raise ValueError(f"{path}: line {f_lines[tok_line[k]] + 1}: face index {raw[k]} is outside the file's {V} vertices")
    start = np.cumsum(counts) - counts                                               # the fan: (0, k, k + 1) for k = 1 .. count - 2
    ntri = counts - 2
    tri_start = np.repeat(start, ntri)
    k = np.arange(int(ntri.sum())) - np.repeat(np.cumsum(ntri) - ntri, ntri) + 1
    faces = np.stack([idx[tri_start], idx[tri_start + k], idx[tri_start + k + 1]], axis=1)
    return torch.from_numpy(verts), torch.from_numpy(np.ascontiguousarray(faces, dtype=np.int64))


# ------------------------------------------------------------------------------------------------ packing and validation
def pack_meshes(verts_list, faces_list, device=None):
    """Validate (dtypes, shapes, index ranges - on the host, from the min / max of the faces, before anything is launched) and pack:
    -> (verts fp32 [sumV, 3], faces int32 [sumF, 3] local indices, vert_off int64 [N + 1], face_off int64 [N + 1], max_faces)."""
    if len(verts_list) != len(faces_list):
        raise ValueError(f"{len(verts_list)} vertex arrays but {len(faces_list)} face arrays")
    if not verts_list:
        raise ValueError("an empty batch of meshes")
    if device is None:
        device = verts_list[0].device
    device = torch.device(device)
    voff, foff = [0], [0]
    for n, (v, f) in enumerate(zip(verts_list, faces_list)):
        if not torch.is_tensor(v) or v.dtype != torch.float32 or v.dim() != 2 or v.shape[1] != 3:
            raise ValueError(f"mesh {n}: verts must be a float32 tensor of shape [V, 3]")
        if not torch.is_tensor(f) or f.dtype not in (torch.int64, torch.int32) or f.dim() != 2 or f.shape[1] != 3:
            raise ValueError(f"mesh {n}: faces must be an int64 (or int32) tensor of shape [F, 3]")
        if v.shape[0] >= 2 ** 31 or f.shape[0] >= 2 ** 31:
            raise ValueError(f"mesh {n}: 2^31 or more vertices or faces")
        if f.shape[0]:
            lo, hi = int(f.min()), int(f.max())
            if lo < 0 or hi >= v.shape[0]:
                raise ValueError(f"mesh {n}: face indices span {lo} .. {hi} but the mesh has {v.shape[0]} vertices")
        voff.append(voff[-1] + v.shape[0])
        foff.append(foff[-1] + f.shape[0])
    verts = torch.cat([v.to(device) for v in verts_list]).contiguous()
    faces = torch.cat([f.to(device=device, dtype=torch.int32) for f in faces_list]).contiguous()
    return (verts, faces, torch.tensor(voff, dtype=torch.int64, device=device), torch.tensor(foff, dtype=torch.int64, device=device),
            max(b - a for a, b in zip(foff, foff[1:])))


def pack_materials(face_mat_list, kd_list, device=None):
    """-> (face_mat int32 [sumF], mat_kd fp32 [sumM, 3], mat_off int64 [N + 1]); validated on the host."""
    moff = [0]
    for n, (fm, kd) in enumerate(zip(face_mat_list, kd_list)):
        if kd.dim() != 2 or kd.shape[1] != 3 or kd.shape[0] < 1 or kd.dtype != torch.float32:
            raise ValueError(f"mesh {n}: Kd must be a float32 tensor of shape [M >= 1, 3]")
        if fm.numel() and (int(fm.min()) < 0 or int(fm.max()) >= kd.shape[0]):
            raise ValueError(f"mesh {n}: material indices span {int(fm.min())} .. {int(fm.max())} but the mesh has {kd.shape[0]} materials")
        moff.append(moff[-1] + kd.shape[0])
    device = device or "cpu"
    return (torch.cat([fm.to(device=device, dtype=torch.int32).reshape(-1) for fm in face_mat_list]).contiguous(),
            torch.cat([kd.to(device) for kd in kd_list]).contiguous(), torch.tensor(moff, dtype=torch.int64, device=device))


def host_boxes(verts_list):
    """float64 [N, 3, 2]: per-axis (min, max) over all vertices of every mesh (tensors or arrays), zeros for a mesh without vertices.
    Minimum and maximum are exact, so whatever is derived from a box has the bits it would have from the vertices themselves."""
    out = np.zeros((len(verts_list), 3, 2), np.float64)
    for n, verts in enumerate(verts_list):
        v = verts.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(verts) else np.asarray(verts, dtype=np.float64)
        if v.shape[0]:
            out[n, :, 0], out[n, :, 1] = v.min(0), v.max(0)
    return out


@dataclass
class MeshBatch:
    """A packed batch on one device; the three material tensors are None for a batch packed without materials."""
    verts: torch.Tensor
    faces: torch.Tensor
    vert_off: torch.Tensor
    face_off: torch.Tensor
    face_mat: torch.Tensor | None
    mat_kd: torch.Tensor | None
    mat_off: torch.Tensor | None
    max_faces: int                                  # the largest face count of a mesh (sizes ops.mesh_face_cdf's grid)
    boxes: np.ndarray                               # host_boxes of the input lists

    @classmethod
    def pack(cls, verts_list, faces_list, face_mat_list=None, kd_list=None, device=None):
        """pack_meshes, then pack_materials where face_mat_list and kd_list are given; device=None: where verts_list[0] lives."""
        verts, faces, voff, foff, max_faces = pack_meshes(verts_list, faces_list, device)
        mats = (None, None, None)
        if face_mat_list is not None:
            if len(face_mat_list) != len(faces_list) or any(fm.shape[0] != f.shape[0] for fm, f in zip(face_mat_list, faces_list)):
                raise ValueError("every mesh needs one material index per face")
            mats = pack_materials(face_mat_list, kd_list, verts.device)
        return cls(verts, faces, voff, foff, *mats, max_faces, host_boxes(verts_list))

    @property
    def tensors(self):                              # the first seven arguments of ops.render_views and ops.voxelize_meshes, in their order
        return self.verts, self.faces, self.vert_off, self.face_off, self.face_mat, self.mat_kd, self.mat_off


# ------------------------------------------------------------------------------------------------ shared by the torch restatements
def clamp_index(idx, count):
    """int64: the kernels' unsigned clamp of a vertex or material index - a negative or too large one becomes count - 1."""
    idx = idx.to(torch.int64)
    return torch.where(idx < 0, torch.full_like(idx, count - 1), idx.clamp(max=count - 1))


def face_kd(face_mat, kd):
    """fp32 [F, 3]: the diffuse colour of every face's (clamped) material, grey 0.4 for a mesh without materials."""
    if kd.shape[0] > 0:
        return kd[clamp_index(face_mat, kd.shape[0])]
    return torch.full((face_mat.shape[0], 3), 0.4, dtype=torch.float32)


def cross(a, b, c):
    """The components of (b - a) x (c - a) for points fp32 [F, 3], every operation rounded on its own, in the kernels' order."""
    u, w = b - a, c - a
    return u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
