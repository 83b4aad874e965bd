"""Coloured solid voxel grids from ShapeNet meshes: the voxel32 / voxel64 / voxel128 entries of a packed .npz made from
model_normalized.obj by csrc/voxelize.hip (ops.voxelize_meshes), for data that has no nrrd_256_filter_div_{V}_solid download.

The reference has no voxeliser - it reads Text2Shape's grids - so what is computed here is a definition of our own, spelled out at
the head of csrc/voxelize.hip: vertices snapped to 1/256 voxel of a per-mesh frame (origin, cell size), a voxel on the surface when
its closed box overlaps a face (exact integer test; touching counts), its colour the rounded mean of the 8-bit Kd of ALL
overlapping faces, and the "carve" fill: a non-surface voxel with a surface voxel on each of its six axis rays is interior and
takes the colour of the nearest of them.  NOBODY HAS COMPARED A GRID OF THIS VOXELISER WITH TEXT2SHAPE'S: not the occupancy
(Text2Shape voxelises at 256^3, filters and divides), not the orientation of the grid axes relative to the ShapeNetCore.v2 meshes
(here mesh x, y, z map to grid x, y, z), not the colour of interior voxels.

On GPU tensors ops.voxelize_meshes launches the HIP kernels; on CPU tensors the same call runs voxelize_meshes_cpu below, a torch
restatement of the kernel's arithmetic that gives the same bits.  It exists for checking and for machines without a GPU and is not
tuned.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from ..meshes import MeshBatch, clamp_index, face_kd, host_boxes

SNAP_MAX = float(2 ** 17)
CANDIDATES_PER_PASS = 1 << 19                       # (face, voxel) pairs the fallback expands at a time


# ------------------------------------------------------------------------------------------------ frames
def box_frames(boxes, V):
    """meshes.host_boxes' float64 [N, 3, 2] -> float32 [N, 4] = (origin x, y, z, cell size) per mesh, formed in float64: the grid
    cube is centred on the box centre, its edge L is the box's longest side (no margin), cell = fl32(L / V) and origin = centre -
    V cell / 2.  A mesh without vertices (a zero box) or of zero extent gets cell = 0 (an all-zero grid)."""
    out = np.zeros((len(boxes), 4), np.float64)
    for n, box in enumerate(boxes):
        lo, hi = box[:, 0], box[:, 1]
        cell = float(np.float32((hi - lo).max() / V))
        centre = 0.5 * (lo + hi)
        out[n, :3] = centre - V * cell / 2.0 if cell > 0.0 else centre
        out[n, 3] = cell
    return torch.from_numpy(out.astype(np.float32))


def default_frames(verts_list, V):
    """box_frames of the bounding boxes of all vertices of every mesh."""
    return box_frames(host_boxes(verts_list), V)


# ------------------------------------------------------------------------------------------------ the torch fallback
def snap_vertices(verts, frame):
    """verts fp32 [Vn, 3], frame fp32 [4] -> (ok bool [Vn], G int64 [Vn, 3]): inside the snap range on every axis; the position in
    1/256 voxel."""
    d = verts - frame[:3]
    s = (d.to(torch.float64) / frame[3].to(torch.float64)).to(torch.float32) * 256.0
    inside = s.abs() <= SNAP_MAX                                                      # False for NaN
    G = torch.where(inside, torch.round(s), torch.zeros_like(s)).to(torch.int64)
    return inside.all(dim=1), G


def material_bytes(face_mat, kd):
    """q int64 [F, 3]: floor(255 clamp(Kd, 0, 1) + 0.5) of every face's material in fp32 (grey 0.4 without materials)."""
    col = face_kd(face_mat, kd)
    col = torch.where(col > 0, col, torch.zeros_like(col)).clamp(max=1.0)             # fminf(fmaxf(kd, 0), 1): NaN -> 0
    return torch.floor(255.0 * col + 0.5).to(torch.int64)


def face_setup(G, faces, V):
    """-> (Gf int64 [F, vertex, axis], normal int64 [F, 3], b0, b1 int64 [F, 3]): the snapped corners, (G1 - G0) x (G2 - G0) and
    the candidate voxel range per axis that test (a) leaves, clipped to the grid (empty where b0 > b1)."""
    Gf = G[faces]
    e1, e2 = Gf[:, 1] - Gf[:, 0], Gf[:, 2] - Gf[:, 0]
    nrm = torch.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                       e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    b0 = (((Gf.amin(1) + 255) >> 8) - 1).clamp(min=0)                                 # ceil(min / 256) - 1
    b1 = (Gf.amax(1) >> 8).clamp(max=V - 1)                                           # floor(max / 256)
    return Gf, nrm, b0, b1


def _voxelize_one(verts, faces, face_mat, kd, frame, V, fill):
    """(grid u8 [4, V, V, V], labels u8 [V, V, V]) of one mesh."""
    grid = torch.zeros((4, V, V, V), dtype=torch.uint8)
    labels = torch.zeros((V, V, V), dtype=torch.uint8)
    fr = [float(x) for x in frame.tolist()]
    if verts.shape[0] == 0 or faces.shape[0] == 0 or not all(math.isfinite(x) for x in fr) or not fr[3] > 0.0:
        return grid, labels
    okv, G = snap_vertices(verts, frame)
    Gf, nrm, b0, b1 = face_setup(G, faces, V)
    acc = torch.zeros((V * V * V, 4), dtype=torch.int64)                              # per voxel: faces that pass, their three byte sums
    keep = okv[faces].all(dim=1) & (nrm != 0).any(dim=1) & (b0 <= b1).all(dim=1)
    fidx = torch.nonzero(keep).reshape(-1)
    q = material_bytes(face_mat, kd)
    dims = (b1 - b0 + 1)[fidx]
    cnt = dims[:, 0] * dims[:, 1] * dims[:, 2]
    ends = torch.cumsum(cnt, 0)
    start = 0
    while start < fidx.numel():                                                       # passes of about CANDIDATES_PER_PASS pairs
        base = int(ends[start - 1]) if start else 0
        stop = int(torch.searchsorted(ends, torch.tensor(base + CANDIDATES_PER_PASS), right=True))
        stop = max(stop, start + 1)
        sel, c, dm = fidx[start:stop], cnt[start:stop], dims[start:stop]
        rep = torch.repeat_interleave(torch.arange(sel.numel()), c)
        local = torch.arange(int(c.sum())) - torch.repeat_interleave(torch.cumsum(c, 0) - c, c)
        djk = (dm[:, 1] * dm[:, 2])[rep]
        di = torch.div(local, djk, rounding_mode="floor")
        rem = local - di * djk
        dj = torch.div(rem, dm[rep, 2], rounding_mode="floor")
        dk = rem - dj * dm[rep, 2]
        f = sel[rep]
        ijk = [b0[f, 0] + di, b0[f, 1] + dj, b0[f, 2] + dk]
        u = [[Gf[f, k, a] - (256 * ijk[a] + 128) for a in range(3)] for k in range(3)]           # u_k = G_k - C, one vector per component
        n = [nrm[f, a] for a in range(3)]
        hit = ((n[0] * u[0][0] + n[1] * u[0][1]) + n[2] * u[0][2]).abs() <= 128 * ((n[0].abs() + n[1].abs()) + n[2].abs())   # test (b)
        for j in range(3):                                                            # test (c): a = e_i x f_j
            fj = [u[(j + 1) % 3][a] - u[j][a] for a in range(3)]
            for i in range(3):
                i1, i2 = (i + 1) % 3, (i + 2) % 3
                a1, a2 = -fj[i2], fj[i1]
                p = [a1 * u[k][i1] + a2 * u[k][i2] for k in range(3)]
                r = 128 * (a1.abs() + a2.abs())
                hit &= (torch.minimum(torch.minimum(p[0], p[1]), p[2]) <= r) & (torch.maximum(torch.maximum(p[0], p[1]), p[2]) >= -r)
        f, vox = f[hit], ((ijk[0] * V + ijk[1]) * V + ijk[2])[hit]
        acc.index_add_(0, vox, torch.cat([torch.ones((f.numel(), 1), dtype=torch.int64), q[f]], 1))
        start = stop
    count = acc[:, 0].view(V, V, V)
    surface = count > 0
    safe = torch.where(surface, count, torch.ones_like(count))
    rgb = [torch.div(2 * acc[:, 1 + k].view(V, V, V) + count, 2 * safe, rounding_mode="floor") for k in range(3)]   # 0 off the surface
    labels[surface] = 1
    src = torch.where(surface, torch.arange(V * V * V).view(V, V, V), torch.full((V, V, V), -1, dtype=torch.int64))
    if fill:
        idx = torch.arange(V)
        best = torch.full((V, V, V), V, dtype=torch.int64)
        hit_at = torch.full((V, V, V), -1, dtype=torch.int64)
        closed = ~surface
        stride = (V * V, V, 1)
        for axis in range(3):                                                         # rays in the order -x, +x, -y, +y, -z, +z
            shape = [1, 1, 1]
            shape[axis] = V
            pos = idx.view(shape).expand(V, V, V)
            below = torch.cummax(torch.where(surface, pos, torch.full_like(pos, -1)), dim=axis)[0]           # last surface index <= p
            above = V - 1 - torch.cummax(torch.where(surface, V - 1 - pos, torch.full_like(pos, -1)).flip(axis), dim=axis)[0].flip(axis)
            for found, where, dist in ((below >= 0, below, pos - below), (above <= V - 1, above, above - pos)):
                closed &= found
                nearer = found & (dist < best)                                        # strictly: an earlier ray keeps a tie
                best = torch.where(nearer, dist, best)
                flat = torch.arange(V * V * V).view(V, V, V) + (where - pos) * stride[axis]
                hit_at = torch.where(nearer, flat, hit_at)
        interior = closed & ~surface
        labels[interior] = 2
        src = torch.where(interior, hit_at, src)
    solid = src >= 0
    pick = src.clamp(min=0).reshape(-1)
    for k in range(3):
        grid[k] = torch.where(solid, rgb[k].reshape(-1)[pick].view(V, V, V), torch.zeros_like(count)).to(torch.uint8)
    grid[3] = solid.to(torch.uint8) * 255
    return grid, labels


def voxelize_meshes_cpu(verts, faces, vert_off, face_off, face_mat, mat_kd, mat_off, frame, V, fill=1, return_labels=False):
    """ops.voxelize_meshes on CPU tensors: one mesh after the other, the kernel's arithmetic in torch."""
    voff, foff, moff = vert_off.tolist(), face_off.tolist(), mat_off.tolist()
    N = len(voff) - 1
    grid = torch.zeros((N, 4, V, V, V), dtype=torch.uint8)
    labels = torch.zeros((N, V, V, V), dtype=torch.uint8)
    for n in range(N):
        v = verts[voff[n]:voff[n + 1]]
        f = faces[foff[n]:foff[n + 1]]
        if v.shape[0] == 0 or f.shape[0] == 0:
            continue
        grid[n], labels[n] = _voxelize_one(v, clamp_index(f, v.shape[0]), face_mat[foff[n]:foff[n + 1]], mat_kd[moff[n]:moff[n + 1]], frame[n], V, fill)
    return (grid, labels) if return_labels else grid


# ------------------------------------------------------------------------------------------------ the convenient calls
def voxelize_batch(batch, voxel_size, fill="carve", return_labels=False):
    """Coloured voxel grids of every mesh of a meshes.MeshBatch packed with materials -> uint8 [N, 4, V, V, V] on the batch's device,
    indexed [channel, x, y, z] as data.nrrd.read_nrrd returns the downloaded grids; with return_labels also uint8 [N, V, V, V]
    (0 exterior, 1 surface, 2 interior).  Frames every mesh by box_frames - the grid cube spans the longest side of the bounding
    box, centred, without margin - and calls ops.voxelize_meshes.

    What is defined (head of csrc/voxelize.hip): a voxel is on the surface when its closed box overlaps a face whose vertices were
    snapped to 1/256 voxel - touching counts, so a face in a boundary plane sets both layers; alpha is 255 there.  fill="carve"
    also fills every non-surface voxel that has a surface voxel on each of its six axis rays with the colour of the nearest of them
    (ties in the order -x, +x, -y, +y, -z, +z): carving fills ANY cavity no axis ray can see out of - the inside of a closed shell,
    but also a pocket that is open only diagonally - and it leaves open whatever one ray can escape from; it is no flood fill.
    fill="surface" keeps the shell alone.  In a voxel's colour every overlapping face weighs the same, whatever its area or how
    little of it lies in the voxel.  Textures (map_Kd) are ignored: a textured material contributes its Kd.  No grid has been
    compared with Text2Shape's (occupancy, axis orientation, interior colours)."""
    from .. import ops
    V = int(voxel_size)
    return ops.voxelize_meshes(*batch.tensors, box_frames(batch.boxes, V).to(batch.verts.device), V, fill, return_labels)


def voxelize_meshes(verts_list, faces_list, face_mat_list, kd_list, voxel_size, fill="carve", device=None, return_labels=False):
    """voxelize_batch of the lists, packed (meshes.MeshBatch.pack) on `device` (where verts_list[0] lives when None)."""
    return voxelize_batch(MeshBatch.pack(verts_list, faces_list, face_mat_list, kd_list, device), voxel_size, fill, return_labels)
