"""An independent statement of the smooth shading of csrc/raster.hip (normals= of ops.render_views) and of the vertex normals of
csrc/mesh_normals.hip (ops.mesh_vertex_normals) for the tests: float64 numpy, one mesh and one view, in the manner of
tests/texture_reference.py.  Which face a pixel shows comes from tests/raster_reference.visibility (a float64 brute force, with its
`ambiguous` pixels); this file shades it its own way.  It shares with the code under test only the vertices' snapped integer screen
positions (tricolo_amd.data.render.snap_vertices), as raster_reference does.  Everything else is taken differently:
  * the screen barycentrics are E_k / 2A from the exact edge functions of the face in its ORIGINAL corner order (no swap), the depths
    1 / z come from a float64 camera transform, the perspective-correct weights are b_k / z_k normalised;
  * the corner normals are interpolated with those weights in float64; a face whose marker is NaN, and a pixel where the
    interpolated normal is not finite or has no length, takes the flat shade of texture_reference.shades;
  * the normal is turned toward the eye by the sign of n . (eye - vertex 0), then Lambert: 0.1 + 3 / pi max(n_y / |n|, 0);
  * colour = clamp(Kd shade, 0, 1), u8 = floor(255 colour + 1/2).
With affine=True the normals are interpolated with the screen barycentrics alone - WRONG on purpose, for the test that shows the
perspective division is visible.

Beyond raster_reference's own `ambiguous` pixels a pixel is ambiguous here when fp32 cannot decide what float64 decides:
  * the sign of side = n . e: |side| <= SIDE_REL |n| |e|.  The error of a three-term fp32 dot product is about 2.4e-7 of |n| |e|, the
    fp32 interpolation of n adds about 1e-6, so 1e-5 leaves an order of margin;
  * whether the normal has a length: |n| < LENGTH_REL of the largest corner normal of the face.
The scenes used must keep all of them below raster_reference.MAX_AMBIGUOUS (1 %) of the covered pixels.

vertex_normals is the float64 statement of the vertex normals: the plain sum of the float64 cross products of the faces at every
vertex index, normalised."""
import math

import numpy as np
import torch

from tests import raster_reference as rr
from tests import texture_reference as tr
from tricolo_amd.data import render as R

SIDE_REL = 1e-5
LENGTH_REL = 1e-3


def render(verts, faces, face_mat, kd, face_vn, cam, H, W, yfov=R.YFOV, znear=R.ZNEAR, affine=False):
    """One mesh, one view.  verts fp32 [V, 3], faces int64 [F, 3], face_mat int [F], kd fp32 [M, 3], face_vn fp32 [F, 3, 3] (torch
    tensors), cam fp32 [12] -> (image uint8 [3, H, W], face int64 [H, W], ambiguous bool [H, W], smooth bool [H, W]: the pixels that
    took an interpolated normal)."""
    face, ambiguous, covered = rr.visibility(verts, faces, cam, H, W, yfov, znear)
    okv, Xv, Yv, _ = R.snap_vertices(verts, cam, H, W, yfov, znear)
    X, Y = Xv.numpy().astype(np.float64), Yv.numpy().astype(np.float64)
    v, c, f = verts.numpy().astype(np.float64), cam.numpy().astype(np.float64), faces.numpy()
    inv_z = 1.0 / np.where(okv.numpy(), -((v - c[:3]) @ c[9:12]), 1.0)
    kd64, vn64 = kd.numpy().astype(np.float64), face_vn.numpy().astype(np.float64)
    fm = np.asarray(face_mat).astype(np.int64)
    flat = tr.shades(v, f, c[:3])
    image = np.full((3, H, W), 255, np.uint8)
    ambiguous, smooth = ambiguous.copy(), np.zeros((H, W), bool)
    py, px = np.nonzero(covered)
    fw = face[py, px]
    Px, Py = 256.0 * px + 128.0, 256.0 * py + 128.0
    fi = f[fw]
    bary = np.empty((fw.shape[0], 3))
    for k in range(3):
        a, b = (k + 1) % 3, (k + 2) % 3
        bary[:, k] = (X[fi[:, b]] - X[fi[:, a]]) * (Py - Y[fi[:, a]]) - (Y[fi[:, b]] - Y[fi[:, a]]) * (Px - X[fi[:, a]])
    bary /= bary.sum(1, keepdims=True)                                                  # the three edge functions add up to 2A
    wgt = bary if affine else bary * inv_z[fi]
    wgt = wgt / wgt.sum(1, keepdims=True)
    with np.errstate(invalid="ignore", over="ignore"):
        n = (wgt[:, :, None] * vn64[fw]).sum(1)                                         # NaN for a face without normals, or with an inf
        length = np.sqrt((n * n).sum(1))
        has = ~np.isnan(vn64[fw, 0, 0]) & np.isfinite(n).all(1) & (length > 0)
        e = c[:3] - v[fi[:, 0]]
        side = (n * e).sum(1)
        ny = np.where(side < 0, -n[:, 1], n[:, 1]) / np.where(has, length, 1.0)
        largest = np.sqrt((vn64[fw] ** 2).sum(2)).max(1)
        unsure = has & ((np.abs(side) <= SIDE_REL * length * np.sqrt((e * e).sum(1))) | (length < LENGTH_REL * largest))
    shade = np.where(has, 0.1 + 3.0 / math.pi * np.maximum(np.where(has, ny, 0.0), 0.0), flat[fw])
    colour = np.clip(kd64[fm[fw]] * shade[:, None], 0.0, 1.0)
    image[:, py, px] = np.floor(255.0 * colour + 0.5).astype(np.uint8).T
    ambiguous[py, px] |= unsure
    smooth[py, px] = has
    return image, face, ambiguous, smooth


def vertex_normals(verts, faces):
    """verts fp32 [V, 3], faces int64 [F, 3] of one mesh (torch tensors) -> (normal float64 [V, 3], the unit sum of the float64 cross
    products of the faces at every vertex, zeros where the sum has no length; total float64 [V, 3], that sum; largest float64 [V],
    the largest area - half the length of the cross product - among the faces at the vertex)."""
    v, f = verts.numpy().astype(np.float64), faces.numpy()
    cr = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    total, largest = np.zeros_like(v), np.zeros(v.shape[0])
    for j in range(3):
        np.add.at(total, f[:, j], cr)
        np.maximum.at(largest, f[:, j], 0.5 * np.sqrt((cr * cr).sum(1)))
    length = np.sqrt((total * total).sum(1))
    return total / np.where(length > 0, length, 1.0)[:, None], total, largest


def sphere(rings=10, radius=0.3):
    """A UV sphere around the origin, 2 * rings * (rings - 1) faces (180 at rings = 10), with its radial corner normals
    -> (verts fp32 [V, 3], faces int64 [F, 3], face_vn fp32 [F, 3, 3])."""
    lat = np.linspace(0.0, math.pi, rings + 1)[1:-1]
    lon = np.linspace(0.0, 2.0 * math.pi, rings, endpoint=False)
    ring = np.stack([np.outer(np.sin(lat), np.cos(lon)), np.broadcast_to(np.cos(lat)[:, None], (rings - 1, rings)),
                     np.outer(np.sin(lat), np.sin(lon))], -1).reshape(-1, 3)
    unit = np.concatenate([ring, [[0.0, 1.0, 0.0], [0.0, -1.0, 0.0]]])
    top, bottom = ring.shape[0], ring.shape[0] + 1
    f = []
    for i in range(rings - 2):
        for j in range(rings):
            a, b = i * rings + j, i * rings + (j + 1) % rings
            f += [(a, b, b + rings), (a, b + rings, a + rings)]
    for j in range(rings):
        f += [(top, (j + 1) % rings, j), (bottom, (rings - 2) * rings + j, (rings - 2) * rings + (j + 1) % rings)]
    faces = np.array(f)
    return (torch.from_numpy((radius * unit).astype(np.float32)), torch.from_numpy(faces.astype(np.int64)),
            torch.from_numpy(unit[faces].astype(np.float32)))
