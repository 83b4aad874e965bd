"""An independent statement of the textured shading of csrc/raster.hip (ops.render_views_textured) for the tests: float64 numpy,
one mesh and one view.  Which face a pixel shows comes from tests/raster_reference.visibility (itself a float64 brute force, with
its `ambiguous` pixels); this file colours it its own way.  It shares with the code under test only the vertices' snapped integer
screen positions (tricolo_amd.data.render.snap_vertices), as raster_reference does.  Everything else is taken differently:
  * the screen barycentrics are E_k / 2A from the exact edge functions of the face in its ORIGINAL corner order (no swap - the signs
    cancel), the depths 1 / z come from a float64 camera transform, the perspective-correct weights are b_k / z_k normalised;
  * (u, v) wraps by repeat, the texel position is x = u W - 1/2, y = (1 - v) H - 1/2 (row 0 = top, v = 0 = bottom), the four
    neighbours wrap, and the bilinear blend is the weighted sum of the four texels;
  * the Lambert shade (light from +y, ambient 0.1, intensity 3 / pi, normal turned toward the eye) is formed in float64;
  * colour = clamp(Kd texel shade, 0, 1), u8 = floor(255 colour + 1/2); an untextured face (material without a texture, or a NaN in
    its UVs) is Kd shade.
With affine=True the UVs are interpolated with the screen barycentrics alone - WRONG on purpose, for the test that shows the
perspective division is visible.  face_colours is the float64 statement of ops.mesh_face_colours."""
import math

import numpy as np

from tests import raster_reference as rr
from tricolo_amd.data import render as R

SAMPLES = ((1 / 3, 1 / 3, 1 / 3), (2 / 3, 1 / 6, 1 / 6), (1 / 6, 2 / 3, 1 / 6), (1 / 6, 1 / 6, 2 / 3))


def sample(tex, u, v):
    """tex uint8 [H, W, >= 3], u and v float64 [P] -> float64 [P, 3]: repeat wrap, bilinear over texel centres."""
    Ht, Wt = tex.shape[:2]
    t = tex[:, :, :3].astype(np.float64) / 255.0
    u, v = u - np.floor(u), v - np.floor(v)
    x, y = u * Wt - 0.5, (1.0 - v) * Ht - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[:, None], (y - y0)[:, None]
    xa, ya = np.mod(x0.astype(np.int64), Wt), np.mod(y0.astype(np.int64), Ht)
    xb, yb = np.mod(xa + 1, Wt), np.mod(ya + 1, Ht)
    return (t[ya, xa] * (1 - fx) + t[ya, xb] * fx) * (1 - fy) + (t[yb, xa] * (1 - fx) + t[yb, xb] * fx) * fy


def shades(v, f, eye):
    """float64 [F]: 0.1 + 3 / pi max(n . (0, 1, 0), 0) with the unit normal turned toward the eye; 0.1 for a face without area."""
    a = v[f[:, 0]]
    nrm = np.cross(v[f[:, 1]] - a, v[f[:, 2]] - a)
    ln = np.linalg.norm(nrm, axis=1)
    ny = np.where(ln > 0, nrm[:, 1] / np.where(ln > 0, ln, 1.0), 0.0)
    ny = np.where((nrm * (eye - a)).sum(1) < 0, -ny, ny)
    return 0.1 + 3.0 / math.pi * np.maximum(ny, 0.0)


def render(verts, faces, face_mat, kd, face_uv, mat_tex, textures, cam, H, W, yfov=R.YFOV, znear=R.ZNEAR, affine=False):
    """One mesh, one view.  verts fp32 [V, 3], faces int64 [F, 3], face_mat int [F], kd fp32 [M, 3], face_uv fp32 [F, 3, 2], mat_tex
    int [M] (indices into `textures`, -1 = none; torch tensors), textures a list of uint8 [H, W, 4] arrays, cam fp32 [12]
    -> (image uint8 [3, H, W], face int64 [H, W], ambiguous bool [H, W])."""
    face, ambiguous, covered = rr.visibility(verts, faces, cam, H, W, yfov, znear)
    okv, Xv, Yv, _ = R.snap_vertices(verts, cam, H, W, yfov, znear)
    X, Y = Xv.numpy().astype(np.float64), Yv.numpy().astype(np.float64)
    v, c, f = verts.numpy().astype(np.float64), cam.numpy().astype(np.float64), faces.numpy()
    inv_z = 1.0 / np.where(okv.numpy(), -((v - c[:3]) @ c[9:12]), 1.0)
    kd64, uv64 = kd.numpy().astype(np.float64), face_uv.numpy().astype(np.float64)
    mt, fm = np.asarray(mat_tex).astype(np.int64), np.asarray(face_mat).astype(np.int64)
    shade = shades(v, f, c[:3])
    image = np.full((3, H, W), 255, np.uint8)
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
    uv = (wgt[:, :, None] * uv64[fw]).sum(1)
    colour = kd64[fm[fw]].copy()
    tex_of = mt[fm[fw]]
    tex_of = np.where(np.isnan(uv64[fw, 0, 0]), -1, tex_of)
    for t in np.unique(tex_of[tex_of >= 0]):
        sel = tex_of == t
        colour[sel] *= sample(textures[t], uv[sel, 0], uv[sel, 1])
    colour = np.clip(colour * shade[fw][:, None], 0.0, 1.0)
    image[:, py, px] = np.floor(255.0 * colour + 0.5).astype(np.uint8).T
    return image, face, ambiguous


def face_colours(face_mat, kd, face_uv, mat_tex, textures):
    """float64 [F, 3] of one mesh: Kd, times the mean of the four SAMPLES of its texture for a textured face (UVs used affinely)."""
    kd64, uv64 = kd.numpy().astype(np.float64), face_uv.numpy().astype(np.float64)
    out = kd64[np.asarray(face_mat).astype(np.int64)].copy()
    tex_of = np.asarray(mat_tex).astype(np.int64)[np.asarray(face_mat).astype(np.int64)]
    for i in range(out.shape[0]):
        if tex_of[i] >= 0 and not np.isnan(uv64[i, 0, 0]):
            pts = np.array([[sum(b[k] * uv64[i, k, j] for k in range(3)) for j in range(2)] for b in SAMPLES])
            out[i] *= sample(textures[tex_of[i]], pts[:, 0], pts[:, 1]).mean(0)
    return out
