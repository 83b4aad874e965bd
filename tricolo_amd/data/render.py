"""Multi-view renderings of ShapeNet meshes without a GL stack: the scene of the reference's data/preprocess_all_data.py:52-80,
restated for the rasteriser of csrc/raster.hip (ops.render_views).

What is restated: a perspective camera with yfov pi/3 on a square 224 x 224 viewport, pyrender's default znear 0.05, a white
background, ambient light 0.1, one white directional light of intensity 3 turned by rotation_matrix(pi/2, [-1, 0, 0]) - it shines
straight down, so the direction toward it is (0, 1, 0) - and, for view i of num_views, the camera pose R = R_y(angle) R_x(-pi/5),
eye = c + R (0, 0, 0.85) with angle = 2 pi i / num_views and c the centre of the mesh's bounding box.  That reading of trimesh's
Scene.centroid and scene.cameras.look_at (one point, a given distance) comes from their documented behaviour.  trimesh and pyrender
are not installed where this was written: NOBODY HAS COMPARED A PIXEL OF THIS RENDERER WITH PYRENDER'S OUTPUT.

Geometry is what is pinned; colour fidelity to pyrender is not claimed.  Deliberate differences:
  * Lambert by default; the glTF BRDF on request.  The default is Lambert diffuse plus ambient, Kd (0.1 + 3/pi max(n . l, 0)).
    brdf= of ops.render_views and ops.render_views_textured (brdf="gltf" below, --brdf gltf of data/preprocess.py) colours every
    position - the pixel centre, with samples=4 each sample - with the glTF 2.0 metallic-roughness model instead: base = Kd (times
    the texel), F0 = 0.04 + (base - 0.04) m, cdiff = 0.96 base (1 - m), Schlick's F, the Smith-GGX G and the GGX D with alpha = r^2,
    colour = clamp(0.1 base + 3 NL ((1 - F) cdiff / pi + F G D / (4 NL NV)), 0, 1), the view vector from the world position on the
    face, the normal flat or smooth as above (head of csrc/raster.hip).  The BRDF formulas are the glTF 2.0 specification's, which is
    public.  What rests ON MEMORY and has been checked by nobody, neither trimesh nor pyrender being installed where this was
    written: **material conversion** - that pyrender turns a trimesh SimpleMaterial into a MetallicRoughnessMaterial with
    baseColorFactor = the diffuse colour, baseColorTexture = the image, roughnessFactor = (2 / (Ns + 2))^(1/4) with Ns defaulting to
    1, and metallicFactor left at its default 1.0 (the least certain part, hence --metallic; with it the images carry almost no
    diffuse term, a face turned away from the light shows only the ambient tenth of its colour and an upward face a broad
    highlight); **default material** - that its default material is grey 0.4, metallic 0.2, roughness 0.8; **fragment shader** -
    that it follows the Khronos glTF-WebGL-PBR reference shader with the clamps NL, NV in [0.001, 1] and NH, VH in [0, 1], radiance =
    intensity times colour, ambient times base colour added, no gamma.  NOBODY HAS COMPARED A PIXEL WITH PYRENDER'S OUTPUT;
  * flat face normals by default, turned toward the eye.  Smooth shading is opt-in (normals= of ops.render_views and
    ops.render_views_textured, shading="smooth" below, --shading smooth of data/preprocess.py): the corner normals of the batch - the
    `vn` lines of the OBJ file (data/materials.py load_obj_normals) and, for faces without, vertex normals computed by
    ops.mesh_vertex_normals - are interpolated with the perspective-correct weights at the pixel centre (with samples=4, at each
    sample's own position) and lit as the flat normal is.  It rests on two readings FROM MEMORY of the published sources that nobody
    has checked, neither library being installed where this was written: that pyrender.Mesh.from_trimesh defaults to smooth=True, so
    the reference's images are shaded with per-vertex normals, and that trimesh keeps the `vn` of a file as vertex_normals or
    computes them.  Two things are OUR OWN DEFINITION: the computed normals are weighted by face AREA and summed by vertex index
    (trimesh weighs by the face's angle at the vertex, and we do not merge vertices by position), and the interpolated normal is
    turned toward the eye per position, like the flat one per face, because neither ShapeNet's winding nor its vn can be trusted -
    compared with one-sided lighting that brightens the last pixels before a silhouette.  No pixel has been compared with pyrender's;
  * no back-face culling: both sides of a face are drawn (ShapeNet's winding is unreliable);
  * map_Kd textures are opt-in (ops.render_views_textured, textures=True below; the default renders a textured material with its
    bare Kd): colour = Kd x texel, the MTL rule and - from their documentation - what trimesh's SimpleMaterial becomes in pyrender
    (baseColorFactor x baseColorTexture); repeat wrap, bilinear over texel centres at the perspective-correct (u, v) of the pixel
    centre, no gamma.  That call has NO mip-maps (the parser reduces textures to 256 texels on a side, which bounds the minification
    but a face much smaller on screen than its texture still aliases).  Mip-mapping is opt-in as well (mips= of
    ops.render_views_textured, textures="mip" below, --textures mip of data/preprocess.py): ops.texture_mips builds a pyramid of exact
    integer box means of every texture, and a pixel (with samples=4, a sample) blends the two levels around log2(rho), rho the longer
    of the two steps of (u, v), in texels, to the pixel on the right and to the pixel below - isotropic, no LOD bias; a magnified
    texture (rho <= 1) keeps the colours of the plain call bit for bit.  pyrender samples its textures through a mip chain too, but
    the level rule here is OUR OWN DEFINITION (head of csrc/raster.hip), like the voxeliser's: nobody has compared a pixel of it with
    pyrender's output, nor its level selection with OpenGL's;
  * no near-plane clipping: a face with a vertex nearer than znear is dropped whole.  model_normalized.obj lies within 0.5 of its
    centre and the camera stands 0.85 away, so no face of such a mesh comes near the plane;
  * anti-aliasing is opt-in (samples=4 below, --antialias 4x of data/preprocess.py; the default decides visibility at the pixel
    centre alone): coverage and depth at the four positions (96, 32), (224, 96), (32, 160), (160, 224) in 1/256 pixel from the pixel's
    top-left corner - the 4x rotated grid - by the same exact rules, every sample coloured as a pixel is, the pixel their rounded
    integer mean (c0 + c1 + c2 + c3 + 2) >> 2.  For untextured faces that is a multisample resolve, for textured ones 4x supersampling
    (the (u, v) of each sample's own position; no attribute is extrapolated outside its face).  It rests on our reading, FROM MEMORY,
    of pyrender's published source: its off-screen passes draw into a 4-sample multisample renderbuffer and blit it down.  pyrender is
    not installed where this was written, so nobody has checked that reading, nor pyrender's sample positions, nor a pixel.

On GPU tensors ops.render_views launches the HIP kernels; on CPU tensors the same call runs render_views_cpu below, a torch
restatement of the kernel's arithmetic (spelled out at the head of csrc/raster.hip) that gives the same bits.  It exists for
checking and for machines without a GPU and is not tuned.  ops.render_views_textured and ops.mesh_face_colours have theirs here too,
and so has the BRDF (_brdf_one).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from ..meshes import MeshBatch, clamp_index, cross, face_kd, host_boxes, pack_materials  # noqa: F401  (pack_materials: offered from here too)

YFOV, ZNEAR, IMAGE_SIZE = math.pi / 3, 0.05, 224
DISTANCE, ELEVATION = 0.85, math.pi / 5
SNAP_MAX = float(2 ** 20)
KDIFF = float(np.float32(3.0 / math.pi))
CANDIDATES_PER_PASS = 1 << 21                       # (face, pixel) pairs the fallback expands at a time
CENTRE = ((128, 128),)                              # where a pixel is sampled, in 1/256 pixel from its top-left corner: samples=1 ...
SAMPLE_OFFSETS = ((96, 32), (224, 96), (32, 160), (160, 224))                                   # ... and samples=4, the 4x rotated grid
B13, B23, B16 = (float(np.float32(c)) for c in ("0.33333334", "0.6666667", "0.16666667"))      # csrc/raster.hip RS_B13, RS_B23, RS_B16
FACE_SAMPLES = ((B13, B13, B13), (B23, B16, B16), (B16, B23, B16), (B16, B16, B23))
TEXEL_VALUE = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255.0))           # byte / 255, correctly rounded


# ------------------------------------------------------------------------------------------------ cameras
def camera_poses(center, num_views, distance=DISTANCE, elevation=ELEVATION):
    """-> (eye float64 [num_views, 3], R float64 [num_views, 3, 3]): R is the world-to-camera rotation (its rows are the camera's
    x, y, z axes in the world; the camera looks down its -z), the transpose of the pose rotation R_y(angle) R_x(-elevation) of
    preprocess_all_data.py:71-78, angle = 2 pi i / num_views; eye = center + distance * (third row of R)."""
    c = np.asarray(center, dtype=np.float64).reshape(3)
    ce, se = math.cos(-elevation), math.sin(-elevation)
    rx = np.array([[1.0, 0.0, 0.0], [0.0, ce, -se], [0.0, se, ce]])
    eyes, rots = [], []
    for i in range(int(num_views)):
        a = 2.0 * math.pi * i / num_views
        ry = np.array([[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]])
        pose = ry @ rx                                                              # camera-to-world
        eyes.append(c + pose @ np.array([0.0, 0.0, distance]))
        rots.append(pose.T)
    return np.stack(eyes) if eyes else np.zeros((0, 3)), np.stack(rots) if rots else np.zeros((0, 3, 3))


def box_centers(boxes):
    """float64 [..., 3] from meshes.host_boxes' [..., 3, 2]."""
    return 0.5 * (boxes[..., 0] + boxes[..., 1])


def bbox_center(verts):
    """The centre of the bounding box of all vertices, float64 (zeros for a mesh without vertices)."""
    return box_centers(host_boxes([verts])[0])


def pack_cameras(centers, num_views, device=None):
    """float32 [N, num_views, 12] for ops.render_views: eye, then the world-to-camera rotation row by row."""
    rows = []
    for c in centers:
        eye, rot = camera_poses(c, num_views)
        rows.append(np.concatenate([eye, rot.reshape(-1, 9)], axis=1))
    cam = np.stack(rows).astype(np.float32) if rows else np.zeros((0, int(num_views), 12), np.float32)
    return torch.from_numpy(np.ascontiguousarray(cam)).to(device or "cpu")


def projection_scales(H, W, yfov):
    """(fx, fy) as the kernel's host code forms them: float64, then rounded to fp32."""
    fy = 1.0 / math.tan(float(yfov) / 2.0)
    return float(np.float32(fy * float(H) / float(W))), float(np.float32(fy))


# ------------------------------------------------------------------------------------------------ the torch fallback
def _f32(x):
    return torch.tensor(x, dtype=torch.float32)


def snap_vertices(verts, cam, H, W, yfov, znear):
    """Per vertex of one mesh in one view: (ok bool [V], X int64 [V], Y int64 [V], d fp32 [V]) - in front of znear and inside the
    snap range, the screen position in 1/256 pixel, 1 / depth."""
    fx, fy = (_f32(s) for s in projection_scales(H, W, yfov))
    eye, R = cam[:3], cam[3:]
    q = verts - eye
    px = (R[0] * q[:, 0] + R[1] * q[:, 1]) + R[2] * q[:, 2]
    py = (R[3] * q[:, 0] + R[4] * q[:, 1]) + R[5] * q[:, 2]
    nz = -((R[6] * q[:, 0] + R[7] * q[:, 1]) + R[8] * q[:, 2])
    front = nz >= _f32(float(np.float32(znear)))
    z = torch.where(front, nz, torch.ones_like(nz))
    xf = torch.round((((fx * px) / z + 1.0) * (0.5 * W)) * 256.0)
    yf = torch.round(((1.0 - (fy * py) / z) * (0.5 * H)) * 256.0)
    inside = (xf.abs() <= SNAP_MAX) & (yf.abs() <= SNAP_MAX)
    X = torch.where(inside, xf, torch.zeros_like(xf)).to(torch.int64)
    Y = torch.where(inside, yf, torch.zeros_like(yf)).to(torch.int64)
    return front & inside, X, Y, 1.0 / z


def project_faces(verts, faces, cam, H, W, yfov, znear, with_order=False):
    """Setup of csrc/raster.hip for one mesh and one view.  verts fp32 [V, 3], faces int64 [F, 3] (already clamped to the mesh),
    cam fp32 [12] -> (keep bool [F], X int64 [F, 3], Y int64 [F, 3], d fp32 [F, 3], A2 int64 [F]) with vertices 1 and 2 swapped
    where the doubled area was negative; keep is False for dropped faces (behind znear, off the snap range, zero area).
    with_order: also order int64 [F, 3], the corner each of the three positions came from ((0, 2, 1) for a swapped face)."""
    okv, Xv, Yv, dv = snap_vertices(verts, cam, H, W, yfov, znear)
    X, Y, d = Xv[faces], Yv[faces], dv[faces]
    A2 = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (X[:, 2] - X[:, 0]) * (Y[:, 1] - Y[:, 0])
    keep = okv[faces].all(dim=1) & (A2 != 0)
    flip = A2 < 0
    order = torch.where(flip[:, None], torch.tensor([0, 2, 1]), torch.tensor([0, 1, 2]))
    out = (keep, X.gather(1, order), Y.gather(1, order), d.gather(1, order), A2.abs())
    return out + (order,) if with_order else out


def _visibility_one(verts, faces, cam, H, W, yfov, znear, offsets=CENTRE):
    """keys int64 [H * W * S] of one mesh and one view, the S = len(offsets) samples of a pixel innermost:
    bits(d) << 32 | (0xFFFFFFFF - face), 0 for background.  offsets: the sample positions in 1/256 pixel from the pixel's top-left
    corner, CENTRE or SAMPLE_OFFSETS; the box of candidate pixels holds every pixel with a sample inside the face's bounding box."""
    S = len(offsets)
    lo, hi = min(min(o) for o in offsets), max(max(o) for o in offsets)              # 128, 128 or 32, 224: csrc/raster.hip rs_setup's LO, HI
    keys = torch.zeros((H * W * S,), dtype=torch.int64)
    keep, X, Y, d, A2 = project_faces(verts, faces, cam, H, W, yfov, znear)
    x0 = ((X.amin(1) + (255 - hi)) >> 8).clamp(min=0)
    x1 = ((X.amax(1) - lo) >> 8).clamp(max=W - 1)
    y0 = ((Y.amin(1) + (255 - hi)) >> 8).clamp(min=0)
    y1 = ((Y.amax(1) - lo) >> 8).clamp(max=H - 1)
    keep = keep & (x0 <= x1) & (y0 <= y1)
    fidx = torch.nonzero(keep).reshape(-1)
    if fidx.numel() == 0:
        return keys
    bw, bh = (x1 - x0 + 1)[fidx], (y1 - y0 + 1)[fidx]
    cnt = bw * bh
    ends = torch.cumsum(cnt, 0)
    start = 0
    while start < fidx.numel():                                                     # passes of about CANDIDATES_PER_PASS pairs
        base = int(ends[start - 1]) if start else 0
        stop = int(torch.searchsorted(ends, torch.tensor(base + CANDIDATES_PER_PASS), right=True))
        stop = max(stop, start + 1)
        sel = fidx[start:stop]
        c, w = cnt[start:stop], bw[start:stop]
        rep = torch.repeat_interleave(torch.arange(sel.numel()), c)
        local = torch.arange(int(c.sum())) - torch.repeat_interleave(torch.cumsum(c, 0) - c, c)
        iy = torch.div(local, w[rep], rounding_mode="floor")
        ix = local - iy * w[rep]
        pair = sel[rep]
        for s, (ox, oy) in enumerate(offsets):
            f, px, py = pair, x0[pair] + ix, y0[pair] + iy
            Px, Py = 256 * px + ox, 256 * py + oy
            inside = torch.ones_like(f, dtype=torch.bool)
            E = []
            for k in range(3):
                a, b = (k + 1) % 3, (k + 2) % 3
                dx, dy = X[f, b] - X[f, a], Y[f, b] - Y[f, a]
                e = dx * (Py - Y[f, a]) - dy * (Px - X[f, a])
                top_left = (dy < 0) | ((dy == 0) & (dx > 0))
                inside &= (e > 0) | ((e == 0) & top_left)
                E.append(e)
            f, px, py = f[inside], px[inside], py[inside]
            fa = A2[f].to(torch.float32)
            lam = [e[inside].to(torch.float32) / fa for e in E]
            depth = (lam[0] * d[f, 0] + lam[1] * d[f, 1]) + lam[2] * d[f, 2]
            key = (depth.view(torch.int32).to(torch.int64) << 32) | (0xFFFFFFFF - f)
            keys.scatter_reduce_(0, (py * W + px) * S + s, key, reduce="amax", include_self=True)
        start = stop
    return keys


def face_textures(face_mat, mat_tex, face_uv, T):
    """int64 [F]: the (clamped, batch-global) texture of every face of one mesh, -1 for none (csrc/mesh_batch.h mb_face_tex);
    mat_tex: the mesh's rows of the batch's table."""
    if T <= 0 or mat_tex.shape[0] == 0:
        return torch.full((face_mat.shape[0],), -1, dtype=torch.int64)
    t = mat_tex[clamp_index(face_mat, mat_tex.shape[0])].to(torch.int64)
    none = (t == -1) | torch.isnan(face_uv[:, 0, 0])
    return torch.where(none, torch.full_like(t, -1), clamp_index(t, T))


def sample_textures(t, u, v, texels, tex_off, tex_size):
    """csrc/mesh_batch.h mb_tex_sample: textures t int64 [P] (0 <= t < T) at u, v fp32 [P] -> (ok bool [P], c fp32 [P, 3]); rows of c
    with ok False (a non-finite u or v) mean nothing."""
    return _sample_level(u, v, tex_size[t, 0].to(torch.int64), tex_size[t, 1].to(torch.int64), tex_off[t], int(tex_off[-1]) - 1, texels)


def sample_mip_level(t, level, u, v, mip_texels, mip_off, tex_size):
    """csrc/mesh_batch.h mb_mip_sample: level `level` int64 [P] (0 <= level < the texture's levels) of the pyramids of textures t
    int64 [P] at u, v fp32 [P] -> (ok, c) as sample_textures; the level's start is walked from tex_size as the kernels walk it."""
    H0, W0 = tex_size[t, 0].to(torch.int64), tex_size[t, 1].to(torch.int64)
    base = mip_off[t].clone()
    for k in range(int(level.max()) if level.numel() else 0):
        base += torch.where(k < level, (H0 >> k).clamp(min=1) * (W0 >> k).clamp(min=1), torch.zeros_like(base))
    return _sample_level(u, v, (H0 >> level).clamp(min=1), (W0 >> level).clamp(min=1), base, int(mip_off[-1]) - 1, mip_texels)


def _sample_level(u, v, Ht, Wt, base, last, texels):
    """The sampling rule itself on one image per row: size (Ht, Wt) int64 [P], its first texel at base int64 [P] of texels, no index
    beyond `last`."""
    ok = torch.isfinite(u) & torch.isfinite(v)
    u, v = torch.where(ok, u, torch.zeros_like(u)), torch.where(ok, v, torch.zeros_like(v))
    u, v = u - torch.floor(u), v - torch.floor(v)
    x, y = u * Wt.to(torch.float32) - 0.5, (1.0 - v) * Ht.to(torch.float32) - 0.5
    xf, yf = torch.floor(x), torch.floor(y)
    fx, fy = (x - xf)[:, None], (y - yf)[:, None]
    xa, ya = torch.remainder(xf.to(torch.int64), Wt), torch.remainder(yf.to(torch.int64), Ht)
    xb, yb = torch.where(xa + 1 == Wt, torch.zeros_like(xa), xa + 1), torch.where(ya + 1 == Ht, torch.zeros_like(ya), ya + 1)

    def texel(row, col):
        return TEXEL_VALUE[texels[(base + row * Wt + col).clamp(0, last), :3].to(torch.int64)]

    t00, t10, t01, t11 = texel(ya, xa), texel(ya, xb), texel(yb, xa), texel(yb, xb)
    a, b = t00 + (t10 - t00) * fx, t01 + (t11 - t01) * fx
    return ok, a + (b - a) * fy


def texture_mips_cpu(texels, tex_off, tex_size):
    """ops.texture_mips on CPU tensors -> (mip_texels u8 [sumMipTexels, 4], mip_off int64 [T + 1]): the integers of csrc/mesh_batch.h in
    torch.  Per level and axis the weights wy [H_l, H0], wx [W_l, W0] of the interval overlaps, S = wy texel0 wx^T in int64, the texel
    (2 S + D) // (2 D) with D = H0 W0; level 0 is copied.  Dense weight matrices: untuned, for checking."""
    from ..meshes import mip_level_sizes, mip_offsets
    mip_off = mip_offsets(tex_size)
    out = torch.empty((int(mip_off[-1]), 4), dtype=torch.uint8)
    for t, (H0, W0) in enumerate(tex_size.tolist()):
        src = texels[int(tex_off[t]):int(tex_off[t]) + H0 * W0]
        at = int(mip_off[t])
        out[at:at + H0 * W0] = src
        at += H0 * W0
        tex = src[:, :3].reshape(H0, W0, 3).to(torch.int64)
        for Hl, Wl in mip_level_sizes(H0, W0)[1:]:
            w = []
            for n0, nl in ((H0, Hl), (W0, Wl)):                                     # overlap of [y n0, (y + 1) n0] with [i nl, (i + 1) nl]
                y, i = torch.arange(nl)[:, None], torch.arange(n0)[None, :]
                w.append((torch.minimum((y + 1) * n0, (i + 1) * nl) - torch.maximum(y * n0, i * nl)).clamp(min=0))
            S = torch.einsum("yi,ijk,xj->yxk", w[0], tex, w[1])
            D = H0 * W0
            out[at:at + Hl * Wl, :3] = torch.div(2 * S + D, 2 * D, rounding_mode="floor").reshape(-1, 3).to(torch.uint8)
            out[at:at + Hl * Wl, 3] = 255
            at += Hl * Wl
    return out, mip_off


def sample_mips(t, u, v, right, down, mip_texels, mip_off, tex_size):
    """The level of detail and the blend of two pyramid levels (head of csrc/raster.hip, rs_texel<true>): textures t int64 [P] at
    u, v fp32 [P]; right, down: (u, v, d) of the same face one whole pixel to the right and one whole pixel down -> (ok, c) as
    sample_textures."""
    (ux, vx, dx), (uy, vy, dy) = right, down
    H0, W0 = tex_size[t, 0].to(torch.int64), tex_size[t, 1].to(torch.int64)
    Hf, Wf = H0.to(torch.float32), W0.to(torch.float32)
    a, b, c, e = (ux - u) * Wf, (vx - v) * Hf, (uy - u) * Wf, (vy - v) * Hf
    r2 = torch.maximum(a * a + b * b, c * c + e * e)
    bounded = (dx > 0) & (dy > 0) & torch.isfinite(ux) & torch.isfinite(vx) & torch.isfinite(uy) & torch.isfinite(vy) & torch.isfinite(r2)
    rho = torch.sqrt(torch.where(bounded, r2, torch.ones_like(r2)))
    top = torch.frexp(torch.maximum(H0, W0).to(torch.float64))[1].to(torch.int64) - 1     # levels - 1: the bit length of the longer side, - 1
    mant, ex = torch.frexp(rho)                                                     # rho = mant 2^ex with mant in [0.5, 1)
    l, g = ex.to(torch.int64) - 1, mant * 2.0 - 1.0                                 # floor(log2(rho)) and rho 2^-l - 1, both exact
    two = bounded & (rho > 1.0) & (l < top)
    lo = torch.where(bounded, torch.where(rho <= 1.0, torch.zeros_like(top), torch.where(l < top, l, top)), top)
    ok, c0 = sample_mip_level(t, lo, u, v, mip_texels, mip_off, tex_size)
    _, c1 = sample_mip_level(t, torch.where(two, lo + 1, lo), u, v, mip_texels, mip_off, tex_size)
    return ok, torch.where(two[:, None], c0 + (c1 - c0) * g[:, None], c0)


def _weights(X, Y, d, fa, f, Px, Py):
    """csrc/raster.hip rs_weights: ([b0, b1, b2], d) fp32 [P] of the faces f int64 [P] of project_faces' (X, Y, d) at the positions
    (Px, Py) in 1/256 pixel, fa = fl32(2A) of those faces: l_k = fl32(E_k) / fa, w_k = l_k d_k, d = (w0 + w1) + w2, b_k = w_k / d."""
    w = []
    for k in range(3):
        a, b = (k + 1) % 3, (k + 2) % 3
        e = (X[f, b] - X[f, a]) * (Py - Y[f, a]) - (Y[f, b] - Y[f, a]) * (Px - X[f, a])
        w.append((e.to(torch.float32) / fa) * d[f, k])
    dd = (w[0] + w[1]) + w[2]
    return [wk / dd for wk in w], dd


def _smooth_one(verts, faces, cam, H, W, yfov, znear, vis, face_vn, offsets=CENTRE):
    """(has bool [HW S], shade fp32 [HW S]) of one mesh and one view: where the winning face of vis int64 [HW S] has corner normals
    (face_vn fp32 [F, 3, 3], the mesh's rows) and their interpolation at the sample's own position is finite and has a length, and the
    smooth shade there (head of csrc/raster.hip, rs_smooth_shade); everywhere else the caller keeps the flat shade."""
    has = torch.zeros((vis.numel(),), dtype=torch.bool)
    shade = torch.zeros((vis.numel(),), dtype=torch.float32)
    pix = torch.nonzero((vis >= 0) & ~torch.isnan(face_vn[vis.clamp(min=0), 0, 0])).reshape(-1)
    if pix.numel() == 0:
        return has, shade
    _, X, Y, d, A2, order = project_faces(verts, faces, cam, H, W, yfov, znear, with_order=True)
    f = vis[pix]
    S, off = len(offsets), torch.tensor(offsets, dtype=torch.int64)
    pixel, s = torch.div(pix, S, rounding_mode="floor"), pix % S
    Px, Py = 256 * (pixel % W) + off[s, 0], 256 * torch.div(pixel, W, rounding_mode="floor") + off[s, 1]
    bw, _ = _weights(X, Y, d, A2[f].to(torch.float32), f, Px, Py)
    vn = face_vn[f].gather(1, order[f][:, :, None].expand(-1, 3, 3))
    n = [(bw[0] * vn[:, 0, j] + bw[1] * vn[:, 1, j]) + bw[2] * vn[:, 2, j] for j in range(3)]
    length = torch.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    ok = torch.isfinite(n[0]) & torch.isfinite(n[1]) & torch.isfinite(n[2]) & (length != 0)
    e = cam[:3] - verts[faces[f, 0]]
    side = (n[0] * e[:, 0] + n[1] * e[:, 1]) + n[2] * e[:, 2]
    ny = n[1] / torch.where(ok, length, torch.ones_like(length))
    ndl = torch.where(side < 0, -ny, ny).clamp(min=0.0)
    has[pix[ok]] = True
    shade[pix[ok]] = (0.1 + _f32(KDIFF) * ndl)[ok]
    return has, shade


def _texels_one(verts, faces, cam, H, W, yfov, znear, vis, face_t, face_uv, texels, tex_off, tex_size, offsets=CENTRE, mips=None):
    """(has bool [HW S], c fp32 [HW S, 3]) of one mesh and one view: where the winning face of vis int64 [HW S] (the S = len(offsets)
    samples of a pixel innermost) is textured, and the texture colour at the perspective-correct (u, v) of the sample's own position
    - the pixel centre for CENTRE.  mips: the pyramid pair; the colour is then sample_mips', its footprint from the positions one whole
    pixel (256) to the right and down."""
    has = torch.zeros((vis.numel(),), dtype=torch.bool)
    c = torch.ones((vis.numel(), 3), dtype=torch.float32)
    pix = torch.nonzero((vis >= 0) & (face_t[vis.clamp(min=0)] >= 0)).reshape(-1)
    if pix.numel() == 0:
        return has, c
    _, X, Y, d, A2, order = project_faces(verts, faces, cam, H, W, yfov, znear, with_order=True)
    f = vis[pix]
    S, off = len(offsets), torch.tensor(offsets, dtype=torch.int64)
    pixel, s = torch.div(pix, S, rounding_mode="floor"), pix % S
    Px, Py = 256 * (pixel % W) + off[s, 0], 256 * torch.div(pixel, W, rounding_mode="floor") + off[s, 1]
    fa = A2[f].to(torch.float32)
    uv = face_uv[f].gather(1, order[f][:, :, None].expand(-1, 3, 2))

    def uvd(Px, Py):
        bw, dd = _weights(X, Y, d, fa, f, Px, Py)
        return ((bw[0] * uv[:, 0, 0] + bw[1] * uv[:, 1, 0]) + bw[2] * uv[:, 2, 0],
                (bw[0] * uv[:, 0, 1] + bw[1] * uv[:, 1, 1]) + bw[2] * uv[:, 2, 1], dd)

    u, v, _ = uvd(Px, Py)
    if mips is None:
        ok, col = sample_textures(face_t[f], u, v, texels, tex_off, tex_size)
    else:
        ok, col = sample_mips(face_t[f], u, v, uvd(Px + 256, Py), uvd(Px, Py + 256), mips[0], mips[1], tex_size)
    has[pix[ok]] = True
    c[pix[ok]] = col[ok]
    return has, c


def _shade_one(verts, faces, face_mat, kd, cam, vis, tex=None, smooth=None):
    """u8 [3, HW] of one mesh and one view from its visibility buffer vis int64 [HW] (-1 = background); tex: _texels_one's pair;
    smooth: _smooth_one's pair, whose shade replaces the flat one where it has one.
    Every entry is coloured on its own, so a four-sample buffer [HW 4] gives the four sample colours of every pixel."""
    out = torch.full((3, vis.numel()), 255, dtype=torch.uint8)
    pix = torch.nonzero(vis >= 0).reshape(-1)
    if pix.numel() == 0:
        return out
    f = vis[pix]
    a = verts[faces[f, 0]]
    cx, cy, cz = cross(a, verts[faces[f, 1]], verts[faces[f, 2]])
    length = torch.sqrt((cx * cx + cy * cy) + cz * cz)
    e = cam[:3] - a
    side = (cx * e[:, 0] + cy * e[:, 1]) + cz * e[:, 2]
    ok = length > 0
    ny = cy / torch.where(ok, length, torch.ones_like(length))
    ndl = torch.where(ok, torch.where(side < 0, -ny, ny).clamp(min=0.0), torch.zeros_like(ny))
    shade = 0.1 + _f32(KDIFF) * ndl
    if smooth is not None:
        shade = torch.where(smooth[0][pix], smooth[1][pix], shade)
    colour = face_kd(face_mat[f], kd)
    if tex is not None:
        colour = torch.where(tex[0][pix][:, None], colour * tex[1][pix], colour)
    rgb = torch.floor(255.0 * (colour * shade[:, None]).clamp(0.0, 1.0) + 0.5).to(torch.uint8)
    out[:, pix] = rgb.t()
    return out


PI32 = float(np.float32(math.pi))                                                  # csrc/raster.hip RS_PI
DEFAULT_PBR = (0.2, 0.8)                                                            # (metallic, roughness) of a mesh without materials


def _clamp(x, lo, hi):
    """fminf(fmaxf(x, lo), hi): a NaN takes the lower bound (torch.clamp would keep it)."""
    return torch.fmin(torch.fmax(x, _f32(lo)), _f32(hi))


def face_pbr(face_mat, pbr):
    """(metallic, roughness) fp32 [F] each: csrc/mesh_batch.h mb_face_pbr - the factors of every face's (clamped) material, clamped
    to [0, 1] and [0.04, 1] with a NaN taking the lower bound; DEFAULT_PBR for a mesh without materials."""
    if pbr.shape[0] > 0:
        mr = pbr[clamp_index(face_mat, pbr.shape[0])]
    else:
        mr = torch.tensor(DEFAULT_PBR, dtype=torch.float32).expand(face_mat.shape[0], 2)
    return _clamp(mr[:, 0], 0.0, 1.0), _clamp(mr[:, 1], 0.04, 1.0)


def _brdf_one(verts, faces, face_mat, kd, pbr, cam, H, W, yfov, znear, vis, tex=None, face_vn=None, offsets=CENTRE):
    """u8 [3, HW S] of one mesh and one view from its visibility buffer vis int64 [HW S] under the metallic-roughness BRDF (head of
    csrc/raster.hip, rs_resolve_brdf): every entry coloured at its own position.  pbr: the mesh's rows of mat_pbr; tex: _texels_one's
    pair; face_vn: the mesh's corner normals for the smooth normal, or None.  Where the BRDF falls back the entry takes the Lambert
    colour of _shade_one."""
    out = torch.full((3, vis.numel()), 255, dtype=torch.uint8)
    pix = torch.nonzero(vis >= 0).reshape(-1)
    if pix.numel() == 0:
        return out
    f = vis[pix]
    eye = cam[:3]
    corner = verts[faces[f]]                                                        # [P, 3, 3]
    a = corner[:, 0]
    e = eye - a

    def turned(x, length, has_length):
        side = (x[0] * e[:, 0] + x[1] * e[:, 1]) + x[2] * e[:, 2]
        safe = torch.where(has_length, length, torch.ones_like(length))
        unit = [torch.where(has_length, xj / safe, torch.zeros_like(xj)) for xj in x]
        return torch.stack([torch.where(side < 0, -u, u) for u in unit], dim=1)

    x = cross(a, corner[:, 1], corner[:, 2])
    length = torch.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])
    n = turned(x, length, length > 0)
    good = (length > 0) & torch.isfinite(length)

    keep, X, Y, d, A2, order = project_faces(verts, faces, cam, H, W, yfov, znear, with_order=True)
    S, off = len(offsets), torch.tensor(offsets, dtype=torch.int64)
    pixel, s = torch.div(pix, S, rounding_mode="floor"), pix % S
    Px, Py = 256 * (pixel % W) + off[s, 0], 256 * torch.div(pixel, W, rounding_mode="floor") + off[s, 1]
    bw, _ = _weights(X, Y, d, A2[f].to(torch.float32), f, Px, Py)
    if face_vn is not None:
        vn = face_vn[f].gather(1, order[f][:, :, None].expand(-1, 3, 3))
        y = [(bw[0] * vn[:, 0, j] + bw[1] * vn[:, 1, j]) + bw[2] * vn[:, 2, j] for j in range(3)]
        ylen = torch.sqrt((y[0] * y[0] + y[1] * y[1]) + y[2] * y[2])
        has = keep[f] & ~torch.isnan(face_vn[f, 0, 0]) & torch.isfinite(y[0]) & torch.isfinite(y[1]) & torch.isfinite(y[2]) & (ylen != 0)
        n = torch.where(has[:, None], turned(y, ylen, has), n)
        good = torch.where(has, torch.isfinite(ylen), good)

    base = face_kd(face_mat[f], kd)
    if tex is not None:
        base = torch.where(tex[0][pix][:, None], base * tex[1][pix], base)
    shade = 0.1 + _f32(KDIFF) * torch.fmax(n[:, 1], _f32(0.0))
    lambert = _clamp(base * shade[:, None], 0.0, 1.0)

    P = corner.gather(1, order[f][:, :, None].expand(-1, 3, 3))                     # the corners in the swapped order
    q = [eye[j] - ((bw[0] * P[:, 0, j] + bw[1] * P[:, 1, j]) + bw[2] * P[:, 2, j]) for j in range(3)]
    dist = torch.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2])
    ok = keep[f] & good & torch.isfinite(bw[0]) & torch.isfinite(bw[1]) & torch.isfinite(bw[2]) & (dist > 0) & torch.isfinite(dist)
    v = [qj / torch.where(ok, dist, torch.ones_like(dist)) for qj in q]
    g = [v[0], 1.0 + v[1], v[2]]
    hl = torch.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
    ok = ok & (hl > 0) & torch.isfinite(hl)
    h = [gj / torch.where(ok, hl, torch.ones_like(hl)) for gj in g]
    NL = _clamp(n[:, 1], 0.001, 1.0)
    NV = _clamp(((n[:, 0] * v[0] + n[:, 1] * v[1]) + n[:, 2] * v[2]).abs(), 0.001, 1.0)
    NH = _clamp((n[:, 0] * h[0] + n[:, 1] * h[1]) + n[:, 2] * h[2], 0.0, 1.0)
    VH = _clamp((v[0] * h[0] + v[1] * h[1]) + v[2] * h[2], 0.0, 1.0)
    w = 1.0 - VH
    w5 = (((w * w) * w) * w) * w
    metal, rough = face_pbr(face_mat[f], pbr)
    alpha = rough * rough
    a2 = alpha * alpha

    def smith(c):
        return (2.0 * c) / (c + torch.sqrt(a2 + (1.0 - a2) * (c * c)))

    G = smith(NL) * smith(NV)
    t = (NH * NH) * (a2 - 1.0) + 1.0
    D = a2 / ((_f32(PI32) * t) * t)
    spec = ((G * D) / ((4.0 * NL) * NV))[:, None]
    light = (3.0 * NL)[:, None]
    F0 = 0.04 + (base - 0.04) * metal[:, None]
    cdiff = (0.96 * base) * (1.0 - metal)[:, None]
    F = F0 + (1.0 - F0) * w5[:, None]
    colour = _clamp(0.1 * base + light * (((1.0 - F) * cdiff) / _f32(PI32) + F * spec), 0.0, 1.0)
    rgb = torch.floor(255.0 * torch.where(ok[:, None], colour, lambert) + 0.5).to(torch.uint8)
    out[:, pix] = rgb.t()
    return out


def render_views_cpu(verts, faces, vert_off, face_off, face_mat, mat_kd, mat_off, cam, H, W, yfov=YFOV, znear=ZNEAR,
                     return_visibility=False, textures=None, samples=1, mips=None, normals=None, brdf=None):
    """ops.render_views on CPU tensors: one mesh and one view after the other, the kernel's arithmetic in torch.  textures: the five
    texture tensors of the batch (face_uv, mat_tex, texels, tex_off, tex_size) for ops.render_views_textured.  samples=4: coverage,
    depth and colour at the four SAMPLE_OFFSETS of every pixel, the pixel their rounded integer mean (c0 + c1 + c2 + c3 + 2) >> 2 per
    channel, the visibility int32 [N, views, H, W, 4].  mips: the pyramid pair (texture_mips_cpu) for the mip-mapped colours of
    ops.render_views_textured(..., mips=).  normals: the batch's corner normals face_vn fp32 [sumF, 3, 3] for the smooth shade of
    ops.render_views(..., normals=) - interpolated at every sample's own position - in any of those modes.  brdf: the batch's PBR
    factors mat_pbr fp32 [sumM, 2] for the metallic-roughness colours of ops.render_views(..., brdf=), in any of those modes."""
    if samples not in (1, 4):
        raise ValueError(f"render_views_cpu: samples must be 1 or 4, got {samples!r}")
    offsets = SAMPLE_OFFSETS if samples == 4 else CENTRE
    voff, foff, moff = vert_off.tolist(), face_off.tolist(), mat_off.tolist()
    N, views = len(voff) - 1, cam.shape[1]
    image = torch.full((N, views, 3, H, W), 255, dtype=torch.uint8)
    vis = torch.full((N, views, H, W) + ((4,) if samples == 4 else ()), -1, dtype=torch.int32)
    for n in range(N):
        v = verts[voff[n]:voff[n + 1]]
        f = faces[foff[n]:foff[n + 1]]
        if v.shape[0] == 0 or f.shape[0] == 0 or H * W == 0:
            continue
        f = clamp_index(f, v.shape[0])
        fm, kd = face_mat[foff[n]:foff[n + 1]], mat_kd[moff[n]:moff[n + 1]]
        for k in range(views):
            keys = _visibility_one(v, f, cam[n, k], H, W, yfov, znear, offsets)
            face = torch.where(keys != 0, 0xFFFFFFFF - (keys & 0xFFFFFFFF), torch.full_like(keys, -1))
            vis[n, k] = face.to(torch.int32).view(vis.shape[2:])
            tex = None
            if textures is not None:
                face_uv, mat_tex, texels, tex_off, tex_size = textures
                uv = face_uv[foff[n]:foff[n + 1]]
                face_t = face_textures(fm, mat_tex[moff[n]:moff[n + 1]], uv, tex_size.shape[0])
                tex = _texels_one(v, f, cam[n, k], H, W, yfov, znear, face, face_t, uv, texels, tex_off, tex_size, offsets, mips)
            vn = None if normals is None else normals[foff[n]:foff[n + 1]]
            if brdf is not None:
                colour = _brdf_one(v, f, fm, kd, brdf[moff[n]:moff[n + 1]], cam[n, k], H, W, yfov, znear, face, tex, vn, offsets)
            else:
                smooth = None if vn is None else _smooth_one(v, f, cam[n, k], H, W, yfov, znear, face, vn, offsets)
                colour = _shade_one(v, f, fm, kd, cam[n, k], face, tex, smooth)
            if samples == 4:
                colour = ((colour.view(3, H * W, 4).to(torch.int32).sum(dim=2) + 2) >> 2).to(torch.uint8)
            image[n, k] = colour.view(3, H, W)
    return (image, vis) if return_visibility else image


def mesh_face_colours_cpu(verts, faces, vert_off, face_off, face_mat, mat_kd, mat_off, face_uv, mat_tex, texels, tex_off, tex_size):
    """ops.mesh_face_colours on CPU tensors -> fp32 [sumF, 3]: Kd, for a textured face times the mean of the four samples of
    FACE_SAMPLES (summed in their order, times 0.25); the UVs are used affinely."""
    foff, moff = face_off.tolist(), mat_off.tolist()
    out = torch.empty((faces.shape[0], 3), dtype=torch.float32)
    for n in range(len(foff) - 1):
        fm, uv = face_mat[foff[n]:foff[n + 1]], face_uv[foff[n]:foff[n + 1]]
        colour = face_kd(fm, mat_kd[moff[n]:moff[n + 1]])
        face_t = face_textures(fm, mat_tex[moff[n]:moff[n + 1]], uv, tex_size.shape[0])
        sel = torch.nonzero(face_t >= 0).reshape(-1)
        if sel.numel():
            t, q = face_t[sel], uv[sel]
            ok, total = torch.ones_like(sel, dtype=torch.bool), None
            for b0, b1, b2 in FACE_SAMPLES:
                good, c = sample_textures(t, (b0 * q[:, 0, 0] + b1 * q[:, 1, 0]) + b2 * q[:, 2, 0],
                                          (b0 * q[:, 0, 1] + b1 * q[:, 1, 1]) + b2 * q[:, 2, 1], texels, tex_off, tex_size)
                ok, total = ok & good, c if total is None else total + c
            colour[sel[ok]] = colour[sel[ok]] * (total[ok] * 0.25)
        out[foff[n]:foff[n + 1]] = colour
    return out


NORMAL_CLAMP, NORMAL_SCALE = float(2 ** 16), float(2 ** 36)                       # csrc/mesh_normals.hip MN_CLAMP, MN_SCALE


def mesh_vertex_normals_cpu(verts, faces, vert_off, face_off, face_vn=None, fill_all=False):
    """ops.mesh_vertex_normals on CPU tensors -> face_vn fp32 [sumF, 3, 3]: the integers and the float64 of csrc/mesh_normals.hip in
    torch.  Per mesh the fp32 cross products (meshes.cross) of the faces whose three components are finite, clamped to +-2^16 and
    rounded to int64 at 2^36 (torch.round: ties to even), are index_add_-ed at the faces' clamped vertices; a corner is
    fl32(fl64(S) / sqrt((S_x^2 + S_y^2) + S_z^2)); a face with a corner whose sum is (0, 0, 0), or of a mesh without vertices, is nine
    NaNs.  Unless fill_all, a face whose face_vn[f, 0, 0] is not NaN keeps its nine values."""
    voff, foff = vert_off.tolist(), face_off.tolist()
    out = torch.full((faces.shape[0], 3, 3), float("nan"), dtype=torch.float32)
    for n in range(len(voff) - 1):
        V, f = voff[n + 1] - voff[n], faces[foff[n]:foff[n + 1]]
        if V <= 0 or f.shape[0] == 0:
            continue
        v, f = verts[voff[n]:voff[n + 1]], clamp_index(f, V)
        c = torch.stack(cross(v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]), dim=1)
        q = torch.round(c.clamp(-NORMAL_CLAMP, NORMAL_CLAMP).to(torch.float64) * NORMAL_SCALE)
        q = torch.where(torch.isfinite(c).all(dim=1, keepdim=True), q, torch.zeros_like(q)).to(torch.int64)
        acc = torch.zeros((V, 3), dtype=torch.int64)
        for j in range(3):
            acc.index_add_(0, f[:, j], q)
        S = acc[f]                                                                  # [F, 3 corners, 3]
        x, y, z = (S[:, :, k].to(torch.float64) for k in range(3))
        some = (S != 0).any(dim=2)
        length = torch.where(some, torch.sqrt((x * x + y * y) + z * z), torch.ones_like(x))
        normal = torch.stack([x / length, y / length, z / length], dim=2).to(torch.float32)
        out[foff[n]:foff[n + 1]] = torch.where(some.all(dim=1)[:, None, None], normal, torch.full_like(normal, float("nan")))
    if face_vn is not None and not fill_all:
        given = ~torch.isnan(face_vn[:, 0, 0])
        out[given] = face_vn[given]
    return out


SHADING_MODES = ("flat", "smooth")
BRDF_MODES = ("lambert", "gltf")


# ------------------------------------------------------------------------------------------------ the convenient calls
def render_batch(batch, num_views=12, image_size=IMAGE_SIZE, return_visibility=False, textures=False, samples=1, shading="flat",
                 brdf="lambert"):
    """The reference's num_views renderings of every mesh of a meshes.MeshBatch packed with materials -> uint8
    [N, num_views, 3, S, S] on the batch's device: places the cameras around every mesh's bounding-box centre and calls
    ops.render_views, or with textures=True ops.render_views_textured (the batch must have been packed with textures).
    textures="mip": render_views_textured with the mip pyramid of the batch's textures, built here (MeshBatch.with_texture_mips)
    unless the batch carries one.  samples=4: four coverage samples per pixel (ops.render_views).  shading="smooth": the batch's
    corner normals batch.face_vn (MeshBatch.pack(..., face_vn_list=) and / or MeshBatch.with_vertex_normals()) are interpolated
    across every face that has them (normals= of the two calls); a batch without face_vn raises.  brdf="gltf": the glTF
    metallic-roughness BRDF with the batch's PBR factors batch.mat_pbr (MeshBatch.pack(..., pbr_list=); brdf= of the two calls) in
    place of the Lambert shade, in any of those modes; a batch without mat_pbr raises."""
    from .. import ops
    if not isinstance(textures, bool) and textures != "mip":
        raise ValueError(f"textures must be False, True or \"mip\", got {textures!r}")
    if shading not in SHADING_MODES:
        raise ValueError(f"shading must be one of {SHADING_MODES}, got {shading!r}")
    if shading == "smooth" and batch.face_vn is None:
        raise ValueError("render_batch: shading=\"smooth\" needs corner normals - MeshBatch.pack(..., face_vn_list=) or "
                         "MeshBatch.with_vertex_normals()")
    if brdf not in BRDF_MODES:
        raise ValueError(f"brdf must be one of {BRDF_MODES}, got {brdf!r}")
    if brdf == "gltf" and batch.mat_pbr is None:
        raise ValueError("render_batch: brdf=\"gltf\" needs the materials' PBR factors - MeshBatch.pack(..., pbr_list=)")
    normals = batch.face_vn if shading == "smooth" else None
    pbr = batch.pbr_tensor if brdf == "gltf" else None
    cam = pack_cameras(box_centers(batch.boxes), num_views, batch.verts.device)
    H, W = (image_size, image_size) if isinstance(image_size, int) else image_size
    if textures:
        mips = None
        if textures == "mip":
            if batch.tex_size is None:
                raise ValueError("render_batch: the batch was packed without textures (MeshBatch.pack(..., face_uv_list=, mat_tex_list=, textures_list=))")
            mips = (batch if batch.mip_texels is not None else batch.with_texture_mips()).mip_tensors
        return ops.render_views_textured(*batch.tensors, *batch.texture_tensors, cam, H, W, YFOV, ZNEAR, return_visibility, samples=samples,
                                         mips=mips, normals=normals, brdf=pbr)
    return ops.render_views(*batch.tensors, cam, H, W, YFOV, ZNEAR, return_visibility, samples=samples, normals=normals, brdf=pbr)


def render_meshes(verts_list, faces_list, face_mat_list, kd_list, num_views=12, image_size=IMAGE_SIZE, device=None, return_visibility=False,
                  textures=False, face_uv_list=None, mat_tex_list=None, textures_list=None, samples=1, face_vn_list=None, brdf="lambert",
                  pbr_list=None):
    """render_batch of the lists, packed (meshes.MeshBatch.pack) on `device` (where verts_list[0] lives when None); textures=True
    and textures="mip" need the three texture lists of MeshBatch.pack.  face_vn_list (per mesh float32 [F, 3, 3], NaN rows for faces
    without; data.materials.load_obj_normals) turns smooth shading on: the faces without normals take computed ones
    (MeshBatch.with_vertex_normals(fill="missing")) and the batch is rendered with shading="smooth".  brdf="gltf" with pbr_list (per
    mesh float32 [M, 2]; data.materials.load_obj_pbr) renders with the metallic-roughness BRDF."""
    batch = MeshBatch.pack(verts_list, faces_list, face_mat_list, kd_list, device, face_uv_list=face_uv_list, mat_tex_list=mat_tex_list,
                           textures_list=textures_list, face_vn_list=face_vn_list, pbr_list=pbr_list)
    if face_vn_list is None:
        return render_batch(batch, num_views, image_size, return_visibility, textures, samples, brdf=brdf)
    return render_batch(batch.with_vertex_normals(fill="missing"), num_views, image_size, return_visibility, textures, samples, shading="smooth",
                        brdf=brdf)
