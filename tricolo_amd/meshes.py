"""The packed batch of triangle meshes that the sampler, the renderer and the voxeliser share (csrc/mesh_batch.h lays it out): reading
OBJ files, validating and packing lists of meshes (with their materials and, on request, their textures) on the host, the float64 bounding boxes the cameras and voxel frames come from, and
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


TEXTURE_MAX_SIDE = 2 ** 24                                                         # texel positions are formed in fp32


def check_textures(face_uv, mat_tex, texels, tex_off, tex_size, num_faces, num_materials):
    """The five texture fields of csrc/mesh_batch.h, validated on the host (ValueError): shapes and dtypes, mat_tex in [-1, T), every
    texture 1 <= H, W <= 2^24, tex_off the running sum of H * W ending at the number of texels."""
    for name, x, dtype, tail in (("face_uv", face_uv, torch.float32, (3, 2)), ("mat_tex", mat_tex, torch.int32, ()),
                                 ("texels", texels, torch.uint8, (4,)), ("tex_off", tex_off, torch.int64, ()), ("tex_size", tex_size, torch.int32, (2,))):
        if not torch.is_tensor(x) or x.dtype != dtype or x.dim() != 1 + len(tail) or tuple(x.shape[1:]) != tail:
            raise ValueError(f"{name} must be a {dtype} tensor of shape {['*', *tail]}")
    T = tex_size.shape[0]
    if face_uv.shape[0] != num_faces or mat_tex.shape[0] != num_materials or tex_off.shape[0] != T + 1:
        raise ValueError(f"textures: {face_uv.shape[0]} face_uv rows for {num_faces} faces, {mat_tex.shape[0]} mat_tex entries for "
                         f"{num_materials} materials, {tex_off.shape[0]} offsets for {T} textures")
    if mat_tex.numel() and (int(mat_tex.min()) < -1 or int(mat_tex.max()) >= T):
        raise ValueError(f"mat_tex spans {int(mat_tex.min())} .. {int(mat_tex.max())} but the batch has {T} textures (-1 = none)")
    size = tex_size.to("cpu", torch.int64)
    if T and (int(size.min()) < 1 or int(size.max()) > TEXTURE_MAX_SIDE):
        raise ValueError(f"every texture needs 1 <= H, W <= 2^24, got sizes from {int(size.min())} to {int(size.max())}")
    want = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(size[:, 0] * size[:, 1], 0)])
    if not torch.equal(tex_off.cpu(), want) or int(want[-1]) != texels.shape[0]:
        raise ValueError("tex_off must be the running sum of H * W over tex_size and end at the number of texels")


def mip_level_sizes(height, width):
    """[(H_l, W_l)] of the mip chain of a texture of size (height, width), both >= 1: floor(log2(max(H, W))) + 1 levels, level l of
    size (max(1, H >> l), max(1, W >> l)) (csrc/mesh_batch.h)."""
    height, width = int(height), int(width)
    return [(max(1, height >> l), max(1, width >> l)) for l in range(max(height, width).bit_length())]


def mip_offsets(tex_size):
    """int64 [T + 1] on the host: where the chain of every texture starts in the pyramid, the running sum of the chain lengths."""
    off = [0]
    for h, w in tex_size.to("cpu", torch.int64).tolist():
        off.append(off[-1] + sum(hl * wl for hl, wl in mip_level_sizes(h, w)))
    return torch.tensor(off, dtype=torch.int64)


def check_texture_mips(mip_texels, mip_off, tex_size):
    """The two pyramid fields of csrc/mesh_batch.h against the batch's tex_size, validated on the host (ValueError): shapes and
    dtypes, one device, mip_off the running sum of the chain lengths ending at the number of pyramid texels."""
    for name, x, dtype, tail in (("mip_texels", mip_texels, torch.uint8, (4,)), ("mip_off", mip_off, torch.int64, ())):
        if not torch.is_tensor(x) or x.dtype != dtype or x.dim() != 1 + len(tail) or tuple(x.shape[1:]) != tail:
            raise ValueError(f"{name} must be a {dtype} tensor of shape {['*', *tail]}")
    if not mip_texels.device == mip_off.device == tex_size.device:
        raise ValueError("the mip pyramid must live on the device of the textures it was built from")
    T = tex_size.shape[0]
    if mip_off.shape[0] != T + 1:
        raise ValueError(f"mip_off holds {mip_off.shape[0]} offsets for {T} textures")
    want = mip_offsets(tex_size)
    if not torch.equal(mip_off.cpu(), want) or int(want[-1]) != mip_texels.shape[0]:
        raise ValueError(f"mip_off must be the running sum of the chain lengths of tex_size and end at the number of pyramid texels: "
                         f"{int(want[-1])} for these textures, got {mip_texels.shape[0]}")


def pack_textures(face_uv_list, mat_tex_list, textures_list, device=None):
    """Per mesh: face_uv fp32 [F, 3, 2] (a NaN row = no texture coordinates), mat_tex int [M] indexing that mesh's own list of
    textures (-1 = none), textures a list of uint8 [H, W, 4] RGBA arrays or tensors (row 0 = top)
    -> (face_uv, mat_tex with batch-global indices, texels u8 [sumTexels, 4], tex_off int64 [T + 1], tex_size int32 [T, 2])."""
    device = device or "cpu"
    mat_tex, texels, sizes, base = [], [], [], 0
    for n, (mt, texs) in enumerate(zip(mat_tex_list, textures_list)):
        mt = torch.as_tensor(mt).to(torch.int64).reshape(-1)
        if mt.numel() and (int(mt.min()) < -1 or int(mt.max()) >= len(texs)):
            raise ValueError(f"mesh {n}: texture indices span {int(mt.min())} .. {int(mt.max())} but the mesh has {len(texs)} textures (-1 = none)")
        mat_tex.append(torch.where(mt < 0, mt, mt + base).to(torch.int32))
        for k, tex in enumerate(texs):
            tex = torch.as_tensor(tex)
            if tex.dtype != torch.uint8 or tex.dim() != 3 or tex.shape[2] != 4 or tex.shape[0] < 1 or tex.shape[1] < 1:
                raise ValueError(f"mesh {n}: texture {k} must be a uint8 array of shape [H >= 1, W >= 1, 4]")
            sizes.append((tex.shape[0], tex.shape[1]))
            texels.append(tex.reshape(-1, 4))
        base += len(texs)
    off = [0]
    for h, w in sizes:
        off.append(off[-1] + h * w)
    return (torch.cat([torch.as_tensor(uv).to(device) for uv in face_uv_list]).contiguous() if face_uv_list else torch.zeros((0, 3, 2), device=device),
            torch.cat(mat_tex).to(device).contiguous() if mat_tex else torch.zeros((0,), dtype=torch.int32, device=device),
            torch.cat(texels).to(device).contiguous() if texels else torch.zeros((0, 4), dtype=torch.uint8, device=device),
            torch.tensor(off, dtype=torch.int64, device=device), torch.tensor(sizes, dtype=torch.int32, device=device).reshape(-1, 2))


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
    """A packed batch on one device; the three material tensors are None for a batch packed without materials, the five texture
    tensors for a batch packed without textures, the two pyramid tensors until with_texture_mips() has built them, face_vn for a
    batch packed without face_vn_list until with_vertex_normals() has computed it, mat_pbr for a batch packed without pbr_list."""
    verts: torch.Tensor
    faces: torch.Tensor
    vert_off: torch.Tensor
    face_off: torch.Tensor
    face_mat: torch.Tensor | None
    mat_kd: torch.Tensor | None
    mat_off: torch.Tensor | None
    max_faces: int                                  # the largest face count of a mesh (sizes ops.mesh_face_cdf's grid)
    boxes: np.ndarray                               # host_boxes of the input lists
    face_uv: torch.Tensor | None = None
    mat_tex: torch.Tensor | None = None
    texels: torch.Tensor | None = None
    tex_off: torch.Tensor | None = None
    tex_size: torch.Tensor | None = None
    mip_texels: torch.Tensor | None = None          # the mip pyramid of the textures (with_texture_mips); None without one
    mip_off: torch.Tensor | None = None
    face_vn: torch.Tensor | None = None             # corner normals fp32 [sumF, 3, 3], a NaN row = a face without; None without any
    mat_pbr: torch.Tensor | None = None             # (metallic, roughness) fp32 [sumM, 2] per material, indexed like mat_kd; None without

    @classmethod
    def pack(cls, verts_list, faces_list, face_mat_list=None, kd_list=None, device=None, *, face_uv_list=None, mat_tex_list=None,
             textures_list=None, face_vn_list=None, pbr_list=None):
        """pack_meshes, then pack_materials where face_mat_list and kd_list are given; device=None: where verts_list[0] lives.  With
        face_uv_list, mat_tex_list and textures_list (all three, beside the materials) pack_textures adds the texture fields,
        validated by check_textures.  face_vn_list: per mesh the corner normals float32 [F, 3, 3] (data.materials.load_obj_normals;
        all nine values NaN for a face without), concatenated into face_vn.  pbr_list: per mesh the (metallic, roughness) of its
        materials, float32 [M, 2] beside its Kd [M, 3] (data.materials.load_obj_pbr), concatenated into mat_pbr; the values are not
        range-checked - the renderer clamps them."""
        verts, faces, voff, foff, max_faces = pack_meshes(verts_list, faces_list, device)
        mats = (None, None, None)
        if face_mat_list is not None:
            if len(face_mat_list) != len(faces_list) or any(fm.shape[0] != f.shape[0] for fm, f in zip(face_mat_list, faces_list)):
                raise ValueError("every mesh needs one material index per face")
            mats = pack_materials(face_mat_list, kd_list, verts.device)
        tex = (None,) * 5
        given = [x is not None for x in (face_uv_list, mat_tex_list, textures_list)]
        if any(given):
            if not all(given) or face_mat_list is None:
                raise ValueError("textures need face_uv_list, mat_tex_list and textures_list, and the materials they belong to")
            if not len(face_uv_list) == len(mat_tex_list) == len(textures_list) == len(faces_list):
                raise ValueError("every mesh needs its face_uv, mat_tex and list of textures")
            for n, (uv, f, mt, kd) in enumerate(zip(face_uv_list, faces_list, mat_tex_list, kd_list)):
                if not torch.is_tensor(uv) or uv.dtype != torch.float32 or tuple(uv.shape) != (f.shape[0], 3, 2):
                    raise ValueError(f"mesh {n}: face_uv must be a float32 tensor of shape [{f.shape[0]}, 3, 2]")
                if len(mt) != kd.shape[0]:
                    raise ValueError(f"mesh {n}: {len(mt)} mat_tex entries for {kd.shape[0]} materials")
            tex = pack_textures(face_uv_list, mat_tex_list, textures_list, verts.device)
            check_textures(*tex, faces.shape[0], mats[1].shape[0])
        face_vn = None
        if face_vn_list is not None:
            if len(face_vn_list) != len(faces_list):
                raise ValueError("every mesh needs its face_vn")
            for n, (vn, f) in enumerate(zip(face_vn_list, faces_list)):
                if not torch.is_tensor(vn) or vn.dtype != torch.float32 or tuple(vn.shape) != (f.shape[0], 3, 3):
                    raise ValueError(f"mesh {n}: face_vn must be a float32 tensor of shape [{f.shape[0]}, 3, 3]")
            face_vn = torch.cat([vn.to(verts.device) for vn in face_vn_list]).contiguous()
        mat_pbr = None
        if pbr_list is not None:
            if face_mat_list is None or len(pbr_list) != len(faces_list):
                raise ValueError("every mesh needs its pbr factors, and the materials they belong to")
            for n, (pbr, kd) in enumerate(zip(pbr_list, kd_list)):
                if not torch.is_tensor(pbr) or pbr.dtype != torch.float32 or tuple(pbr.shape) != (kd.shape[0], 2):
                    raise ValueError(f"mesh {n}: pbr must be a float32 tensor of shape [{kd.shape[0]}, 2] = (metallic, roughness) per material")
            mat_pbr = torch.cat([pbr.to(verts.device) for pbr in pbr_list]).contiguous()
        return cls(verts, faces, voff, foff, *mats, max_faces, host_boxes(verts_list), *tex, face_vn=face_vn, mat_pbr=mat_pbr)

    @property
    def tensors(self):                              # the first seven arguments of ops.render_views and ops.voxelize_meshes, in their order
        return self.verts, self.faces, self.vert_off, self.face_off, self.face_mat, self.mat_kd, self.mat_off

    @property
    def texture_tensors(self):                      # the next five arguments of ops.render_views_textured and ops.mesh_face_colours
        return self.face_uv, self.mat_tex, self.texels, self.tex_off, self.tex_size

    @property
    def mip_tensors(self):                          # the mips= pair of ops.render_views_textured, None for a batch without a pyramid
        return None if self.mip_texels is None else (self.mip_texels, self.mip_off)

    @property
    def pbr_tensor(self):                           # the brdf= argument of ops.render_views and ops.render_views_textured, None without pbr_list
        return self.mat_pbr

    def with_texture_mips(self):
        """The batch with the mip pyramid of its textures (ops.texture_mips, built once on the batch's device; validated by
        check_texture_mips): what render_batch(..., textures="mip") renders from.  Everything else is shared, not copied."""
        from dataclasses import replace

        from . import ops
        if self.tex_size is None:
            raise ValueError("with_texture_mips: the batch was packed without textures")
        mip_texels, mip_off = ops.texture_mips(self.texels, self.tex_off, self.tex_size)
        check_texture_mips(mip_texels, mip_off, self.tex_size)
        return replace(self, mip_texels=mip_texels, mip_off=mip_off)

    def with_vertex_normals(self, fill="missing"):
        """The batch with computed corner normals (ops.mesh_vertex_normals: area-weighted, by vertex index; head of
        csrc/mesh_normals.hip): what render_batch(..., shading="smooth") renders from.  fill="missing" keeps the normals the batch
        was packed with and fills the faces without; fill="all" overwrites every face.  Everything else is shared, not copied."""
        from dataclasses import replace

        from . import ops
        return replace(self, face_vn=ops.mesh_vertex_normals(self.verts, self.faces, self.vert_off, self.face_off, self.face_vn, fill))

    def with_face_colours(self, colours):
        """The batch with one material per face, `colours` fp32 [sumF, 3] (ops.mesh_face_colours) as their Kd, and no textures or
        normals: what the voxeliser takes to colour its voxels from textures.  face_mat counts up within every mesh and mat_off = face_off;
        mat_pbr, where the batch has it, becomes one row per face, that of the face's (clamped) material."""
        sumF = self.faces.shape[0]
        if not torch.is_tensor(colours) or colours.dtype != torch.float32 or tuple(colours.shape) != (sumF, 3) or colours.device != self.verts.device:
            raise ValueError(f"colours must be a float32 tensor of shape [{sumF}, 3] on the batch's device")
        counts = self.face_off[1:] - self.face_off[:-1]
        local = torch.arange(sumF, dtype=torch.int64, device=self.verts.device) - torch.repeat_interleave(self.face_off[:-1], counts)
        mat_pbr = None
        if self.mat_pbr is not None:
            count = torch.repeat_interleave(self.mat_off[1:] - self.mat_off[:-1], counts)                 # the materials of every face's mesh
            j = torch.minimum(self.face_mat.to(torch.int64) & 0xFFFFFFFF, (count - 1).clamp(min=0))      # the kernels' unsigned clamp
            default = self.mat_pbr.new_tensor([[0.2, 0.8]])                                               # a mesh without materials
            rows = torch.cat([self.mat_pbr, default])[(torch.repeat_interleave(self.mat_off[:-1], counts) + j).clamp(max=self.mat_pbr.shape[0])]
            mat_pbr = torch.where((count > 0)[:, None], rows, default).contiguous()
        return MeshBatch(self.verts, self.faces, self.vert_off, self.face_off, local.to(torch.int32), colours.contiguous(), self.face_off.clone(),
                         self.max_faces, self.boxes, mat_pbr=mat_pbr)


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
