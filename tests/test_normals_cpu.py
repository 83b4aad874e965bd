"""CPU: smooth shading - normals= of ops.render_views and ops.render_views_textured on CPU tensors, the torch restatement of the SMOOTH
resolve kernels of csrc/raster.hip - against the float64 statement of tests/normals_reference.py; ops.mesh_vertex_normals on CPU
tensors (the restatement of csrc/mesh_normals.hip) against the float64 sums of that file and against its own promises (independent
of the face order, fill, batching, the clamp); the identities that tie the mode to the existing calls byte for byte; the `vn` parser;
the refusals; and python -m tricolo_amd.data.preprocess --shading smooth end to end on the host.

The scenes are those of tests/test_texture_cpu.py (one triangle, the soup, the flat quads at different depths) with random corner
normals of length 0.5 to 2, and a UV sphere of 180 faces with radial normals.  Normals do not change visibility, so the pixels left
out of a comparison are raster_reference's `ambiguous` ones plus those normals_reference adds (the sign of n . e, a vanishing
normal), together under the 1 % cap.  Colours may differ from float64 by 1 LSB, the allowance of tests/test_texture_cpu.py: the fp32
error of the interpolated unit normal is some 1e-6, three orders below an LSB of 255 Kd 0.955 n_y, so only a value next to a rounding
boundary of floor(255 c + 0.5) moves, and then by one.

Vertex normals against float64: a face of area A contributes a cross product of length 2 A whose fp32 error is a few 2^-24 of the
edge products and whose fixed-point rounding is 2^-37 per component; for areas of 1e-6 and more the rounding is below 1e-5 of the
contribution and the fp32 error dominates, some 1e-7 of it.  Where the sum at a vertex is longer than 1e-3 of the largest area there,
the direction is therefore off by 1e-7 / 1e-3 = 1e-4 rad at the most.  Measured on the scenes below: 5.3e-8 rad (sphere), 5.9e-6
(the soup, whose slivers have edge products far above their area), 4.2e-7 (fan).

The check_* functions run here on the host and from tests/test_gpu_normals.py on the GPU."""
import math
import os

import numpy as np
import pytest
import torch

from tests import normals_reference as nr
from tests import raster_reference as rr
from tests import test_mip_cpu as tm
from tests import test_preprocess as tp
from tests import test_texture_cpu as tc
from tricolo_amd import _C, ops
from tricolo_amd import config as tcfg
from tricolo_amd.data import preprocess as pp
from tricolo_amd.data import render as R
from tricolo_amd.data.materials import load_obj_materials, load_obj_normals
from tricolo_amd.meshes import MeshBatch, load_obj

MODES = ("plain", "textured", "mip")
NAN = float("nan")


def random_normals(n, seed):
    """fp32 [n, 3, 3]: random directions, lengths 0.5 to 2."""
    g = np.random.default_rng(seed)
    d = g.normal(size=(n, 3, 3))
    d *= (g.uniform(0.5, 2.0, (n, 3, 1)) / np.linalg.norm(d, axis=2, keepdims=True))
    return torch.from_numpy(d.astype(np.float32))


def scene(name):
    """tests/test_mip_cpu.scene (its six textures) plus "vn"; "sphere": normals_reference.sphere, one material, one view at 32 x 32."""
    if name == "sphere":
        verts, faces, vn = nr.sphere()
        s = dict(verts=verts, faces=faces, fm=torch.zeros(faces.shape[0], dtype=torch.int32), kd=torch.tensor([[0.9, 0.8, 0.7]]),
                 uv=tc.random_uv(faces.shape[0], 47), mt=torch.tensor([3], dtype=torch.int32), texs=tm.mip_textures(),
                 cam=R.pack_cameras([R.bbox_center(verts)], 1)[0], H=32, W=32, yfov=R.YFOV)
    else:
        s = tm.scene(name, 0)
        vn = random_normals(s["faces"].shape[0], 60)
        if name == "soup":
            vn[30] = NAN                                                                 # a face without normals among the others
            vn[31, 2, 1] = float("inf")                                                  # not the marker: flat where the normal is not finite
    s["vn"] = vn
    return s


def pack(scenes, device="cpu"):
    return MeshBatch.pack([s["verts"] for s in scenes], [s["faces"] for s in scenes], [s["fm"] for s in scenes], [s["kd"] for s in scenes], device,
                          face_uv_list=[s["uv"] for s in scenes], mat_tex_list=[s["mt"] for s in scenes], textures_list=[s["texs"] for s in scenes],
                          face_vn_list=[s["vn"] for s in scenes]).with_texture_mips()


def render(batch, cam, H, W, yfov=R.YFOV, mode="plain", samples=1, normals=None):
    """(image, vis) on the CPU of the call `mode` names, with normals= (None: the call as it was)."""
    cam = cam.to(batch.verts.device)
    if mode == "plain":
        out = ops.render_views(*batch.tensors, cam, H, W, yfov, R.ZNEAR, return_visibility=True, samples=samples, normals=normals)
    else:
        out = ops.render_views_textured(*batch.tensors, *batch.texture_tensors, cam, H, W, yfov, R.ZNEAR, return_visibility=True, samples=samples,
                                        mips=batch.mip_tensors if mode == "mip" else None, normals=normals)
    return out[0].cpu(), out[1].cpu()


# ---------------------------------------------------------------------------------------------------- against float64
@pytest.mark.parametrize("name", ["triangle", "soup", "quads", "sphere"])
def test_restatement_matches_the_float64_reference(name):
    s = scene(name)
    batch = pack([s])
    img, vis = render(batch, s["cam"][None], s["H"], s["W"], s["yfov"], normals=batch.face_vn)
    compared = smooth = left_out = covered = worst = 0
    for k in range(s["cam"].shape[0]):
        want, face, ambiguous, has = nr.render(s["verts"], s["faces"], s["fm"], s["kd"], s["vn"], s["cam"][k], s["H"], s["W"], s["yfov"])
        keep = ~ambiguous
        assert np.array_equal(vis[0, k].numpy()[keep], face[keep])
        diff = np.abs(img[0, k].numpy().astype(int) - want.astype(int))[:, keep]
        compared, worst = compared + int((face[keep] >= 0).sum()), max(worst, int(diff.max()))
        smooth, left_out, covered = smooth + int((has & keep).sum()), left_out + int((ambiguous & (face >= 0)).sum()), covered + int((face >= 0).sum())
    print(f"{name}: {compared} covered pixels compared ({smooth} smooth), {left_out} of {covered} left out, largest colour difference {worst}")
    assert left_out <= rr.MAX_AMBIGUOUS * covered, "the scene leaves too many pixels out - change the scene"
    assert compared > (100 if name in ("soup", "sphere") else 20) and smooth > 0.8 * compared and worst <= 1


def test_the_perspective_division_is_visible():
    s = tc.slanted_quad()
    per_vertex = torch.tensor([[0.0, 1.0, 0.2], [0.0, 1.0, 0.2], [0.0, 0.2, 1.0], [0.0, 0.2, 1.0]])
    vn = per_vertex[s["faces"]].contiguous()
    batch = MeshBatch.pack([s["verts"]], [s["faces"]], [s["fm"]], [s["kd"]], face_vn_list=[vn])
    img, vis = ops.render_views(*batch.tensors, s["cam"][None], s["H"], s["W"], return_visibility=True, normals=batch.face_vn)
    args = (s["verts"], s["faces"], s["fm"], s["kd"], vn, s["cam"][0], s["H"], s["W"])
    right, face, ambiguous, _ = nr.render(*args)
    wrong = nr.render(*args, affine=True)[0]
    keep = ~ambiguous & (face >= 0)
    assert keep.sum() > 50
    assert np.abs(img[0, 0].numpy().astype(int) - right.astype(int))[:, keep].max() <= 1
    apart = np.abs(right.astype(int) - wrong.astype(int))[:, keep].max()
    print(f"perspective against affine normals: up to {apart} LSB apart")
    assert apart > 1


# ---------------------------------------------------------------------------------------------------- identities, byte for byte
def check_identities(device="cpu"):
    soup, tri = scene("soup"), scene("triangle")
    tri["cam"] = R.pack_cameras([R.bbox_center(tri["verts"])], 3)[0]
    batch = pack([soup, tri], device)
    cam, H, W = torch.stack([soup["cam"], tri["cam"]]), 32, 48
    none = torch.full_like(batch.face_vn, NAN)
    for mode in MODES:
        for samples in (1, 4):
            base = render(batch, cam, H, W, mode=mode, samples=samples)
            assert (base[1] >= 0).sum() > 100
            got = render(batch, cam, H, W, mode=mode, samples=samples, normals=none)         # no face has normals: the call as it was
            assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), f"all NaN, {mode}, {samples} sample(s)"
            got = render(batch, cam, H, W, mode=mode, samples=samples, normals=batch.face_vn)
            assert torch.equal(got[1], base[1]), f"visibility, {mode}, {samples} sample(s)"
            assert not torch.equal(got[0], base[0]), f"{mode}, {samples} sample(s): the picture does change"
    # one face with three equal corner normals: the negated normal is turned back toward the eye
    one = scene("triangle")
    for normal in ([0.3, 0.8, 0.5], [-0.2, -0.4, 0.9], [1.0, 0.0, 0.0]):
        vn = torch.tensor(normal).expand(1, 3, 3).contiguous()
        single = MeshBatch.pack([one["verts"]], [one["faces"]], [one["fm"]], [one["kd"]], device, face_vn_list=[vn])
        args = (*single.tensors, one["cam"][None].to(device), 16, 16)
        a = ops.render_views(*args, normals=single.face_vn).cpu()
        b = ops.render_views(*args, normals=(-single.face_vn).contiguous()).cpu()
        assert torch.equal(a, b) and int(a.min()) < 255, normal


def test_identities():
    check_identities()


def test_a_smooth_sphere_shows_more_grey_levels_than_a_flat_one():
    s = scene("sphere")
    batch = pack([s])
    row = s["H"] // 2
    flat = render(batch, s["cam"][None], s["H"], s["W"])[0][0, 0, 0, row]
    smooth = render(batch, s["cam"][None], s["H"], s["W"], normals=batch.face_vn)[0][0, 0, 0, row]
    levels = [len(set(x[x != 255].tolist())) for x in (flat, smooth)]
    print(f"grey levels along the middle row of the sphere: {levels[0]} flat, {levels[1]} smooth")
    assert levels[1] > levels[0]


# ---------------------------------------------------------------------------------------------------- vertex normals
def fan(n=300):
    """n faces around vertex 0, the apex of a shallow cone over a rim of n vertices."""
    a = np.linspace(0.0, 2.0 * math.pi, n, endpoint=False)
    rim = np.stack([0.3 * np.cos(a), np.full(n, -0.1), 0.3 * np.sin(a)], 1)
    verts = torch.from_numpy(np.concatenate([[[0.0, 0.0, 0.0]], rim]).astype(np.float32))
    faces = torch.tensor([[0, 1 + (i + 1) % n, 1 + i] for i in range(n)], dtype=torch.int64)
    return verts, faces


def normals_of(meshes, device="cpu", face_vn=None, fill="missing"):
    batch = MeshBatch.pack([m[0] for m in meshes], [m[1] for m in meshes], device=device)
    return ops.mesh_vertex_normals(batch.verts, batch.faces, batch.vert_off, batch.face_off, None if face_vn is None else face_vn.to(device), fill).cpu()


def bits(t):
    return t.contiguous().view(torch.int32)


def vertex_meshes():
    sphere = nr.sphere()[:2]
    return [sphere, rr.soup(), fan()]


def test_vertex_normals_against_float64():
    worst = 0.0
    for name, (verts, faces) in zip(("sphere", "soup", "fan"), vertex_meshes()):
        got = normals_of([(verts, faces)]).numpy().astype(np.float64)
        want, total, largest = nr.vertex_normals(verts, faces)
        sure = np.sqrt((total * total).sum(1)) > 1e-3 * largest
        f = faces.numpy()
        rows = sure[f]                                                                   # [F, 3]: the corners to compare
        assert rows.sum() > 0.9 * rows.size and not np.isnan(got[rows]).any(), name
        cos = (got[rows] * want[f][rows]).sum(1) / np.linalg.norm(got[rows], axis=1)
        cross = np.linalg.norm(np.cross(got[rows], want[f][rows]), axis=1) / np.linalg.norm(got[rows], axis=1)
        angle = np.arctan2(cross, cos)
        print(f"{name}: {int(rows.sum())} corners compared, largest angle {angle.max():.2e} rad")
        worst = max(worst, float(angle.max()))
        assert np.abs(np.linalg.norm(got[rows], axis=1) - 1.0).max() < 1e-6, name
    assert worst < 1e-4


def test_the_sphere_s_computed_normals_are_nearly_radial():
    verts, faces, radial = nr.sphere()
    got = normals_of([(verts, faces)])
    cos = (got * radial).sum(2).clamp(-1.0, 1.0)
    print(f"sphere: computed normals within {float(torch.acos(cos).max()):.3f} rad of radial")
    assert float(torch.acos(cos).max()) < 0.2


def check_face_order_and_repeats(device="cpu"):
    for name, (verts, faces) in zip(("sphere", "soup", "fan"), vertex_meshes()):
        base = normals_of([(verts, faces)], device)
        assert torch.equal(bits(normals_of([(verts, faces)], device)), bits(base)), f"{name}: two calls"
        perm = torch.from_numpy(np.random.default_rng(9).permutation(faces.shape[0]))
        assert torch.equal(bits(normals_of([(verts, faces[perm])], device)), bits(base[perm])), f"{name}: face order"
    verts, faces = fan()
    apex = normals_of([(verts, faces)], device)[:, 0]                                    # corner 0 of every face is the apex
    assert torch.equal(bits(apex), bits(apex[:1].expand_as(apex))) and float(apex[0, 1]) > 0.9


def test_face_order_and_repeats():
    check_face_order_and_repeats()


def check_fill(device="cpu"):
    verts, faces, radial = nr.sphere()
    given = radial * 1.5
    given[::3] = NAN
    computed = normals_of([(verts, faces)], device)
    missing = normals_of([(verts, faces)], device, given, "missing")
    every = normals_of([(verts, faces)], device, given, "all")
    marked = torch.isnan(given[:, 0, 0])
    assert torch.equal(bits(missing[~marked]), bits(given[~marked])) and torch.equal(bits(missing[marked]), bits(computed[marked]))
    assert torch.equal(bits(every), bits(computed)) and not torch.isnan(computed).any()


def test_fill():
    check_fill()
    with pytest.raises(ValueError):
        normals_of([nr.sphere()[:2]], fill="some")


def test_coincident_faces_of_opposite_winding_have_no_normal():
    verts = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 1.0], [0.0, 1.0, 1.0]])
    faces = torch.tensor([[0, 1, 2], [0, 2, 1], [3, 4, 5]])
    got = normals_of([(verts, faces)])
    assert torch.isnan(got[:2]).all() and torch.equal(got[2], torch.tensor([0.0, 0.0, 1.0]).expand(3, 3))


def test_batching_and_empty_meshes():
    sphere, soup, cone = vertex_meshes()
    empty_faces = (sphere[0][:5].contiguous(), torch.zeros((0, 3), dtype=torch.int64))
    empty_verts = (torch.zeros((0, 3)), torch.zeros((0, 3), dtype=torch.int64))
    meshes = [sphere, empty_faces, soup, empty_verts, cone]
    got = normals_of(meshes)
    at = 0
    for m in meshes:
        F = m[1].shape[0]
        if F:
            assert torch.equal(bits(got[at:at + F]), bits(normals_of([m])))
        at += F
    assert at == got.shape[0] and tuple(normals_of([empty_faces, empty_verts]).shape) == (0, 3, 3)


def test_a_bad_vertex_index_takes_the_clamp():
    verts, faces = nr.sphere()[:2]
    V = verts.shape[0]
    off = (torch.tensor([0, V]), torch.tensor([0, faces.shape[0]]))
    good = faces.to(torch.int32).clone()
    good[7, 1], good[9, 2] = V - 1, V - 1
    bad = good.clone()
    bad[7, 1], bad[9, 2] = V + 50, -3
    assert torch.equal(bits(ops.mesh_vertex_normals(verts, bad, *off)), bits(ops.mesh_vertex_normals(verts, good, *off)))


# ---------------------------------------------------------------------------------------------------- the parser
OBJ = """v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
v 0.5 1.5 0
vt 0 0
vn 0 0 1
vn 0 1 0
vn 1 0 0
f 1//1 2//2 3//3
f 1/1/3 2/1/2 3/1/1
vn 0 0 -2
f 1//-1 2//-2 3//-4
f 1//1 2//2 3//3 4//4 5//1
f 1//1 2 3//3
f 1//1 2//2 3//9
f 1/1 2/1 3/1
vn 0 nan 1
vn 1 2
f 1//5 2//1 3//1
f 1//1 2//6 3//1
"""


@pytest.mark.parametrize("newline", ["\n", "\r\n"])
def test_obj_normals(tmp_path, newline):
    path = str(tmp_path / "m.obj")
    with open(path, "wb") as f:
        f.write(OBJ.replace("\n", newline).encode())
    vn = load_obj_normals(path)
    z, y, x, back = [0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, -2.0]
    assert vn.dtype == torch.float32 and tuple(vn.shape) == (11, 3, 3) and vn.shape[0] == load_obj(path)[1].shape[0]
    assert vn[0].tolist() == [z, y, x]                                                     # i//k
    assert vn[1].tolist() == [x, y, z]                                                     # i/j/k
    assert vn[2].tolist() == [back, x, z]                                                  # negative: counted back from the four read so far
    assert vn[3].tolist() == [z, y, x] and vn[4].tolist() == [z, x, back] and vn[5].tolist() == [z, back, z]      # the pentagon, fanned
    assert torch.isnan(vn[6:]).all()        # a corner without vn; an index beyond the file; no third index; a vn that is not finite; a short vn line


def test_obj_normals_row_count_must_match(tmp_path, monkeypatch):
    path = str(tmp_path / "m.obj")
    with open(path, "w") as f:
        f.write("v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nf 1//1 2//1 3//1\n")
    from tricolo_amd.data import materials
    monkeypatch.setattr(materials, "load_obj", lambda p: (torch.zeros((3, 3)), torch.zeros((2, 3), dtype=torch.int64)))
    with pytest.raises(ValueError):
        load_obj_normals(path)


# ---------------------------------------------------------------------------------------------------- refusals
def check_refusals(device="cpu"):
    s = scene("triangle")
    batch = pack([s], device)
    cam = s["cam"][None].to(device)
    other = "cpu" if torch.device(device).type == "cuda" else "meta"
    bad = [batch.face_vn.double(), batch.face_vn[:, :2].contiguous(), batch.face_vn.reshape(-1, 9), batch.face_vn.to(other),
           torch.cat([batch.face_vn, batch.face_vn]), batch.face_vn.numpy() if device == "cpu" else [1.0]]
    for normals in bad:
        with pytest.raises(ValueError):
            ops.render_views(*batch.tensors, cam, 8, 8, normals=normals)
        with pytest.raises(ValueError):
            ops.render_views_textured(*batch.tensors, *batch.texture_tensors, cam, 8, 8, normals=normals)
    with pytest.raises(ValueError):
        ops.mesh_vertex_normals(batch.verts, batch.faces, batch.vert_off, batch.face_off, batch.face_vn.double())


def test_refusals():
    check_refusals()
    s = scene("triangle")
    lists = ([s["verts"]], [s["faces"]], [s["fm"]], [s["kd"]])
    for vn in (s["vn"].double(), s["vn"][:, :2], torch.cat([s["vn"], s["vn"]]), s["vn"].numpy()):
        with pytest.raises(ValueError):
            MeshBatch.pack(*lists, face_vn_list=[vn])
    with pytest.raises(ValueError):
        MeshBatch.pack(*lists, face_vn_list=[s["vn"], s["vn"]])
    plain = MeshBatch.pack(*lists)
    assert plain.face_vn is None and len(plain.tensors) == 7 and len(plain.texture_tensors) == 5
    with pytest.raises(ValueError):
        R.render_batch(plain, 2, 8, shading="smooth")
    with pytest.raises(ValueError):
        R.render_batch(plain, 2, 8, shading="gouraud")
    packed = pack([s])
    assert packed.face_vn is not None and packed.with_texture_mips().face_vn is packed.face_vn
    assert packed.with_face_colours(ops.mesh_face_colours(packed)).face_vn is None
    assert "[--shading flat|smooth]" in pp.__doc__ and pp.SHADING_MODES == ("flat", "smooth")
    with pytest.raises(SystemExit):
        pp.main(["--shading", "bumpy"], log=lambda *a: None)


def test_entry_points_refuse_bad_arguments_before_anything_runs():
    lib = _C.lib()
    tail, some = (None, None, None, None), 64                                                                 # `some`: not null, never read
    TEX, VN = _C.TRI_MESH_TEXTURES, _C.TRI_MESH_NORMALS

    def null(N, T, face_vn, fields=VN):                                                                       # every other pointer null
        return _C.TriMeshBatch(N=N, T=T, face_vn=face_vn, fields=fields)

    view = (None, 200, 3, 8, 8, R.YFOV, R.ZNEAR)
    assert lib.tri_raster_render(null(1, 0, None), *view, 1, *tail) == _C.TRI_ERR_ARG
    assert "face_vn" in lib.tri_last_error().decode()
    assert lib.tri_raster_render(null(1, 0, some), *view, 2, *tail) == _C.TRI_ERR_ARG                         # samples
    assert lib.tri_raster_render(null(1, 3, some, TEX | VN), *view, 1, *tail) == _C.TRI_ERR_ARG              # textures without fields
    assert lib.tri_raster_render(null(1, -1, some), *view, 4, *tail) == _C.TRI_ERR_ARG
    assert lib.tri_raster_render(null(1, 0, some), None, 200, 3, 8, 8, 4.0, R.ZNEAR, 1, *tail) != 0           # yfov beyond pi
    for samples in (1, 4):
        assert lib.tri_raster_render(null(0, 0, some), None, 0, 3, 8, 8, R.YFOV, R.ZNEAR, samples, *tail) == 0     # nothing to draw
    assert lib.tri_mesh_vertex_normals_workspace(10) == 240 and lib.tri_mesh_vertex_normals_workspace(0) == 0 and lib.tri_mesh_vertex_normals_workspace(-5) == 0
    one, three = _C.TriMeshBatch(N=1), _C.TriMeshBatch(N=3)                                                   # null arrays, no optional group
    assert lib.tri_mesh_vertex_normals(one, -1, 5, 0, None, None, None, None) == _C.TRI_ERR_ARG
    assert lib.tri_mesh_vertex_normals(one, 5, 5, 2, None, None, None, None) == _C.TRI_ERR_ARG               # fill
    assert lib.tri_mesh_vertex_normals(one, 5, 5, 0, None, None, None, None) == _C.TRI_ERR_ARG               # faces without arrays
    assert "tri_mesh_vertex_normals" in lib.tri_last_error().decode()
    assert lib.tri_mesh_vertex_normals(one, 5, 2 ** 31, 0, None, None, None, None) == _C.TRI_ERR_UNSUPPORTED
    assert lib.tri_mesh_vertex_normals(three, 5, 0, 1, None, None, None, None) == 0                            # no faces: nothing runs


# ---------------------------------------------------------------------------------------------------- the command line
def test_preprocess_with_smooth_shading_end_to_end_on_the_host(tmp_path):
    """Two models, chairA rewritten with vn lines on its quad (its triangle has none) and tableB without any: --shading smooth writes
    what render_meshes(..., face_vn_list=) gives, changes the images of both against --shading flat, leaves every voxel grid alone
    and counts the faces; the flat run's stats are what they were."""
    runs, stats = {}, {}
    for mode in ("flat", "smooth"):
        root = str(tmp_path / mode)
        overrides = [o for o in tp.write_dataset(root) if not o.startswith("data.ignored_models")]
        overrides.append("data.ignored_models=[04379243/ignoredD,03001627/chairC]")
        obj_root = os.path.join(root, "text2shape-data", "ShapeNetCore.v2")
        with open(os.path.join(obj_root, *tp.MODELS[0], "models", "model_normalized.obj"), "w") as f:
            f.write("mtllib model_normalized.mtl\nv -0.2 -0.1 -0.2\nv 0.2 -0.1 -0.2\nv 0.2 0.1 0.2\nv -0.2 0.1 0.2\nv 0 0.3 0\n"
                    "vn -0.5 1 -0.5\nvn 0.5 1 -0.5\nvn 0.5 0.4 0.5\nvn -0.5 0.4 0.5\n"
                    "usemtl top\nf 1//1 2//2 3//3 4//4\nusemtl side\nf 1 2 5\n")
        stats[mode] = pp.main(overrides + ["--device", "cpu", "--voxels", "mesh", "--shading", mode], log=lambda *a: None)
        cfg = tcfg.compose(overrides=overrides)
        runs[mode] = {m: dict(np.load(os.path.join(cfg.data.exp_data_root_path, c, f"{m}.npz"))) for c, m in tp.MODELS[:2]}
    assert stats["flat"]["train"] == {"models": 2, "written": 2, "skipped": 0}
    assert stats["smooth"]["train"] == {"models": 2, "written": 2, "skipped": 0, "faces_with_vn": 2, "faces_with_computed_normals": 4}
    paths = [os.path.join(obj_root, c, m, "models", "model_normalized.obj") for c, m in tp.MODELS[:2]]
    meshes = [load_obj_materials(p) for p in paths]
    normals = [load_obj_normals(p) for p in paths]
    assert [int(torch.isnan(vn[:, 0, 0]).sum()) for vn in normals] == [1, 3]
    lists = [[m[j] for m in meshes] for j in range(4)]
    want = R.render_meshes(*lists, num_views=int(cfg.data.num_views), face_vn_list=normals)
    filled = MeshBatch.pack(*lists, face_vn_list=normals).with_vertex_normals(fill="missing")
    assert not torch.isnan(filled.face_vn).any() and torch.equal(want, R.render_batch(filled, int(cfg.data.num_views), shading="smooth"))
    for k, (_, m) in enumerate(tp.MODELS[:2]):
        assert runs["smooth"][m]["images"].dtype == np.uint8 and np.array_equal(runs["smooth"][m]["images"], want[k].numpy()), m
        changed = (runs["smooth"][m]["images"] != runs["flat"][m]["images"]).any(1).mean()
        print(f"--shading smooth changes {100 * changed:.1f} % of {m}'s pixels against --shading flat")
        assert changed > 0.005
        for name in ("voxel32", "voxel64", "voxel128"):
            assert np.array_equal(runs["smooth"][m][name], runs["flat"][m][name]), (m, name)
