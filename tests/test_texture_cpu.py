"""CPU: the torch restatements of the textured resolve pass and of the face colours (ops.render_views_textured and
ops.mesh_face_colours on CPU tensors; csrc/raster.hip and csrc/mesh_batch.h define the arithmetic) against the float64 brute force
of tests/texture_reference.py, the identities that tie them to ops.render_views byte for byte, the conventions (v = 0 is the bottom
row; the perspective division), the host validation of MeshBatch.pack and the batch the voxeliser takes.

The scenes are those of tests/test_preprocess.py (one triangle, the soup, the flat quads) with random UVs in [-2, 3] and
random-noise textures of 1 x 1, 2 x 3, 5 x 7 and 16 x 16 texels.  Adding UVs does not change visibility, so the pixels left out
of a comparison (raster_reference's `ambiguous` ones) are the ones those scenes already have, under its 1 % cap.  Colours may
differ from float64 by 1 LSB: the fp32 error of (u, v) is some 1e-6 of a texel, of the blend 1e-7 - three orders below an LSB -
so only a value that falls next to a rounding boundary of floor(255 c + 0.5) moves, and then by one.

check_identities(device) runs here on the host and from tests/test_gpu_texture.py on the GPU."""
import numpy as np
import pytest
import torch

from tests import raster_reference as rr
from tests import test_preprocess as tp
from tests import texture_reference as tr
from tricolo_amd import ops
from tricolo_amd.data import render as R
from tricolo_amd.data import voxelize as VX
from tricolo_amd.meshes import MeshBatch, check_textures

TEXTURE_SIZES = [(1, 1), (2, 3), (5, 7), (16, 16)]                                     # (height, width)
TRIANGLE = torch.tensor([[-0.3, -0.2, 0.0], [0.3, -0.25, 0.1], [0.05, 0.3, -0.1]], dtype=torch.float32)


def noise_textures(seed=21, sizes=TEXTURE_SIZES):
    g = np.random.default_rng(seed)
    return [np.concatenate([g.integers(0, 256, (h, w, 3), dtype=np.uint8), np.full((h, w, 1), 255, np.uint8)], 2) for h, w in sizes]


def random_uv(n, seed):
    return torch.from_numpy(np.random.default_rng(seed).uniform(-2.0, 3.0, (n, 3, 2)).astype(np.float32))


def scene(name, shift=0):
    """-> dict(verts, faces, fm, kd, uv, mt, texs, cam [views, 12], H, W, yfov): one mesh; material j takes texture (j + shift) % 4."""
    g = np.random.default_rng(3)
    yfov = R.YFOV
    if name == "triangle":
        verts, faces, H, W, views = TRIANGLE, torch.tensor([[0, 1, 2]]), 16, 16, 1
        fm, kd = torch.zeros(1, dtype=torch.int32), torch.tensor([[0.9, 0.6, 0.8]])
    elif name == "soup":
        verts, faces = rr.soup()
        H, W, views = 32, 48, 3
        fm = torch.from_numpy(g.integers(0, 3, faces.shape[0]).astype(np.int32))
        kd = torch.from_numpy(g.uniform(0, 1, (3, 3)).astype(np.float32))
    else:                                                                              # the three quads of test_preprocess, two faces each
        pts = [p for q in tp.QUADS.values() for p in q]
        verts, H, W, views, yfov = tp.flat_vertices(pts, 16, 16), 16, 16, 1, tp.FLAT_YFOV
        verts[:, 2] = torch.from_numpy(g.uniform(-0.5, 0.2, len(pts)).astype(np.float32))  # at different depths: perspective matters
        faces = torch.tensor([[4 * q + a, 4 * q + b, 4 * q + c] for q in range(3) for a, b, c in ((0, 1, 2), (0, 2, 3))])
        fm, kd = torch.tensor([0, 0, 1, 1, 2, 2], dtype=torch.int32), torch.from_numpy(g.uniform(0.3, 1, (3, 3)).astype(np.float32))
    cam = tp.FLAT_CAM[0] if name == "quads" else R.pack_cameras([R.bbox_center(verts)], views)[0]
    mt = torch.tensor([(j + shift) % 4 for j in range(kd.shape[0])], dtype=torch.int32)
    return dict(verts=verts, faces=faces, fm=fm, kd=kd, uv=random_uv(faces.shape[0], 40 + shift), mt=mt, texs=noise_textures(), cam=cam, H=H, W=W,
                yfov=yfov)


def pack(scenes, device="cpu"):
    return MeshBatch.pack([s["verts"] for s in scenes], [s["faces"] for s in scenes], [s["fm"] for s in scenes], [s["kd"] for s in scenes], device,
                          face_uv_list=[s["uv"] for s in scenes], mat_tex_list=[s["mt"] for s in scenes], textures_list=[s["texs"] for s in scenes])


def textured(batch, cam, H, W, yfov=R.YFOV, **fields):
    """(image, vis) of ops.render_views_textured, on the CPU; fields: texture tensors that replace the batch's."""
    tex = dict(zip(("face_uv", "mat_tex", "texels", "tex_off", "tex_size"), batch.texture_tensors))
    tex.update(fields)
    img, vis = ops.render_views_textured(*batch.tensors, *tex.values(), cam.to(batch.verts.device), H, W, yfov, R.ZNEAR, return_visibility=True)
    return img.cpu(), vis.cpu()


def plain(batch, cam, H, W, yfov=R.YFOV, mat_kd=None):
    t = list(batch.tensors)
    if mat_kd is not None:
        t[5] = mat_kd.to(batch.verts.device)
    img, vis = ops.render_views(*t, cam.to(batch.verts.device), H, W, yfov, R.ZNEAR, return_visibility=True)
    return img.cpu(), vis.cpu()


# ---------------------------------------------------------------------------------------------------- against float64
@pytest.mark.parametrize("name,shift", [("triangle", 0), ("triangle", 1), ("triangle", 2), ("triangle", 3), ("soup", 0), ("soup", 2), ("quads", 1),
                                        ("quads", 3)])
def test_restatement_matches_the_float64_brute_force(name, shift):
    s = scene(name, shift)
    if name == "soup":
        s["uv"][5] = float("nan")                                                        # a face without texture coordinates among the others
    img, vis = textured(pack([s]), s["cam"][None], s["H"], s["W"], s["yfov"])
    compared = worst = 0
    for k in range(s["cam"].shape[0]):
        want, face, ambiguous = tr.render(s["verts"], s["faces"], s["fm"], s["kd"], s["uv"], s["mt"], s["texs"], s["cam"][k], s["H"], s["W"], s["yfov"])
        keep = ~ambiguous
        assert np.array_equal(vis[0, k].numpy()[keep], face[keep])
        diff = np.abs(img[0, k].numpy().astype(int) - want.astype(int))[:, keep]
        compared, worst = compared + int((face[keep] >= 0).sum()), max(worst, int(diff.max()))
    print(f"{name}, textures shifted by {shift}: {compared} covered pixels compared, largest colour difference {worst}")
    assert compared > (100 if name == "soup" else 20) and worst <= 1


# ---------------------------------------------------------------------------------------------------- identities, byte for byte
def check_identities(device="cpu"):
    soup, tri = scene("soup", 1), scene("triangle", 3)
    tri["cam"] = R.pack_cameras([R.bbox_center(tri["verts"])], 3)[0]
    batch = pack([soup, tri], device)
    cam, H, W = torch.stack([soup["cam"], tri["cam"]]), 32, 48
    base = plain(batch, cam, H, W)
    assert (base[1] >= 0).sum() > 100
    # no material has a texture; no face has texture coordinates; no texture in the batch at all
    for what, img in (("mat_tex -1", textured(batch, cam, H, W, mat_tex=torch.full_like(batch.mat_tex, -1))),
                      ("NaN face_uv", textured(batch, cam, H, W, face_uv=torch.full_like(batch.face_uv, float("nan")))),
                      ("T == 0", textured(batch, cam, H, W, mat_tex=torch.full_like(batch.mat_tex, -1), texels=batch.texels[:0].contiguous(),
                                          tex_off=batch.tex_off[:1].contiguous(), tex_size=batch.tex_size[:0].contiguous()))):
        assert torch.equal(img[0], base[0]) and torch.equal(img[1], base[1]), what
    ref = textured(batch, cam, H, W)
    assert not torch.equal(ref[0], base[0])                                              # and with them the picture does change
    # a constant texture of colour c under Kd = 1 is Kd = fl32(c) / 255, at any size and for any UVs
    colour = np.array([200, 17, 255], np.uint8)
    kd = (torch.tensor([200.0, 17.0, 255.0]) / 255.0).expand(batch.mat_kd.shape[0], 3).contiguous()
    want = plain(batch, cam, H, W, mat_kd=kd)
    uv = batch.face_uv.clone()
    uv[0:40] = uv[0:40] * 1e6
    uv[40:80] = -uv[40:80] - 7.25
    for s in soup, tri:
        s["texs"] = [np.broadcast_to(np.concatenate([colour, [255]]).astype(np.uint8), (h, w, 4)).copy() for h, w in TEXTURE_SIZES]
        s["kd"] = torch.ones_like(s["kd"])
    const = pack([soup, tri], device)
    got = textured(const, cam, H, W, face_uv=uv.to(device))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), "constant texture"
    # the winding of a face, its UVs permuted alike; the order of the faces, their UVs and materials with them
    soup, tri = scene("soup", 1), scene("triangle", 3)
    flip = torch.arange(soup["faces"].shape[0]) % 2 == 0
    order = torch.where(flip[:, None], torch.tensor([0, 2, 1]), torch.tensor([0, 1, 2]))
    soup["faces"], soup["uv"] = soup["faces"].gather(1, order), soup["uv"].gather(1, order[:, :, None].expand(-1, 3, 2))
    got = textured(pack([soup, tri], device), cam, H, W)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), "winding"
    soup = scene("soup", 1)
    perm = torch.from_numpy(np.random.default_rng(8).permutation(soup["faces"].shape[0]))
    for key in ("faces", "uv", "fm"):
        soup[key] = soup[key][perm]
    got = textured(pack([soup, tri], device), cam, H, W)
    assert torch.equal(got[0], ref[0]), "face order"
    vis = got[1][0].to(torch.int64)
    assert torch.equal(torch.where(vis >= 0, perm[vis.clamp(min=0)], vis), ref[1][0].to(torch.int64)), "face order"


def test_identities():
    check_identities()


# ---------------------------------------------------------------------------------------------------- conventions
def slanted_quad():
    """A quad from 0.25 to 1.6 in front of the eye, a 2 x 2 checker across it: perspective and affine UVs differ by texels."""
    verts = torch.tensor([[-0.25, -0.2, 0.55], [0.25, -0.2, 0.55], [0.9, 0.1, -0.8], [-0.9, 0.1, -0.8]], dtype=torch.float32)
    uv = torch.tensor([[[0, 0], [1, 0], [1, 1]], [[0, 0], [1, 1], [0, 1]]], dtype=torch.float32)
    checker = np.array([[[255, 255, 255, 255], [0, 0, 0, 255]], [[0, 0, 0, 255], [255, 255, 255, 255]]], np.uint8)
    cam = torch.tensor([0.0, 0.0, 0.85, 1, 0, 0, 0, 1, 0, 0, 0, 1], dtype=torch.float32)
    return dict(verts=verts, faces=torch.tensor([[0, 1, 2], [0, 2, 3]]), fm=torch.zeros(2, dtype=torch.int32), kd=torch.ones(1, 3), uv=uv,
                mt=torch.zeros(1, dtype=torch.int32), texs=[checker], cam=cam[None], H=24, W=24, yfov=R.YFOV)


def test_the_perspective_division_is_visible():
    s = slanted_quad()
    img, vis = textured(pack([s]), s["cam"][None], s["H"], s["W"])
    args = (s["verts"], s["faces"], s["fm"], s["kd"], s["uv"], s["mt"], s["texs"], s["cam"][0], s["H"], s["W"])
    right, face, ambiguous = tr.render(*args)
    wrong = tr.render(*args, affine=True)[0]
    keep = ~ambiguous & (face >= 0)
    assert keep.sum() > 50
    got = img[0, 0].numpy().astype(int)
    assert np.abs(got - right.astype(int))[:, keep].max() <= 1
    far = (np.abs(got - wrong.astype(int)).max(0) > 1) & keep
    print(f"slanted quad: {int(far.sum())} of {int(keep.sum())} pixels differ from screen-affine UVs by more than 1 LSB")
    assert far.sum() >= 1


CORNERS = np.array([[[10, 20, 30, 255], [40, 50, 60, 255]], [[70, 80, 90, 255], [100, 110, 120, 255]]], np.uint8)   # [row][column]
CENTRES = [((0.25, 0.25), (1, 0)), ((0.75, 0.25), (1, 1)), ((0.25, 0.75), (0, 0)), ((0.75, 0.75), (0, 1))]            # (u, v) -> (row, column)


def corner_scene():
    """Four copies of the triangle, side by side; all three corners of copy i carry the i-th texel centre as their UV."""
    verts = torch.cat([TRIANGLE * 0.3 + torch.tensor([0.25 * i - 0.375, 0.0, 0.0]) for i in range(4)])
    uv = torch.tensor([[list(c)] * 3 for c, _ in CENTRES], dtype=torch.float32)
    s = dict(verts=verts, faces=torch.arange(12).reshape(4, 3), fm=torch.zeros(4, dtype=torch.int32), kd=torch.ones(1, 3), uv=uv,
             mt=torch.zeros(1, dtype=torch.int32), texs=[CORNERS])
    s["cam"] = R.pack_cameras([R.bbox_center(verts)], 1)[0]
    return s


def test_v_is_zero_at_the_bottom_row():
    """(0.25, 0.25) is the bottom-left texel: row 1, column 0.  Each texel centre returns its texel exactly."""
    s = corner_scene()
    batch = pack([s])
    want = torch.stack([torch.from_numpy(CORNERS[r, c, :3].astype(np.float32)) / 255.0 for _, (r, c) in CENTRES])
    ok, got = R.sample_textures(torch.zeros(4, dtype=torch.int64), s["uv"][:, 0, 0], s["uv"][:, 0, 1], batch.texels, batch.tex_off, batch.tex_size)
    assert ok.all() and torch.equal(got, want)
    assert torch.equal(ops.mesh_face_colours(batch), want)
    # and in a rendering: every copy is the plain rendering with its texel as Kd
    per_face = MeshBatch.pack([s["verts"]], [s["faces"]], [torch.arange(4, dtype=torch.int32)], [want])
    img, vis = textured(batch, s["cam"][None], 24, 48)
    base = plain(per_face, s["cam"][None], 24, 48)
    assert set(vis.unique().tolist()) == {-1, 0, 1, 2, 3}
    assert torch.equal(img, base[0]) and torch.equal(vis, base[1])


# ---------------------------------------------------------------------------------------------------- face colours, the voxeliser's batch
def test_face_colours():
    g = np.random.default_rng(17)
    s = scene("soup", 0)
    s["kd"] = torch.cat([s["kd"], torch.tensor([[0.2, 0.5, 0.7]])])
    s["mt"] = torch.tensor([0, 2, 3, -1], dtype=torch.int32)
    s["fm"][100:150] = 3                                                                 # untextured by their material
    s["uv"][20:30] = float("nan")                                                        # untextured by the marker
    s["uv"][30:33, 1, 0] = float("inf")                                                  # a sample that is not finite
    colour = np.array([9, 130, 251, 255], np.uint8)
    s["texs"][0] = np.broadcast_to(colour, (1, 1, 4)).copy()                             # material 0: a constant texture
    cell = torch.from_numpy(g.uniform(0.0, 1.0, (40, 3, 2)).astype(np.float32))          # material 2 (16 x 16): inside one cell of four texel centres
    ij = torch.from_numpy(g.integers(0, 15, (40, 1, 2)).astype(np.float32))
    s["uv"][160:200] = (ij + 0.5 + cell) / 16.0
    s["fm"][160:200] = 2
    batch = pack([s])
    got = ops.mesh_face_colours(batch)
    assert got.shape == (200, 3) and got.dtype == torch.float32
    kd = s["kd"][s["fm"].long()]
    plain_faces = (s["fm"] == 3) | torch.isnan(s["uv"][:, 0, 0]) | torch.isinf(s["uv"][:, 1, 0])
    assert torch.equal(got[plain_faces], kd[plain_faces]) and int(plain_faces.sum()) >= 63
    const = (s["fm"] == 0) & ~plain_faces
    assert const.sum() > 20 and torch.equal(got[const], kd[const] * (torch.tensor([9.0, 130.0, 251.0]) / 255.0))
    keep = ~torch.isinf(s["uv"][:, 1, 0])
    s["uv"][30:33, 1, 0] = 0.0
    want = tr.face_colours(s["fm"], s["kd"], s["uv"], s["mt"], s["texs"])
    err = np.abs(got.numpy().astype(np.float64) - want)[keep.numpy()]
    print(f"face colours against float64: largest difference {err.max():.2e} over all faces, {err[160:].max():.2e} inside one texel cell")
    assert err[160:].max() <= 1e-6


def test_with_face_colours_feeds_the_voxeliser():
    s = scene("soup", 0)
    batch = pack([s, scene("triangle", 1)])
    kd_faces = torch.cat([s["kd"][s["fm"].long()], torch.tensor([[0.9, 0.6, 0.8]])])
    solid = batch.with_face_colours(kd_faces)
    assert solid.texture_tensors == (None,) * 5 and torch.equal(solid.mat_off, batch.face_off) and solid.max_faces == batch.max_faces
    assert solid.face_mat.dtype == torch.int32 and solid.face_mat.tolist() == list(range(200)) + [0]
    frame = VX.box_frames(batch.boxes, 32)
    a = ops.voxelize_meshes(*batch.tensors, frame, 32, return_labels=True)
    b = ops.voxelize_meshes(*solid.tensors, frame, 32, return_labels=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and int((a[0][:, 3] > 0).sum()) > 50
    with pytest.raises(ValueError, match="colours"):
        batch.with_face_colours(kd_faces[:5])


# ---------------------------------------------------------------------------------------------------- validation on the host
def test_pack_validates_textures():
    s = scene("triangle", 0)
    batch = pack([s])
    assert batch.tex_off.tolist() == [0, 1, 7, 42, 298] and batch.tex_size.tolist() == [[1, 1], [2, 3], [5, 7], [16, 16]]
    assert batch.texels.shape == (298, 4) and batch.texels.dtype == torch.uint8 and batch.face_uv.shape == (1, 3, 2)
    assert MeshBatch.pack([s["verts"]], [s["faces"]], [s["fm"]], [s["kd"]]).texture_tensors == (None,) * 5
    two = pack([s, scene("triangle", 2)])
    assert two.mat_tex.tolist() == [0, 6] and two.tex_off[-1] == 596                     # the second mesh's indices become batch-global
    for key, bad, match in (("mt", torch.tensor([4], dtype=torch.int32), "texture indices"), ("mt", torch.tensor([-2], dtype=torch.int32), "texture indices"),
                            ("mt", torch.tensor([0, 1], dtype=torch.int32), "mat_tex"), ("uv", torch.zeros(2, 3, 2), "face_uv"),
                            ("uv", torch.zeros(1, 3, 2, dtype=torch.float64), "face_uv"), ("texs", [np.zeros((0, 3, 4), np.uint8)], "texture 0"),
                            ("texs", [np.zeros((2, 2, 3), np.uint8)], "texture 0")):
        with pytest.raises(ValueError, match=match):
            pack([dict(s, **{key: bad})])
    with pytest.raises(ValueError, match="textures need"):
        MeshBatch.pack([s["verts"]], [s["faces"]], [s["fm"]], [s["kd"]], face_uv_list=[s["uv"]])
    f = list(batch.texture_tensors)
    check_textures(*f, 1, 1)
    for k, bad, match in ((3, torch.tensor([0, 1, 7, 42, 297]), "tex_off"), (4, torch.tensor([[1, 1], [2, 3], [5, 7], [16, 0]], dtype=torch.int32), "H, W"),
                          (1, torch.tensor([4], dtype=torch.int32), "mat_tex"), (2, batch.texels[:, :3], "texels")):
        with pytest.raises(ValueError, match=match):
            check_textures(*(f[:k] + [bad] + f[k + 1:]), 1, 1)
    plain_batch = MeshBatch.pack([s["verts"]], [s["faces"]], [s["fm"]], [s["kd"]])
    with pytest.raises(ValueError, match="packed without textures"):
        ops.mesh_face_colours(plain_batch)
    with pytest.raises(ValueError, match="packed without textures"):
        R.render_batch(plain_batch, 1, 8, textures=True)
    with pytest.raises(ValueError, match="mat_tex"):
        textured(batch, s["cam"][None], 8, 8, mat_tex=torch.zeros(3, dtype=torch.int32))
