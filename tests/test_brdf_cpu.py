"""CPU: the glTF metallic-roughness BRDF - brdf= of ops.render_views and ops.render_views_textured on CPU tensors, the torch
restatement of the BRDF resolve kernels of csrc/raster.hip - against the float64 statement of tests/brdf_reference.py and against
closed forms; the identities that tie the switch to the existing calls byte for byte; the clamps of the two factors at bit level;
the fallback to the Lambert colour where the half vector has no length; independence of the face order; batching; the refusals; the
`Ns` parser; and python -m tricolo_amd.data.preprocess --brdf gltf end to end on the host.

The scenes are those of tests/test_normals_cpu.py at their sizes, the materials (m, r) = (1, 0.378), (0, 0.9), (0.5, 0.2) and the
mesh without materials, (0.2, 0.8) on grey 0.4.  The BRDF does not change visibility, so the positions left out of a comparison are
the visibility's `ambiguous` ones plus those brdf_reference adds (the sign of n . e, a vanishing normal, a half vector shorter than
1e-3), together under the 1 % cap.  Colours may differ from float64 by 1 LSB, the allowance of tests/test_normals_cpu.py: the BRDF
with its clamps is continuous, its only cancellation is t = NH^2 (a2 - 1) + 1, whose fp32 error relative to t is about 1e-7 / a2 <=
6e-5 for r >= 0.2 - and where t is that small the colour is clamped to 1 anyway - so only a value next to a rounding boundary of
floor(255 c + 0.5) moves, and then by one.

The check_* functions run here on the host and from tests/test_gpu_brdf.py on the GPU."""
import math
import os

import numpy as np
import pytest
import torch

from tests import brdf_reference as br
from tests import raster_reference as rr
from tests import test_normals_cpu as tn
from tests import test_preprocess as tp
from tests.test_gpu_mip import three_meshes
from tricolo_amd import _C, ops
from tricolo_amd import config as tcfg
from tricolo_amd.data import materials
from tricolo_amd.data import preprocess as pp
from tricolo_amd.data import render as R
from tricolo_amd.meshes import MeshBatch

MODES = tn.MODES
PAIRS = ((1.0, 0.378), (0.0, 0.9), (0.5, 0.2))
NAN = float("nan")


def pbr_of(s, start=0):
    """fp32 [M, 2] for the materials of scene s: PAIRS in turn, from PAIRS[start]."""
    return torch.tensor([PAIRS[(start + j) % 3] for j in range(s["kd"].shape[0])], dtype=torch.float32)


def pack(scenes, device="cpu", start=0):
    return MeshBatch.pack([s["verts"] for s in scenes], [s["faces"] for s in scenes], [s["fm"] for s in scenes], [s["kd"] for s in scenes], device,
                          face_uv_list=[s["uv"] for s in scenes], mat_tex_list=[s["mt"] for s in scenes], textures_list=[s["texs"] for s in scenes],
                          face_vn_list=[s["vn"] for s in scenes],
                          pbr_list=[s.get("pbr", pbr_of(s, start + k)) for k, s in enumerate(scenes)]).with_texture_mips()


def render(batch, cam, H, W, yfov=R.YFOV, mode="plain", samples=1, smooth=False, brdf="batch", **kw):
    """(image, vis) on the CPU of the call `mode` names; brdf: "batch" (the batch's mat_pbr), None (the keyword is passed as None), or a tensor."""
    kw["brdf"] = batch.mat_pbr if isinstance(brdf, str) else brdf
    if smooth:
        kw["normals"] = batch.face_vn
    cam = cam.to(batch.verts.device)
    if mode == "plain":
        out = ops.render_views(*batch.tensors, cam, H, W, yfov, R.ZNEAR, return_visibility=True, samples=samples, **kw)
    else:
        out = ops.render_views_textured(*batch.tensors, *batch.texture_tensors, cam, H, W, yfov, R.ZNEAR, return_visibility=True, samples=samples,
                                        mips=batch.mip_tensors if mode == "mip" else None, **kw)
    return out[0].cpu(), out[1].cpu()


# ---------------------------------------------------------------------------------------------------- against float64
def against_reference(s, img, vis, pbr, mode, samples, smooth, what, kd=None, fm=None):
    compared = left_out = covered = worst = 0
    for k in range(s["cam"].shape[0]):
        want, face, ambiguous = br.render(s["verts"], s["faces"], s["fm"] if fm is None else fm, s["kd"] if kd is None else kd, pbr, s["cam"][k],
                                          s["H"], s["W"], s["yfov"], samples=samples, face_vn=s["vn"] if smooth else None,
                                          textures=None if mode == "plain" else (s["uv"], s["mt"], s["texs"]), mip=mode == "mip")
        keep = ~ambiguous
        assert np.array_equal(vis[k].numpy()[keep], face[keep]), what
        clean = keep if samples == 1 else keep.all(-1)                                   # a pixel is compared when none of its samples is ambiguous
        diff = np.abs(img[k].numpy().astype(int) - want.astype(int))[:, clean]
        compared, worst = compared + int((face[keep] >= 0).sum()), max(worst, int(diff.max()))
        left_out, covered = left_out + int((ambiguous & (face >= 0)).sum()), covered + int((face >= 0).sum())
    print(f"{what}: {compared} covered positions compared, {left_out} of {covered} left out, largest colour difference {worst}")
    assert left_out <= rr.MAX_AMBIGUOUS * covered, "the scene leaves too many positions out - change the scene"
    assert worst <= 1, what
    return compared


@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["triangle", "soup", "quads", "sphere"])
def test_restatement_matches_the_float64_reference(name, mode, smooth):
    s = tn.scene(name)
    start = (MODES.index(mode) + int(smooth)) % 3                                        # the one-material scenes meet every pair over the modes
    batch = pack([s], start=start)
    img, vis = render(batch, s["cam"][None], s["H"], s["W"], s["yfov"], mode, 1, smooth)
    compared = against_reference(s, img[0], vis[0], pbr_of(s, start), mode, 1, smooth, f"{name}, {mode}, {'smooth' if smooth else 'flat'}")
    assert compared > (100 if name in ("soup", "sphere") else 20)


@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["sphere", "quads"])
def test_restatement_matches_the_float64_reference_with_four_samples(name, mode, smooth):
    s = tn.scene(name)
    start = (1 + MODES.index(mode) + int(smooth)) % 3
    batch = pack([s], start=start)
    img, vis = render(batch, s["cam"][None], s["H"], s["W"], s["yfov"], mode, 4, smooth)
    compared = against_reference(s, img[0], vis[0], pbr_of(s, start), mode, 4, smooth, f"{name}, {mode}, {'smooth' if smooth else 'flat'}, 4 samples")
    assert compared > 80


def without_materials(s, device="cpu"):
    """The tensors of scene s as a batch whose mat_off gives it no materials, with the empty mat_kd and mat_pbr."""
    batch = pack([s], device)
    t = list(batch.tensors)
    t[5], t[6] = torch.zeros((0, 3), device=device), torch.zeros(2, dtype=torch.int64, device=device)
    return batch, t, torch.zeros((0, 2), device=device)


@pytest.mark.parametrize("smooth", [False, True])
def test_a_mesh_without_materials_against_the_float64_reference(smooth):
    s = tn.scene("sphere")
    batch, t, pbr = without_materials(s)
    img, vis = ops.render_views(*t, s["cam"][None], s["H"], s["W"], s["yfov"], R.ZNEAR, return_visibility=True, brdf=pbr,
                                normals=batch.face_vn if smooth else None)
    against_reference(s, img[0], vis[0], pbr, "plain", 1, smooth, f"sphere without materials, {'smooth' if smooth else 'flat'}", kd=t[5])


# ---------------------------------------------------------------------------------------------------- closed forms
def section_one(base, m, r, NL, NV, NH, VH):
    """The colour of section 1 of the definition in plain math, from the four clamped cosines."""
    a2 = r ** 4
    F0, cdiff = 0.04 + (base - 0.04) * m, 0.96 * base * (1.0 - m)
    F = F0 + (1.0 - F0) * (1.0 - VH) ** 5

    def g(x):
        return 2.0 * x / (x + math.sqrt(a2 + (1.0 - a2) * x * x))

    D = a2 / (math.pi * (NH * NH * (a2 - 1.0) + 1.0) ** 2)
    return min(max(0.1 * base + 3.0 * NL * ((1.0 - F) * cdiff / math.pi + F * g(NL) * g(NV) * D / (4.0 * NL * NV)), 0.0), 1.0)


def quad_scene(corners, kd=0.5, size=33):
    """One quad (two faces) of one grey material, seen from view 0 of pack_cameras at size x size: the centre pixel's centre is the
    principal point, which looks at the centre of the quad's bounding box."""
    verts = torch.tensor(corners, dtype=torch.float32)
    faces = torch.tensor([[0, 1, 2], [0, 2, 3]])
    return dict(verts=verts, faces=faces, fm=torch.zeros(2, dtype=torch.int32), kd=torch.full((1, 3), kd), cam=R.pack_cameras([R.bbox_center(verts)], 1)[0],
                H=size, W=size)


def check_closed_forms(device="cpu"):
    r = materials.ns_to_roughness(10.0)
    pbr = torch.tensor([[1.0, r]], device=device)
    e = math.pi / 5
    v = (0.0, math.sin(e), math.cos(e))
    hl = math.sqrt(v[0] ** 2 + (1.0 + v[1]) ** 2 + v[2] ** 2)
    h = (0.0, (1.0 + v[1]) / hl, v[2] / hl)
    VH = v[1] * h[1] + v[2] * h[2]
    # a horizontal quad through its bounding-box centre: n = l = (0, 1, 0) at the centre pixel
    s = quad_scene([[-0.3, 0.0, -0.3], [0.3, 0.0, -0.3], [0.3, 0.0, 0.3], [-0.3, 0.0, 0.3]])
    batch = MeshBatch.pack([s["verts"]], [s["faces"]], [s["fm"]], [s["kd"]], device)
    img = ops.render_views(*batch.tensors, s["cam"][None].to(device), 33, 33, brdf=pbr).cpu()
    want = math.floor(255.0 * section_one(0.5, 1.0, r, 1.0, v[1], h[1], VH) + 0.5)
    print(f"horizontal quad, m = 1, r = {r:.4f}: centre pixel {img[0, 0, :, 16, 16].tolist()}, closed form {want}")
    assert all(abs(int(c) - want) <= 1 for c in img[0, 0, :, 16, 16]) and want > math.floor(255.0 * 0.05 + 0.5) + 10
    # a vertical wall, n = (0, 0, 1): n . l = 0, so NL takes its clamp 0.001 and a metal keeps the ambient tenth of its colour
    s = quad_scene([[-0.3, -0.3, 0.0], [0.3, -0.3, 0.0], [0.3, 0.3, 0.0], [-0.3, 0.3, 0.0]])
    batch = MeshBatch.pack([s["verts"]], [s["faces"]], [s["fm"]], [s["kd"]], device)
    img = ops.render_views(*batch.tensors, s["cam"][None].to(device), 33, 33, brdf=pbr).cpu()
    full = section_one(0.5, 1.0, r, 0.001, v[2], h[2], VH)
    want, ambient = math.floor(255.0 * full + 0.5), math.floor(255.0 * 0.05 + 0.5)
    print(f"vertical wall: centre pixel {img[0, 0, :, 16, 16].tolist()}, closed form {want} = u8(0.1 Kd) {ambient} plus {255.0 * (full - 0.05):.4f} LSB")
    assert all(abs(int(c) - want) <= 1 for c in img[0, 0, :, 16, 16]) and abs(want - ambient) <= 1
    covered = img[0, 0, 0] != 255
    assert covered.sum() > 100 and int(img[0, 0, 0][covered].max()) <= ambient + 1       # the whole wall is dark: no diffuse term under m = 1


def test_closed_forms():
    check_closed_forms()


# ---------------------------------------------------------------------------------------------------- identities, byte for byte
def check_identities(device="cpu"):
    soup, tri = tn.scene("soup"), tn.scene("triangle")
    tri["cam"] = R.pack_cameras([R.bbox_center(tri["verts"])], 3)[0]
    batch = pack([soup, tri], device)
    cam, H, W = torch.stack([soup["cam"], tri["cam"]]), 32, 48
    for mode in MODES:
        for samples in (1, 4):
            for smooth in (False, True):
                what = f"{mode}, {samples} sample(s), {'smooth' if smooth else 'flat'}"
                kw = dict(normals=batch.face_vn) if smooth else {}
                base = tn.render(batch, cam, H, W, mode=mode, samples=samples, **kw)     # the call without the keyword
                none = render(batch, cam, H, W, mode=mode, samples=samples, smooth=smooth, brdf=None)
                assert torch.equal(none[0], base[0]) and torch.equal(none[1], base[1]), f"brdf=None, {what}"
                got = render(batch, cam, H, W, mode=mode, samples=samples, smooth=smooth)
                assert torch.equal(got[1], base[1]), f"visibility, {what}"
                assert (base[1] >= 0).sum() > 100 and not torch.equal(got[0], base[0]), f"{what}: the picture does change"


def test_identities():
    check_identities()


# ---------------------------------------------------------------------------------------------------- clamps, at bit level
def check_clamps(device="cpu"):
    s = tn.scene("sphere")
    batch = pack([s], device)
    cam = s["cam"][None]

    def image(m, r, smooth=True, samples=1):
        return render(batch, cam, s["H"], s["W"], s["yfov"], "textured", samples, smooth, brdf=torch.tensor([[m, r]], device=device))[0]

    for got, want, what in ((image(0.5, 0.01), image(0.5, 0.04), "r below 0.04"), (image(0.5, -3.0), image(0.5, 0.04), "a negative r"),
                            (image(0.5, 7.0), image(0.5, 1.0), "r above 1"), (image(-0.5, 0.5), image(0.0, 0.5), "m below 0"),
                            (image(1.5, 0.5), image(1.0, 0.5), "m above 1"), (image(NAN, 0.5), image(0.0, 0.5), "m NaN takes 0"),
                            (image(0.5, NAN), image(0.5, 0.04), "r NaN takes 0.04"), (image(float("inf"), float("inf")), image(1.0, 1.0), "inf, inf"),
                            (image(NAN, NAN, False, 4), image(0.0, 0.04, False, 4), "NaN, NaN, flat, 4 samples")):
        assert torch.equal(got, want), what
    assert not torch.equal(image(0.5, 0.04), image(0.5, 0.05)) and not torch.equal(image(0.0, 0.5), image(0.01, 0.5))
    # no materials: (0.2, 0.8) on grey 0.4, whatever mat_pbr would say
    _, t, pbr = without_materials(s, device)
    grey = MeshBatch.pack([s["verts"]], [s["faces"]], [s["fm"]], [torch.full((1, 3), 0.4)], device, pbr_list=[torch.tensor([[0.2, 0.8]])])
    for samples in (1, 4):
        a = ops.render_views(*t, cam.to(device), s["H"], s["W"], s["yfov"], samples=samples, brdf=pbr).cpu()
        b = ops.render_views(*grey.tensors, cam.to(device), s["H"], s["W"], s["yfov"], samples=samples, brdf=grey.mat_pbr).cpu()
        assert torch.equal(a, b) and int(a.min()) < 255, f"no materials, {samples} sample(s)"


def test_clamps():
    check_clamps()


# ---------------------------------------------------------------------------------------------------- degenerate positions
def check_degenerate(device="cpu"):
    """Four faces around a vertex that lies exactly under the principal point of a camera looking straight up, 33 x 33: at the centre
    pixel the weights are (1, 0, 0), p is that vertex, v = (0, -1, 0) = -l and l + v has no length - the Lambert colour, bit for bit.
    The faces look away from the light, so both colours are the ambient tenth of Kd, to which the BRDF adds 0.003 (1 - F) cdiff / pi,
    0.2 LSB at the border of the image; Kd is chosen 0.1 LSB below a rounding boundary, so that the border shows that the BRDF did run.
    Toward the centre VH falls to 0, F rises to 1 and the diffuse term vanishes: the BRDF is continuous there and the fallback cannot
    be told from it by a u8 - what is pinned is that the centre is the Lambert colour and nothing else, whatever 0 / 0 would give."""
    verts = torch.tensor([[0.0, 0.0, 0.0], [-0.3, 0.0, -0.3], [0.3, 0.0, -0.3], [0.3, 0.0, 0.3], [-0.3, 0.0, 0.3]])
    faces = torch.tensor([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1]])
    vn = torch.tensor([[0.3, -1.0, 0.2], [0.0, -1.0, 0.0], [0.4, -1.0, 0.0], [0.0, -1.0, 0.5], [-0.2, -1.0, 0.0]])[faces].contiguous()
    cam = torch.tensor([[[0.0, -0.5, 0.0, 1, 0, 0, 0, 0, 1, 0, -1, 0]]], dtype=torch.float32)
    batch = MeshBatch.pack([verts], [faces], [torch.zeros(4, dtype=torch.int32)], [torch.full((1, 3), 22.4 / 25.5)], device, face_vn_list=[vn],
                           pbr_list=[torch.tensor([[0.0, 0.5]])])
    for normals in (None, batch.face_vn):
        lam, vis = ops.render_views(*batch.tensors, cam.to(device), 33, 33, return_visibility=True, normals=normals)
        got = ops.render_views(*batch.tensors, cam.to(device), 33, 33, normals=normals, brdf=batch.mat_pbr).cpu()
        lam, vis = lam.cpu(), vis.cpu()
        assert int(vis[0, 0, 16, 16]) >= 0 and bool((vis >= 0).all()) and bool((lam == 22).all())  # the faces look away from the light: ambient alone
        assert got[0, 0, :, 16, 16].tolist() == [22, 22, 22]
        assert bool((got[0, 0, :, :4] == 23).all()) and bool((got[0, 0, :, -4:] == 23).all())   # the border takes the BRDF
        assert bool((got[0, 0] >= 22).all()) and bool((got[0, 0] <= 23).all())


def test_a_position_without_a_half_vector_takes_the_lambert_colour():
    check_degenerate()


# ---------------------------------------------------------------------------------------------------- face order, batching
def check_face_order(device="cpu"):
    s = tn.scene("soup")
    s["cam"] = s["cam"][:1]
    perm = torch.from_numpy(np.random.default_rng(5).permutation(s["faces"].shape[0]))
    p = dict(s, faces=s["faces"][perm], fm=s["fm"][perm], uv=s["uv"][perm].contiguous(), vn=s["vn"][perm].contiguous())
    for mode, samples, smooth in (("plain", 1, False), ("mip", 4, True)):
        a = render(pack([s], device), s["cam"][None], 32, 48, mode=mode, samples=samples, smooth=smooth)
        b = render(pack([p], device), s["cam"][None], 32, 48, mode=mode, samples=samples, smooth=smooth)
        inverse = torch.argsort(perm)
        assert torch.equal(torch.where(a[1] >= 0, inverse[a[1].clamp(min=0).long()].to(torch.int32), a[1]), b[1]), "the same faces show"
        assert torch.equal(a[0], b[0]), f"{mode}, {samples} sample(s): the image does not depend on the order of the faces"


def test_independence_of_the_face_order():
    check_face_order()


def brdf_meshes():
    """tests/test_gpu_mip.three_meshes with corner normals (tests/test_gpu_normals.smooth_meshes') and a different (m, r) per material."""
    meshes = three_meshes()
    g = np.random.default_rng(81)
    for k, s in enumerate(meshes):
        s["vn"] = tn.random_normals(s["faces"].shape[0], 70 + k)
        s["pbr"] = torch.from_numpy(np.stack([g.uniform(0.0, 1.0, s["kd"].shape[0]), g.uniform(0.1, 1.0, s["kd"].shape[0])], 1).astype(np.float32))
    meshes[0]["vn"][30] = NAN
    meshes[1]["vn"][:] = NAN
    return meshes


def check_batching(device="cpu", samples_list=(1, 4)):
    meshes = brdf_meshes()
    cam = torch.stack([s["cam"] for s in meshes])
    batch, singles = pack(meshes, device), [pack([s], device) for s in meshes]
    assert batch.mat_pbr.shape == (7, 2) and torch.equal(batch.mat_pbr.cpu(), torch.cat([s["pbr"] for s in meshes]))
    for samples in samples_list:
        for mode, smooth in (("plain", False), ("textured", True), ("mip", True)):
            got = render(batch, cam, 32, 48, mode=mode, samples=samples, smooth=smooth)
            for n, s in enumerate(meshes):
                alone = render(singles[n], s["cam"][None], 32, 48, mode=mode, samples=samples, smooth=smooth)
                assert torch.equal(alone[0][0], got[0][n]) and torch.equal(alone[1][0], got[1][n]), f"mesh {n} alone, {mode}, {samples} sample(s)"
                assert (got[1][n] >= 0).any()


def test_batching_with_every_offset_different():
    check_batching()


# ---------------------------------------------------------------------------------------------------- refusals, the batch
def check_refusals(device="cpu"):
    s = tn.scene("triangle")
    batch = pack([s], device)
    cam = s["cam"][None].to(device)
    other = "cpu" if torch.device(device).type == "cuda" else "meta"
    good = batch.mat_pbr
    wide = torch.zeros((1, 4), device=device)[:, ::2]                                   # the right shape, not contiguous
    assert tuple(wide.shape) == (1, 2) and not wide.is_contiguous()
    bad = [good.double(), good.reshape(-1), torch.cat([good, good]), torch.zeros((1, 3), device=device), good.to(other), wide,
           good.cpu().numpy() if device == "cpu" else [[1.0, 0.5]]]
    for brdf in bad:
        with pytest.raises(ValueError):
            ops.render_views(*batch.tensors, cam, 8, 8, brdf=brdf)
        with pytest.raises(ValueError):
            ops.render_views_textured(*batch.tensors, *batch.texture_tensors, cam, 8, 8, brdf=brdf)


def test_refusals_and_the_packed_batch():
    check_refusals()
    s = tn.scene("soup")
    lists = ([s["verts"]], [s["faces"]], [s["fm"]], [s["kd"]])
    pbr = pbr_of(s)
    for bad in (pbr.double(), pbr[:2], pbr[:, :1], pbr.numpy()):
        with pytest.raises(ValueError):
            MeshBatch.pack(*lists, pbr_list=[bad])
    with pytest.raises(ValueError):
        MeshBatch.pack(*lists, pbr_list=[pbr, pbr])
    with pytest.raises(ValueError):
        MeshBatch.pack(lists[0], lists[1], pbr_list=[pbr])                               # no materials to belong to
    with pytest.raises(TypeError):
        MeshBatch.pack(*lists, None, pbr)                                                # keyword only
    plain = MeshBatch.pack(*lists)
    assert plain.mat_pbr is None and plain.pbr_tensor is None and len(plain.tensors) == 7
    with pytest.raises(ValueError):
        R.render_batch(plain, 2, 8, brdf="gltf")
    with pytest.raises(ValueError):
        R.render_batch(plain, 2, 8, brdf="phong")
    packed = pack([s])
    assert packed.pbr_tensor is packed.mat_pbr and torch.equal(packed.mat_pbr, pbr)
    assert packed.with_texture_mips().mat_pbr is packed.mat_pbr and packed.with_vertex_normals().mat_pbr is packed.mat_pbr
    per_face = packed.with_face_colours(ops.mesh_face_colours(packed))
    assert torch.equal(per_face.mat_pbr, pbr[s["fm"].long()]) and per_face.mat_kd.shape[0] == per_face.mat_pbr.shape[0]
    a = R.render_batch(packed, 2, 16, brdf="gltf")
    assert torch.equal(a, ops.render_views(*packed.tensors, R.pack_cameras(R.box_centers(packed.boxes), 2), 16, 16, brdf=packed.mat_pbr))
    assert torch.equal(R.render_batch(packed, 2, 16, brdf="lambert"), R.render_batch(packed, 2, 16)) and not torch.equal(a, R.render_batch(packed, 2, 16))
    b = R.render_meshes(*lists, num_views=2, image_size=16, brdf="gltf", pbr_list=[pbr])
    assert torch.equal(a, b)


def test_the_entry_point_refuses_bad_arguments_before_anything_runs():
    lib = _C.lib()
    tail, some = (None, None, None, None), 64                                                                 # `some`: not null, never read
    TEX, VN, PBR = _C.TRI_MESH_TEXTURES, _C.TRI_MESH_NORMALS, _C.TRI_MESH_PBR

    def null(N, T, mat_pbr, fields=PBR, face_vn=None):                                                        # every other pointer null
        return _C.TriMeshBatch(N=N, T=T, face_vn=face_vn, mat_pbr=mat_pbr, fields=fields)

    view = (None, 200, 3, 8, 8, R.YFOV, R.ZNEAR)
    assert lib.tri_raster_render(null(1, 0, None), *view, 1, *tail) == _C.TRI_ERR_ARG
    assert "mat_pbr" in lib.tri_last_error().decode()
    assert lib.tri_raster_render(null(1, 0, None, VN | PBR, some), *view, 4, *tail) == _C.TRI_ERR_ARG
    assert "mat_pbr" in lib.tri_last_error().decode()
    assert lib.tri_raster_render(null(1, 0, some), *view, 2, *tail) == _C.TRI_ERR_ARG                         # samples
    assert lib.tri_raster_render(null(1, 3, some, TEX | PBR), *view, 1, *tail) == _C.TRI_ERR_ARG             # textures without fields
    assert lib.tri_raster_render(null(1, 0, some), None, 200, 3, 8, 8, 4.0, R.ZNEAR, 1, *tail) != 0           # yfov beyond pi
    for samples in (1, 4):
        assert lib.tri_raster_render(null(0, 0, some), None, 0, 3, 8, 8, R.YFOV, R.ZNEAR, samples, *tail) == 0     # nothing to draw


# ---------------------------------------------------------------------------------------------------- the parser
OBJ = "mtllib a.mtl b.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\nusemtl ten\nf 1 2 3\nusemtl ghost\nf 1 2 3\n"
MTL_A = ("newmtl ten\nKd 0.5 0.5 0.5\nNs 10\nnewmtl zero\nNs 0\nnewmtl none\nKd 1 0 0\nnewmtl garbage\nNs shiny\nnewmtl negative\nNs -4\n"
         "newmtl infinite\nNs inf\nnewmtl nan\nNs nan\nnewmtl bare\nNs\nnewmtl twice\nNs 30\nNs 98\n")
MTL_B = "newmtl ten\nNs 500\nnewmtl late\nNs 6\n"


@pytest.mark.parametrize("newline", ["\n", "\r\n"])
def test_ns_becomes_roughness(tmp_path, newline):
    for name, text in (("m.obj", OBJ), ("a.mtl", MTL_A), ("b.mtl", MTL_B)):
        (tmp_path / name).write_bytes(text.replace("\n", newline).encode())
    path = str(tmp_path / "m.obj")
    before = materials.load_obj_materials(path)
    pbr = materials.load_obj_pbr(path)
    names = before[4]
    assert names == [None, "ten", "zero", "none", "garbage", "negative", "infinite", "nan", "bare", "twice", "late"]
    assert pbr.dtype == torch.float32 and tuple(pbr.shape) == (len(names), 2)

    def rough(ns):
        return float(np.float32((2.0 / (ns + 2.0)) ** 0.25))

    assert pbr[0].tolist() == [float(np.float32(0.2)), float(np.float32(0.8))]           # material 0, the default grey
    assert pbr[1:, 0].tolist() == [1.0] * (len(names) - 1)
    want = {"ten": rough(10.0), "zero": 1.0, "none": rough(1.0), "garbage": rough(1.0), "negative": rough(1.0), "infinite": rough(1.0),
            "nan": rough(1.0), "bare": rough(1.0), "twice": rough(98.0), "late": rough(6.0)}
    for name, r in want.items():
        assert abs(float(pbr[names.index(name), 1]) - r) <= 6e-8 * r, name               # two square roots against one power: an ulp of fp32 at the most
    assert float(pbr[1, 1]) == float(np.float32(math.sqrt(math.sqrt(2.0 / 12.0)))) and float(pbr[2, 1]) == 1.0
    assert materials.load_obj_pbr(path, metallic=0.25)[1:, 0].tolist() == [0.25] * (len(names) - 1)
    assert materials.load_obj_pbr(path, metallic=0.25)[0].tolist() == pbr[0].tolist()
    after = materials.load_obj_materials(path)                                           # the existing loaders give what they gave
    assert all(torch.equal(a, b) for a, b in zip(before[:4], after[:4])) and after[4] == names and len(after) == 5
    assert materials.load_mtl(str(tmp_path / "a.mtl"))["ten"] == (0.5, 0.5, 0.5) and len(materials.load_obj_textured(path)) == 9
    os.remove(tmp_path / "a.mtl")
    os.remove(tmp_path / "b.mtl")
    assert materials.load_obj_pbr(path).tolist() == [pbr[0].tolist()]                    # no MTL file: material 0 alone


# ---------------------------------------------------------------------------------------------------- the command line
def test_preprocess_with_the_gltf_brdf_end_to_end_on_the_host(tmp_path):
    """One model, with an Ns on one of its two materials: --brdf gltf writes what render_meshes(..., brdf="gltf", pbr_list=) gives, in
    the same keys and shapes; no switch and --brdf lambert write the same bytes; --metallic 0 differs from the default."""
    assert pp.BRDF_MODES == ("lambert", "gltf") and "[--brdf lambert|gltf]" in pp.__doc__ and "[--shading flat|smooth]" in pp.__doc__
    with pytest.raises(SystemExit):
        pp.main(["--brdf", "phong"], log=lambda *a: None)
    runs, files = {}, {}
    for what, switches in (("none", []), ("lambert", ["--brdf", "lambert"]), ("gltf", ["--brdf", "gltf"]), ("diffuse", ["--brdf", "gltf", "--metallic", "0"])):
        root = str(tmp_path / what)
        overrides = [o for o in tp.write_dataset(root) if not o.startswith("data.ignored_models")]
        overrides.append("data.ignored_models=[04379243/ignoredD,03001627/chairC,04379243/tableB]")
        obj_root = os.path.join(root, "text2shape-data", "ShapeNetCore.v2")
        with open(os.path.join(obj_root, *tp.MODELS[0], "models", "model_normalized.mtl"), "a") as f:
            f.write("Ns 40\n")                                                           # the last material, `side`
        stats = pp.main(overrides + ["--device", "cpu"] + switches, log=lambda *a: None)
        assert stats["train"] == {"models": 1, "written": 1, "skipped": 0}
        cfg = tcfg.compose(overrides=overrides)
        path = os.path.join(cfg.data.exp_data_root_path, tp.MODELS[0][0], f"{tp.MODELS[0][1]}.npz")
        runs[what], files[what] = dict(np.load(path)), open(path, "rb").read()
    assert files["none"] == files["lambert"]
    for what in ("gltf", "diffuse"):
        assert sorted(runs[what]) == sorted(runs["none"]) and all(runs[what][k].shape == runs["none"][k].shape and runs[what][k].dtype == runs["none"][k].dtype
                                                                for k in runs["none"])
        for name in ("voxel32", "voxel64", "voxel128"):
            assert np.array_equal(runs[what][name], runs["none"][name])
    obj = os.path.join(obj_root, *tp.MODELS[0], "models", "model_normalized.obj")
    mesh, pbr = materials.load_obj_materials(obj), materials.load_obj_pbr(obj)
    assert pbr[1:].tolist() == [[1.0, materials.ns_to_roughness(1.0)], [1.0, materials.ns_to_roughness(40.0)]]
    want = R.render_meshes(*[[m] for m in mesh[:4]], num_views=int(cfg.data.num_views), brdf="gltf", pbr_list=[pbr])
    assert np.array_equal(runs["gltf"]["images"], want[0].numpy())
    changed = (runs["gltf"]["images"] != runs["none"]["images"]).any(1)
    drawn = (runs["none"]["images"] != 255).any(1)
    print(f"--brdf gltf changes {100 * changed.mean():.1f} % of the pixels, {100 * changed[drawn].mean():.1f} % of the drawn ones, against the Lambert run")
    assert changed[drawn].mean() > 0.5 and not changed[~drawn].any()
    assert not np.array_equal(runs["diffuse"]["images"], runs["gltf"]["images"])
