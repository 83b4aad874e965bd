"""CPU: the four-sample mode of the renderer (ops.render_views / ops.render_views_textured with samples=4 on CPU tensors, the torch
restatement of csrc/raster.hip's four-sample kernels): samples=1 is the call without the keyword, byte for byte; the visibility of
every sample against the float64 brute force of tests/antialias_reference.py; the resolve rule (the pixel is the rounded integer
mean of its four sample colours, a textured sample taking (u, v) at its own position); exact coverage of hand-made screen-space
cases at the sample positions; the refusals; and python -m tricolo_amd.data.preprocess --antialias 4x end to end on the host.

The brute-force scenes, run with the brute force alone: 0 ambiguous of 690, 1,007 and 21,454 covered samples, and 282 of 309, 161 of
321 and 1,526 of 5,478 touched pixels whose samples disagree - the resolve is exercised, not trivial."""
import os

import numpy as np
import pytest
import torch

from tests import antialias_reference as ar
from tests import raster_reference as rr
from tests import test_preprocess as tp
from tests import test_texture_cpu as tc
from tricolo_amd import _C, ops
from tricolo_amd import config as tcfg
from tricolo_amd.data import preprocess as pp
from tricolo_amd.data import render as R
from tricolo_amd.data.materials import load_obj_materials
from tricolo_amd.evaluation.mesh import pack_meshes

OFFSETS_256 = ((96, 32), (224, 96), (32, 160), (160, 224))                               # the issue's table, in 1/256 pixel


def render(verts, faces, face_mat, kd, cam, H, W, yfov=R.YFOV, znear=R.ZNEAR, device="cpu", **kw):
    """(image, vis) of one mesh under cam [views, 12]; kw: samples, or nothing at all."""
    v, f, voff, foff, _ = pack_meshes([verts], [faces], device)
    fm, k, moff = R.pack_materials([face_mat], [kd], device)
    img, vis = ops.render_views(v, f, voff, foff, fm, k, moff, cam[None].contiguous().to(device), H, W, yfov, znear, return_visibility=True, **kw)
    return img[0].cpu(), vis[0].cpu()


def soup_scene(seed=11, n=200, views=3):
    verts, faces = rr.soup(seed, n)
    g = np.random.default_rng(3)
    fm = torch.from_numpy(g.integers(0, 3, faces.shape[0]).astype(np.int32))
    kd = torch.from_numpy(g.uniform(0, 1, (3, 3)).astype(np.float32))
    return verts, faces, fm, kd, R.pack_cameras([R.bbox_center(verts)], views)[0]


def test_the_positions_are_the_rotated_grid():
    assert R.SAMPLE_OFFSETS == OFFSETS_256 and R.CENTRE == ((128, 128),)
    assert tuple((x / 256, y / 256) for x, y in R.SAMPLE_OFFSETS) == ar.POSITIONS


# ---------------------------------------------------------------------------------------------------- 1. samples=1 changes nothing
def test_one_sample_is_the_call_without_the_keyword():
    scene = soup_scene()
    a, b = render(*scene, 32, 48), render(*scene, 32, 48, samples=1)
    assert a[1].shape == (3, 32, 48) and (a[1] >= 0).sum() > 100
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[1].dtype == b[1].dtype == torch.int32
    s = tc.scene("soup", 1)
    batch = tc.pack([s])
    args = (*batch.tensors, *batch.texture_tensors, s["cam"][None], 32, 48, R.YFOV, R.ZNEAR)
    a, b = ops.render_views_textured(*args, return_visibility=True), ops.render_views_textured(*args, return_visibility=True, samples=1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[0].dtype == torch.uint8 and a[1].dtype == torch.int32
    plain = ops.render_views(*batch.tensors, s["cam"][None], 32, 48, return_visibility=True)
    assert not torch.equal(a[0], plain[0])                                                # the textured scene is textured


# ---------------------------------------------------------------------------------------------------- 2. against the float64 brute force
BRUTE_FORCE = {"soup": (690, 282, 309), "small soup": (1007, 161, 321), "procedural mesh": (21454, 1526, 5478)}    # covered samples, mixed / touched pixels


def brute_force_scenes():
    v, f, fm, kd, cam = soup_scene()
    yield "soup", v, f, fm, kd, cam, 32, 48
    v, f, fm, kd, cam = soup_scene(5, 70, 2)
    yield "small soup", v, f, fm, kd, cam, 32, 48
    v, f, fm, kd = rr.procedural_mesh(12)
    assert f.shape[0] == 324
    yield "procedural mesh", v, f, fm, kd, R.pack_cameras([R.bbox_center(v)], 2)[0], 64, 64


def test_restatement_matches_the_float64_brute_force():
    """Faces equal on every sample whose two nearest depths differ by 1e-5 relative or more; at most 1 % of the covered samples
    are closer than that (asserted by ar.compare; the three scenes have none)."""
    for name, v, f, fm, kd, cam, H, W in brute_force_scenes():
        img, vis = render(v, f, fm, kd, cam, H, W, samples=4)
        assert vis.shape == (cam.shape[0], H, W, 4) and vis.dtype == torch.int32 and img.shape == (cam.shape[0], 3, H, W)
        amb, cov, mixed, touched = ar.compare(vis, v, f, cam, H, W, name)
        assert (cov, mixed, touched) == BRUTE_FORCE[name] and amb == 0, name             # the scenes are the ones the counts were taken on


# ---------------------------------------------------------------------------------------------------- 3. the resolve rule
def mean_of_four(colours):
    """u8 [3, HW, 4] -> u8 [3, HW]: (c0 + c1 + c2 + c3 + 2) >> 2."""
    return ((colours.to(torch.int64).sum(dim=2) + 2) >> 2).to(torch.uint8)


def test_the_pixel_is_the_rounded_mean_of_its_sample_colours():
    for name, v, f, fm, kd, cam, H, W in brute_force_scenes():
        img, vis = render(v, f, fm, kd, cam, H, W, samples=4)
        for k in range(cam.shape[0]):
            planes = [R._shade_one(v, f, fm, kd, cam[k], vis[k, :, :, s].reshape(-1).to(torch.int64)) for s in range(4)]
            want = mean_of_four(torch.stack(planes, dim=2))
            assert torch.equal(img[k].reshape(3, -1), want), f"{name}, view {k}"
        partial = ((vis >= 0).sum(-1) % 4 != 0)
        assert partial.sum() > 20 and (img.permute(0, 2, 3, 1)[partial] != 255).any()     # edge pixels exist and are not background


def sample_texels(s, k, vis, H, W):
    """(has bool [HW 4], c fp32 [HW 4, 3]) for view k of a tests/test_texture_cpu scene by the test's own route: the edge functions
    straight from the sample's position in 1/256 pixel (no centre value, no offsets added), fp32 weights as csrc/raster.hip spells
    them, data.render.sample_textures for the texel."""
    _, X, Y, d, A2, order = R.project_faces(s["verts"], s["faces"], s["cam"][k], H, W, s["yfov"], R.ZNEAR, with_order=True)
    face_t = R.face_textures(s["fm"], s["mt"], s["uv"], len(s["texs"]))
    batch = tc.pack([s])
    has, c = torch.zeros(H * W * 4, dtype=torch.bool), torch.ones((H * W * 4, 3))
    flat = vis.reshape(-1).to(torch.int64)
    for i in torch.nonzero(flat >= 0).reshape(-1).tolist():
        face, pixel, smp = int(flat[i]), i // 4, i % 4
        if face_t[face] < 0:
            continue
        Px, Py = 256 * (pixel % W) + OFFSETS_256[smp][0], 256 * (pixel // W) + OFFSETS_256[smp][1]
        w = []
        for e in range(3):
            a, b = (e + 1) % 3, (e + 2) % 3
            E = (X[face, b] - X[face, a]) * (Py - Y[face, a]) - (Y[face, b] - Y[face, a]) * (Px - X[face, a])
            w.append((E.to(torch.float32) / A2[face].to(torch.float32)) * d[face, e])
        dd = (w[0] + w[1]) + w[2]
        uv = s["uv"][face][order[face]]
        u = ((w[0] / dd) * uv[0, 0] + (w[1] / dd) * uv[1, 0]) + (w[2] / dd) * uv[2, 0]
        t = ((w[0] / dd) * uv[0, 1] + (w[1] / dd) * uv[1, 1]) + (w[2] / dd) * uv[2, 1]
        ok, col = R.sample_textures(face_t[face].reshape(1), u.reshape(1), t.reshape(1), batch.texels, batch.tex_off, batch.tex_size)
        if bool(ok[0]):
            has[i], c[i] = True, col[0]
    return has, c


@pytest.mark.parametrize("name,shift,H,W", [("triangle", 2, 16, 16), ("quads", 3, 16, 16), ("soup", 1, 32, 48)])
def test_a_textured_sample_takes_the_texture_at_its_own_position(name, shift, H, W):
    s = tc.scene(name, shift)
    if name == "soup":
        s["uv"][5] = float("nan")
        s["uv"][7, 2, 1] = float("inf")                                                  # untextured where (u, v) is not finite
        s["cam"] = s["cam"][:1]
    batch = tc.pack([s])
    img, vis = ops.render_views_textured(*batch.tensors, *batch.texture_tensors, s["cam"][None], H, W, s["yfov"], R.ZNEAR, return_visibility=True,
                                         samples=4)
    plain = ops.render_views(*batch.tensors, s["cam"][None], H, W, s["yfov"], R.ZNEAR, return_visibility=True, samples=4)
    assert torch.equal(vis, plain[1]) and not torch.equal(img, plain[0])                  # textures leave visibility alone and change the picture
    differs = 0
    for k in range(s["cam"].shape[0]):
        flat = vis[0, k].reshape(-1).to(torch.int64)
        tex = sample_texels(s, k, vis[0, k], H, W)
        colours = R._shade_one(s["verts"], s["faces"], s["fm"], s["kd"], s["cam"][k], flat, tex)
        assert torch.equal(img[0, k].reshape(3, -1), mean_of_four(colours.view(3, H * W, 4))), f"{name}, view {k}"
        same_face = (vis[0, k] == vis[0, k][:, :, :1]).all(-1).reshape(-1) & (flat.view(-1, 4)[:, 0] >= 0)
        c = colours.view(3, H * W, 4)[:, same_face]
        differs += int((c != c[:, :, :1]).any(0).any(-1).sum())
    assert differs > 0                                                                    # one face, four different texture colours: supersampling


# ---------------------------------------------------------------------------------------------------- 4. hand-made screen-space cases
def flat_samples(meshes, H=16, W=16, kd=0.5, device="cpu"):
    """meshes: [(screen points, faces)] -> (image u8 [N, 3, H, W], covered bool [N, H, W, 4]), each mesh seen by the flat camera."""
    verts, faces, voff, foff, _ = pack_meshes([tp.flat_vertices(p, H, W) for p, _ in meshes],
                                              [torch.tensor(f, dtype=torch.int64).reshape(-1, 3) for _, f in meshes], device)
    N = len(meshes)
    fm = torch.zeros((faces.shape[0],), dtype=torch.int32, device=device)
    mat = torch.full((N, 3), kd, dtype=torch.float32, device=device)
    moff = torch.arange(N + 1, dtype=torch.int64, device=device)
    img, vis = ops.render_views(verts, faces, voff, foff, fm, mat, moff, tp.FLAT_CAM.expand(N, 1, 12).contiguous().to(device), H, W, tp.FLAT_YFOV,
                                0.05, return_visibility=True, samples=4)
    return img[:, 0].cpu().numpy(), (vis[:, 0] >= 0).cpu().numpy()


def check_quad_splits(device="cpu"):
    fx, fy = np.array([p[0] for p in ar.POSITIONS]), np.array([p[1] for p in ar.POSITIONS])
    sx, sy = np.arange(16)[None, :, None] + fx, np.arange(16)[:, None, None] + fy         # the sample positions in pixels, [1, 16, 4] and [16, 1, 4]
    for name, quad in tp.QUADS.items():
        for ox, oy in tp.OFFSETS:
            for flip in (False, True):                                                   # both windings
                q = [(x + ox, y + oy) for x, y in (quad[::-1] if flip else quad)]
                _, cov = flat_samples([(q, [(0, 1, 2)]), (q, [(0, 2, 3)]), (q, [(1, 2, 3)]), (q, [(1, 3, 0)]), (q, [(0, 1, 2), (0, 2, 3)])],
                                      device=device)
                what = f"{name} quad, offset ({ox}, {oy}), flipped {flip}"
                assert cov.shape == (5, 16, 16, 4)
                assert not (cov[0] & cov[1]).any() and not (cov[2] & cov[3]).any(), what  # no sample twice, along either diagonal
                assert np.array_equal(cov[0] | cov[1], cov[2] | cov[3]), what             # and none lost: both splits cover the same set
                assert np.array_equal(cov[0] | cov[1], cov[4]) and cov[4].sum() > 0, what
                if name == "axis aligned":                                                # top and left edges in, bottom and right out
                    want = (3 + ox <= sx) & (sx < 11 + ox) & (2 + oy <= sy) & (sy < 9 + oy)
                    assert np.array_equal(cov[4], want), what


def test_quad_splits_cover_every_sample_once():
    check_quad_splits()


def check_grey_triangle(device="cpu"):
    tri = [(2.0, 1.5), (13.25, 4.0), (5.5, 12.75)]
    seen = set()
    for ox, oy in tp.OFFSETS:
        q = [(x + ox, y + oy) for x, y in tri]
        img, cov = flat_samples([(q, [(0, 1, 2)])], kd=0.5, device=device)
        k = cov[0].sum(-1)                                                                # covered samples per pixel
        c = img[0][:, k == 4]
        assert c.size and (c == c[:, :1]).all() and (img[0][:, k == 0] == 255).all()
        grey = c[:, 0].astype(np.int64)                                                   # the face's colour, from a fully covered pixel
        want = (k[None] * grey[:, None, None] + (4 - k[None]) * 255 + 2) >> 2
        assert np.array_equal(img[0].astype(np.int64), want), f"offset ({ox}, {oy})"
        assert ((k > 0) & (k < 4)).sum() > 10
        seen |= set(np.unique(k).tolist())
    assert seen == {0, 1, 2, 3, 4}


def test_a_partly_covered_pixel_blends_face_and_background():
    check_grey_triangle()


def test_a_face_between_the_centres_shows_with_four_samples():
    """A small face around sample 3 of pixel (4, 4), at (4.625, 4.875), that holds no pixel centre: one sample of one pixel, where
    the one-sample renderer draws nothing."""
    sliver = [(4.55, 4.8), (4.75, 4.8), (4.55, 5.0)]
    img, cov = flat_samples([(sliver, [(0, 1, 2)])])
    assert cov[0].sum() == 1 and cov[0][4, 4, 3]
    assert not tp.flat_coverage([(sliver, [(0, 1, 2)])]).any()                            # the one-sample renderer misses it
    assert (img[0][:, 4, 4] < 255).all() and (np.delete(img[0].reshape(3, -1), 4 * 16 + 4, axis=1) == 255).all()


# ---------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_before_anything_runs():
    verts, faces, fm, kd, cam = soup_scene()
    v, f, voff, foff, _ = pack_meshes([verts], [faces])
    m, k, moff = R.pack_materials([fm], [kd])
    cam = cam[None].contiguous()
    for bad in (0, 2, 3, 8, 16, -1, "4x", None):
        with pytest.raises(ValueError, match="samples"):
            ops.render_views(v, f, voff, foff, m, k, moff, cam, 8, 8, samples=bad)
    s = tc.scene("triangle", 0)
    batch = tc.pack([s])
    with pytest.raises(ValueError, match="samples"):
        ops.render_views_textured(*batch.tensors, *batch.texture_tensors, s["cam"][None], 8, 8, samples=2)
    # 3 views x 13378^2 pixels: 5.4e8 pixels pass the one-sample limit, 2.1e9 samples do not
    assert 3 * 13378 * 13378 < 2 ** 31 <= 3 * 13378 * 13378 * 4
    with pytest.raises(ValueError, match="2\\^31 samples.*split the batch"):
        ops.render_views(v, f, voff, foff, m, k, moff, cam, 13378, 13378, samples=4)
    with pytest.raises(ValueError, match="2\\^31 samples.*split the batch"):
        ops.render_views_textured(*batch.tensors, *batch.texture_tensors, s["cam"][None].expand(1, 3, 12).contiguous(), 13378, 13378, samples=4)
    # the C entry point itself: sizes are checked before any pointer is touched, so null pointers and no GPU will do
    lib = _C.lib()
    tail = [None, None, None, None]                                                      # workspace, image, visibility, stream

    def null(N, T):                                                                      # every pointer null, the texture group declared
        return _C.TriMeshBatch(N=N, T=T, fields=_C.TRI_MESH_TEXTURES)

    assert lib.tri_raster_workspace(200, 1, 3, 13378, 13378, 4) == 0
    assert lib.tri_raster_workspace(200, 1, 3, 32, 48, 4) == 3 * 32 * 48 * 32 + 16 + 200 * 3 * 8
    assert lib.tri_raster_workspace(200, 1, 3, 32, 48, 1) == 3 * 32 * 48 * 8 + 16 + 200 * 3 * 8
    assert [lib.tri_raster_workspace(200, 1, 3, 32, 48, bad) for bad in (0, 2, 3, 8, -1)] == [0] * 5
    rc = lib.tri_raster_render(null(1, 0), None, 200, 3, 13378, 13378, R.YFOV, R.ZNEAR, 4, *tail)
    assert rc == _C.TRI_ERR_UNSUPPORTED
    message = lib.tri_last_error().decode()
    assert "tri_raster_render" in message and "2^31 or more samples" in message and "split the batch" in message
    assert lib.tri_raster_render(null(1, -1), None, 200, 3, 8, 8, R.YFOV, R.ZNEAR, 4, *tail) != 0          # a negative texture count
    assert lib.tri_raster_render(null(1, 0), None, 200, 3, 8, 8, 4.0, R.ZNEAR, 4, *tail) != 0             # yfov beyond pi
    assert lib.tri_raster_render(null(0, 0), None, 0, 3, 8, 8, R.YFOV, R.ZNEAR, 4, *tail) == 0            # nothing to draw: nothing runs


# ---------------------------------------------------------------------------------------------------- 6. the command line
def test_preprocess_antialias_end_to_end_on_the_host(tmp_path):
    from tricolo_amd.data.dataset import PackedDataset
    runs = {}
    for mode in ("off", "4x"):
        root = str(tmp_path / mode)
        overrides = tp.write_dataset(root)
        stats = pp.main(overrides + ["--device", "cpu", "--batch-meshes", "2"] + (["--antialias", "4x"] if mode == "4x" else []), log=lambda *a: None)
        assert stats["train"] == {"models": 3, "written": 3, "skipped": 0}
        cfg = tcfg.compose(overrides=overrides)
        runs[mode] = [np.load(os.path.join(cfg.data.exp_data_root_path, c, f"{m}.npz"))["images"] for c, m in tp.MODELS[:3]]
    meshes = [load_obj_materials(os.path.join(root, "text2shape-data", "ShapeNetCore.v2", c, m, "models", "model_normalized.obj")) for c, m in tp.MODELS[:3]]
    lists = [[m[j] for m in meshes] for j in range(4)]
    want = {"off": R.render_meshes(*lists, num_views=4), "4x": R.render_meshes(*lists, num_views=4, samples=4)}
    for mode in runs:
        for k in range(3):
            assert runs[mode][k].dtype == np.uint8 and np.array_equal(runs[mode][k], want[mode][k].numpy()), (mode, k)
    for k in range(3):
        off, aa = runs["off"][k].astype(int), runs["4x"][k].astype(int)
        assert off.shape == aa.shape == (4, 3, 224, 224) and (off != aa).any()
        assert (off != aa).mean() < 0.05                                                 # they differ along the edges only
    ds = PackedDataset(cfg, "train", device="cpu")                                        # the 4x files, written last
    batch = next(iter(ds.batches(4)(0)))
    assert batch["images"].shape == (4, 4, 3, 32, 32) and batch["images"].dtype == torch.uint8
    assert torch.equal(batch["images"], ops.resize_bicubic_aa_u8(want["4x"], 32)[[0, 1, 0, 2]])
    assert "--antialias off|4x" in pp.__doc__
    with pytest.raises(SystemExit):
        pp.main(overrides + ["--antialias", "2x"], log=lambda *a: None)
