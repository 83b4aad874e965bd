"""GPU: the four-sample kernels of csrc/raster.hip (tri_raster_render with samples == 4) through ops.render_views and ops.render_views_textured with
samples=4 against their torch restatement (the same call on CPU tensors, compared with a float64 brute force at the sample positions
in tests/test_antialias_cpu.py): the visibility equal on every sample, the colours equal or within 1 LSB on every pixel - the bound
tests/test_gpu_raster.py uses for this renderer; batching, order independence, textures, the real resolution, and the guard bands
around every operand."""
import numpy as np
import pytest
import torch

from tests import raster_reference as rr
from tests import test_antialias_cpu as ta
from tests import test_gpu_raster as gr
from tests import test_gpu_texture as gt
from tests import test_texture_cpu as tc
from tests.guard_bands import POISON, ZERO, guarded_ops, same_bytes
from tricolo_amd import ops
from tricolo_amd.data import render as R
from tricolo_amd.evaluation.mesh import pack_meshes

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def both(verts_list, faces_list, mats_list, kd_list, cam, H, W):
    """(image, vis) of the same packed batch with four samples, on the GPU and on the host."""
    out = []
    for dev in (DEV, torch.device("cpu")):
        v, f, voff, foff, _ = pack_meshes(verts_list, faces_list, dev)
        fm, kd, moff = R.pack_materials(mats_list, kd_list, dev)
        img, vis = ops.render_views(v, f, voff, foff, fm, kd, moff, cam.to(dev), H, W, return_visibility=True, samples=4)
        assert img.device.type == dev.type and img.dtype == torch.uint8 and vis.dtype == torch.int32
        assert vis.shape == (len(verts_list), cam.shape[1], H, W, 4) and img.shape == (len(verts_list), cam.shape[1], 3, H, W)
        out.append((img.cpu(), vis.cpu()))
    return out


def both_textured(scenes, cam, H, W, yfov=R.YFOV, **fields):
    out = []
    for dev in (DEV, torch.device("cpu")):
        batch = tc.pack(scenes, dev)
        tex = dict(zip(("face_uv", "mat_tex", "texels", "tex_off", "tex_size"), batch.texture_tensors))
        tex.update({k: v.to(dev) for k, v in fields.items()})
        img, vis = ops.render_views_textured(*batch.tensors, *tex.values(), cam.to(dev), H, W, yfov, R.ZNEAR, return_visibility=True, samples=4)
        out.append((img.cpu(), vis.cpu()))
    return out


def assert_same(gpu, host, what):
    (gi, gv), (hi, hv) = gpu, host
    assert gi.shape == hi.shape and gv.shape == hv.shape and gi.dtype == torch.uint8 and gv.dtype == torch.int32, what
    diff = int((gv != hv).sum())
    lsb = int((gi.to(torch.int16) - hi.to(torch.int16)).abs().max()) if gi.numel() else 0
    mixed = int((hv != hv[..., :1]).any(-1).sum())
    print(f"{what}: {int((hv >= 0).sum())} covered samples, {mixed} pixels with differing samples, {diff} visibility differences, "
          f"largest colour difference {lsb}")
    assert diff == 0, what
    assert lsb <= 1, what


def test_one_triangle():
    verts = torch.tensor([[-0.3, -0.2, 0.0], [0.3, -0.25, 0.1], [0.05, 0.3, -0.1]], dtype=torch.float32)
    fm, kd = gr.grey(1)
    cam = R.pack_cameras([R.bbox_center(verts)], 1)
    gpu, host = both([verts], [torch.tensor([[0, 1, 2]])], [fm], [kd], cam, 16, 16)
    assert_same(gpu, host, "one triangle")
    k = (gpu[1][0, 0] >= 0).sum(-1)
    assert 40 < int(k.sum()) < 800 and ((k > 0) & (k < 4)).sum() > 5
    assert (gpu[0][0, 0][:, k == 0] == 255).all() and (gpu[0][0, 0][:, k > 0] < 255).all()
    one = ops.render_views(*pack_meshes([verts], [torch.tensor([[0, 1, 2]])], DEV)[:4], *R.pack_materials([fm], [kd], DEV), cam.to(DEV), 16, 16,
                           return_visibility=True)
    assert one[1].shape == (1, 1, 16, 16) and not torch.equal(one[0].cpu(), gpu[0])       # the default is still one sample


def test_random_soup():
    verts, faces, fm, kd, cam = ta.soup_scene()
    gpu, host = both([verts], [faces], [fm], [kd], cam[None], 32, 48)
    assert_same(gpu, host, "soup")
    seen = set(gpu[1].unique().tolist())
    assert seen & {14, 15, 16, 17} and not seen & {12, 13}                               # the queued faces show; zero area never does


def test_boxes_that_reach_the_border_through_a_sample_offset():
    """Faces whose bounding box ends between the last pixel centre and the last sample of a row or column (and begins between the
    first sample and the first centre): the one-sample box leaves that pixel out, the four-sample box must not - and must not step
    over the image's edge either."""
    H = W = 16
    meshes = []
    for lo, hi in ((15.55, 15.95), (0.05, 0.45)):                                        # beyond the last centre 15.5; before the first, 0.5
        small = [(lo, 3.0), (hi, 3.0), (lo, 9.0), (hi, 9.0)]                              # a lane's box: 1 x 7 pixels
        large = [(3.0, lo), (14.0, lo), (3.0, hi), (14.0, hi)]                            # the queue's: 12 x 1
        for pts in (small, large, [(y, x) for x, y in small], [(y, x) for x, y in large]):
            meshes.append((pts, [(0, 1, 2), (2, 1, 3)]))
    for dev in ("cuda", "cpu"):
        img, cov = ta.flat_samples(meshes, H, W, device=dev)
        if dev == "cuda":
            gpu = (img, cov)
    assert np.array_equal(gpu[1], cov) and np.abs(gpu[0].astype(int) - img.astype(int)).max() <= 1
    assert cov.reshape(len(meshes), -1).any(1).all()                                      # every one of them shows
    assert not np.asarray(ta.tp.flat_coverage(meshes, H, W, device="cuda")).any()        # and none holds a pixel centre


def test_coverage_rules_on_the_gpu():
    ta.check_quad_splits(DEV)
    ta.check_grey_triangle(DEV)


def test_batching():
    meshes = gr.batch_meshes()
    mats = [torch.zeros((m[1].shape[0],), dtype=torch.int32) for m in meshes]
    kds = [torch.tensor([[0.2 + 0.3 * k, 0.5, 0.9 - 0.3 * k]], dtype=torch.float32) for k in range(3)]
    cam = R.pack_cameras([R.bbox_center(m[0]) for m in meshes], 2)
    gpu, host = both([m[0] for m in meshes], [m[1] for m in meshes], mats, kds, cam, 32, 48)
    assert_same(gpu, host, "three meshes")
    assert (gpu[1][1] == -1).all() and (gpu[0][1] == 255).all()                          # the empty mesh: background
    assert (gpu[1][0] >= 0).any() and (gpu[1][2] >= 0).any()
    for n in (0, 2):
        alone, _ = both([meshes[n][0]], [meshes[n][1]], [mats[n]], [kds[n]], cam[n:n + 1].contiguous(), 32, 48)
        assert torch.equal(alone[0][0], gpu[0][n]) and torch.equal(alone[1][0], gpu[1][n]), f"mesh {n} alone"


def test_order_independence():
    meshes = gr.batch_meshes()
    g = np.random.default_rng(9)
    mats = [torch.from_numpy(g.integers(0, 2, m[1].shape[0]).astype(np.int32)) for m in meshes]
    kds = [torch.tensor([[0.9, 0.2, 0.1], [0.1, 0.4, 0.8]], dtype=torch.float32)] * 3
    cam = R.pack_cameras([R.bbox_center(m[0]) for m in meshes], 2).to(DEV)

    def run(faces_list, mats_list):
        v, f, voff, foff, _ = pack_meshes([m[0] for m in meshes], faces_list, DEV)
        fm, kd, moff = R.pack_materials(mats_list, kds, DEV)
        return ops.render_views(v, f, voff, foff, fm, kd, moff, cam, 32, 48, return_visibility=True, samples=4)

    a, b = run([m[1] for m in meshes], mats), run([m[1] for m in meshes], mats)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])                            # two runs: identical bytes
    perms = [torch.from_numpy(g.permutation(m[1].shape[0])) for m in meshes]
    c = run([m[1][p] for m, p in zip(meshes, perms)], [fm[p] for fm, p in zip(mats, perms)])
    assert torch.equal(a[0], c[0])                                                        # the same images
    for n, p in enumerate(perms):                                                         # and the same faces, under their new numbers
        vis = c[1][n].cpu().to(torch.int64)
        back = torch.where(vis >= 0, p[vis.clamp(min=0)] if p.numel() else vis, vis)
        assert torch.equal(back, a[1][n].cpu().to(torch.int64)), f"mesh {n}"


def test_textured():
    s = tc.scene("soup", 1)
    s["uv"][5] = float("nan")
    s["uv"][7, 2, 1] = float("inf")
    gpu, host = both_textured([s], s["cam"][None], 32, 48)
    assert_same(gpu, host, "textured soup")
    q = tc.scene("quads", 2)
    gpu, host = both_textured([q], q["cam"][None], 16, 16, q["yfov"])
    assert_same(gpu, host, "textured quads")
    meshes = gt.three_meshes()                                                            # texture offsets; an untextured mesh in the middle
    cam = torch.stack([m["cam"] for m in meshes])
    gpu, host = both_textured(meshes, cam, 32, 48)
    assert_same(gpu, host, "three textured meshes")
    for n, m in enumerate(meshes):
        alone, _ = both_textured([m], m["cam"][None], 32, 48)
        assert torch.equal(alone[0][0], gpu[0][n]) and torch.equal(alone[1][0], gpu[1][n]), f"mesh {n} alone"


def test_a_batch_without_textures():
    """T == 0 through render_views_textured, and the same batch through render_views: the untextured resolve, the same bytes."""
    s = tc.scene("soup", 1)
    batch = tc.pack([s], DEV)
    none = dict(mat_tex=torch.full_like(batch.mat_tex, -1), texels=batch.texels[:0].contiguous(), tex_off=batch.tex_off[:1].contiguous(),
                tex_size=batch.tex_size[:0].contiguous())
    gpu, host = both_textured([s], s["cam"][None], 32, 48, **{k: v.cpu() for k, v in none.items()})
    assert_same(gpu, host, "T == 0")
    plain = ops.render_views(*batch.tensors, s["cam"][None].to(DEV), 32, 48, return_visibility=True, samples=4)
    assert torch.equal(plain[0].cpu(), gpu[0]) and torch.equal(plain[1].cpu(), gpu[1])
    off = both_textured([s], s["cam"][None], 32, 48, mat_tex=torch.full_like(batch.mat_tex, -1).cpu())[0]     # T > 0, no material uses it
    assert torch.equal(off[0], gpu[0]) and torch.equal(off[1], gpu[1])


def test_real_resolution():
    pv, pf, pm, pk = rr.procedural_mesh(12)
    cam = R.pack_cameras([R.bbox_center(pv)], 2)
    gpu, host = both([pv], [pf], [pm], [pk], cam, 224, 224)
    assert_same(gpu, host, f"procedural mesh, {pf.shape[0]} faces, 2 views at 224 x 224")
    assert int((gpu[1] >= 0).any(-1).sum()) > 0.2 * 2 * 224 * 224
    assert int(gpu[1].max()) >= pf.shape[0] - 60                                         # the boxes (the last 60 faces, all queued) show


def test_guard_bands():
    """Every operand of the call - texels, face_uv and both outputs among them - and the workspace between 1 MiB margins, under both
    fills: the margins come back intact and the results do not depend on what they hold.  With and without textures."""
    meshes = gt.three_meshes()
    host = tc.pack(meshes)
    cam = torch.stack([s["cam"] for s in meshes])
    out = []
    for fill in (POISON, ZERO):
        with guarded_ops(fill) as g:
            t = [g.put(x) for x in host.tensors]
            x = [g.put(x) for x in host.texture_tensors]
            c = g.put(cam)
            img, vis = ops.render_views_textured(*t, *x, c, 32, 48, return_visibility=True, samples=4)
            pimg, pvis = ops.render_views(*t, c, 32, 48, return_visibility=True, samples=4)
            assert all(hasattr(o, "_band") for o in (img, vis, pimg, pvis))               # the outputs are banded too
        assert "tri_raster_render" in g.launched and len(g.raster_calls) == 2 and all(n == 4 for _, n in g.raster_calls)      # four samples, both
        out.append((img.clone(), vis.clone(), pimg.clone(), pvis.clone()))
    for a, b in zip(*out):
        assert same_bytes(a, b)
    want = ops.render_views_textured(*host.tensors, *host.texture_tensors, cam, 32, 48, return_visibility=True, samples=4)
    assert torch.equal(out[0][1].cpu(), want[1]) and int((out[0][0].cpu().to(torch.int16) - want[0].to(torch.int16)).abs().max()) <= 1
    assert vis.shape == (3, 2, 32, 48, 4) and same_bytes(out[0][1], out[0][3])            # textures leave the visibility alone
