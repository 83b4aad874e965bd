"""GPU: csrc/raster.hip through ops.render_views against its torch restatement (the same call on CPU tensors): the visibility
buffer equal on every pixel, the colours equal or within 1 LSB on every pixel; batching, order independence, the full-size mesh
once, and python -m tricolo_amd.data.preprocess end to end into PackedDataset.

The scenes are those of tests/test_preprocess.py, where the restatement is compared with a float64 brute force outside pixels whose
two nearest depths are closer than 1e-5 relative.  The full-size scene here (19,860 faces, 12 views at 224 x 224) is too large for
the brute force in a test; run once by hand on the restatement (tests/raster_reference.compare, ten minutes of CPU) it gave
FULL_SIZE_BRUTE_FORCE below, and no difference outside those pixels."""
import numpy as np
import pytest
import torch

from tests import raster_reference as rr
from tests import test_preprocess as tp
from tricolo_amd import ops
from tricolo_amd.data import render as R
from tricolo_amd.evaluation.mesh import pack_meshes

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FULL_SIZE_BRUTE_FORCE = "4 ambiguous of 388,268 covered pixels (the cap is 1 %)"


def both(verts_list, faces_list, mats_list, kd_list, cam, H, W, yfov=R.YFOV, znear=R.ZNEAR):
    """(image, vis) on the GPU and on the host for the same packed batch."""
    out = []
    for dev in (DEV, torch.device("cpu")):
        v, f, voff, foff, _ = pack_meshes(verts_list, faces_list, dev)
        fm, kd, moff = R.pack_materials(mats_list, kd_list, dev)
        img, vis = ops.render_views(v, f, voff, foff, fm, kd, moff, cam.to(dev), H, W, yfov, znear, return_visibility=True)
        assert img.device.type == dev.type and img.dtype == torch.uint8 and vis.dtype == torch.int32
        out.append((img.cpu(), vis.cpu()))
    return out


def assert_same(gpu, host, what):
    (gi, gv), (hi, hv) = gpu, host
    assert gi.shape == hi.shape and gv.shape == hv.shape, what
    diff = int((gv != hv).sum())
    lsb = int((gi.to(torch.int16) - hi.to(torch.int16)).abs().max()) if gi.numel() else 0
    print(f"{what}: {int((hv >= 0).sum())} covered pixels, {diff} visibility differences, largest colour difference {lsb}")
    assert diff == 0, what
    assert lsb <= 1, what


def grey(n):
    return torch.zeros((n,), dtype=torch.int32), torch.tensor([[0.4, 0.4, 0.4]], dtype=torch.float32)


def test_one_triangle():
    verts = torch.tensor([[-0.3, -0.2, 0.0], [0.3, -0.25, 0.1], [0.05, 0.3, -0.1]], dtype=torch.float32)
    faces = torch.tensor([[0, 1, 2]])
    fm, kd = grey(1)
    cam = R.pack_cameras([R.bbox_center(verts)], 1)
    gpu, host = both([verts], [faces], [fm], [kd], cam, 16, 16)
    assert_same(gpu, host, "one triangle")
    assert 10 < int((gpu[1] == 0).sum()) < 200 and int((gpu[1] == -1).sum()) == 256 - int((gpu[1] == 0).sum())
    assert (gpu[0][gpu[1][:, :, None].expand(1, 1, 3, 16, 16) < 0] == 255).all()


def test_random_soup():
    verts, faces = rr.soup()
    g = np.random.default_rng(3)
    fm = torch.from_numpy(g.integers(0, 3, faces.shape[0]).astype(np.int32))
    kd = torch.from_numpy(g.uniform(0, 1, (3, 3)).astype(np.float32))
    cam = R.pack_cameras([R.bbox_center(verts)], 3)
    gpu, host = both([verts], [faces], [fm], [kd], cam, 32, 48)
    assert_same(gpu, host, "soup")
    assert gpu[0].shape == (1, 3, 3, 32, 48) and int((gpu[1] >= 0).sum()) > 100
    seen = set(gpu[1].unique().tolist())
    assert seen & {14, 15, 16, 17} and not seen & {12, 13}                               # the queued faces show; zero area never does


def test_coplanar_twins_and_the_near_plane():
    tri = torch.tensor([[-0.3, -0.2, 0.0], [0.3, -0.2, 0.0], [0.0, 0.3, 0.0]], dtype=torch.float32)
    verts = torch.cat([tri, tri])                                                       # the same face twice, separate vertices
    fm, kd = grey(2)
    cam = R.pack_cameras([np.zeros(3)], 2)
    for faces in (torch.tensor([[0, 1, 2], [3, 4, 5]]), torch.tensor([[3, 5, 4], [0, 2, 1]])):       # identical: the same vertex order
        gpu, host = both([verts], [faces], [fm], [kd], cam, 24, 24)
        assert_same(gpu, host, "coplanar twins")
        assert set(gpu[1].unique().tolist()) == {-1, 0}                                  # bit-equal depth: the lower index wins
    # one vertex 0.04 in front of the eye (znear 0.05): the face is dropped whole, its neighbour stays
    eye = cam[0, 0, :3].numpy().astype(np.float64)
    toward = -cam[0, 0, 9:12].numpy().astype(np.float64)
    near = torch.from_numpy((eye + 0.04 * toward).astype(np.float32))[None]
    verts = torch.cat([tri, near])
    faces = torch.tensor([[0, 1, 3], [0, 1, 2]])
    gpu, host = both([verts], [faces], [fm], [kd], cam[:, :1].contiguous(), 24, 24)
    assert_same(gpu, host, "a vertex behind znear")
    assert set(gpu[1].unique().tolist()) == {-1, 1}


def test_coverage_rules_on_the_gpu():
    tp.check_quad_splits(DEV)
    tp.check_empty_faces(DEV)


def batch_meshes():
    one = (torch.tensor([[-0.2, -0.2, 0.1], [0.25, -0.1, 0.0], [0.0, 0.3, -0.1]], dtype=torch.float32), torch.tensor([[0, 1, 2]]))
    none = (torch.zeros((0, 3), dtype=torch.float32), torch.zeros((0, 3), dtype=torch.int64))
    sv, sf = rr.soup(seed=5, n=70)
    return [one, none, (sv, sf)]


def test_batching():
    meshes = batch_meshes()
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
    meshes = batch_meshes()
    g = np.random.default_rng(9)
    mats = [torch.from_numpy(g.integers(0, 2, m[1].shape[0]).astype(np.int32)) for m in meshes]
    kds = [torch.tensor([[0.9, 0.2, 0.1], [0.1, 0.4, 0.8]], dtype=torch.float32)] * 3
    cam = R.pack_cameras([R.bbox_center(m[0]) for m in meshes], 2).to(DEV)

    def run(faces_list, mats_list):
        v, f, voff, foff, _ = pack_meshes([m[0] for m in meshes], faces_list, DEV)
        fm, kd, moff = R.pack_materials(mats_list, kds, DEV)
        return ops.render_views(v, f, voff, foff, fm, kd, moff, cam, 32, 48, return_visibility=True)

    a, b = run([m[1] for m in meshes], mats), run([m[1] for m in meshes], mats)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    perms = [torch.from_numpy(g.permutation(m[1].shape[0])) for m in meshes]
    c = run([m[1][p] for m, p in zip(meshes, perms)], [fm[p] for fm, p in zip(mats, perms)])
    assert torch.equal(a[0], c[0])                                                        # the same images
    for n, p in enumerate(perms):                                                         # and the same faces, under their new numbers
        vis = c[1][n].cpu().to(torch.int64)
        back = torch.where(vis >= 0, p[vis.clamp(min=0)] if p.numel() else vis, vis)
        assert torch.equal(back, a[1][n].cpu().to(torch.int64)), f"mesh {n}"


def test_full_size_once():
    pv, pf, pm, pk = rr.procedural_mesh(100)
    assert 19000 < pf.shape[0] < 21000
    cam = R.pack_cameras([R.bbox_center(pv)], 12)
    gpu, host = both([pv], [pf], [pm], [pk], cam, 224, 224)
    assert_same(gpu, host, f"procedural mesh, {pf.shape[0]} faces, 12 views at 224 x 224")
    assert int((gpu[1] >= 0).sum()) > 0.2 * 12 * 224 * 224
    assert int(gpu[1].max()) >= pf.shape[0] - 60                                         # the boxes (the last 60 faces, all queued) show


def test_end_to_end(tmp_path):
    tp.check_end_to_end(str(tmp_path), "cuda")
