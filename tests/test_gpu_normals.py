"""GPU: smooth shading on the device - tri_raster_render with TRI_MESH_NORMALS (the SMOOTH resolve kernels of csrc/raster.hip) and
tri_mesh_vertex_normals (csrc/mesh_normals.hip) against their torch restatements, which tests/test_normals_cpu.py ties to float64.
The scenes are that file's.  Visibility must be equal; colours may differ by 1 LSB, the allowance of tests/test_gpu_raster.py (the
device's fp32 operations are the restatement's, so in practice they are equal; the count is printed).  Computed normals must carry
their NaN markers in exactly the same faces and agree within 1 ulp of fp32, the allowance tests/test_gpu_texture.py makes for face
colours: the integer sums are exact on both sides, only the float64 square root and quotient could differ in their last bit.  The
identities, the independence of the face order and the refusals of the CPU file run here on the device, and both calls run between
guard bands under both fills."""
import pytest
import torch

from tests import guard_bands as gb
from tests import normals_reference as nr
from tests import test_normals_cpu as tn
from tests.test_gpu_mip import three_meshes
from tricolo_amd import _C, ops
from tricolo_amd.data import render as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def assert_same(gpu, host, what):
    assert torch.equal(gpu[1], host[1]), f"{what}: visibility differs in {int((gpu[1] != host[1]).sum())} entries"
    diff = (gpu[0].to(torch.int32) - host[0].to(torch.int32)).abs()
    print(f"{what}: {int((host[1] >= 0).sum())} covered, {int((diff > 0).sum())} colour values differ, largest difference {int(diff.max())}")
    assert int(diff.max()) <= 1, what


def both(packed, cam, H, W, yfov, mode, samples):
    """packed: (the batch on the device, the batch on the host), packed once per scene."""
    return tuple(tn.render(b, cam, H, W, yfov, mode, samples, b.face_vn) for b in packed)


def packed_both(scenes):
    return tn.pack(scenes, DEV), tn.pack(scenes)


@pytest.mark.parametrize("name", ["triangle", "soup", "quads", "sphere"])
def test_device_matches_the_restatement(name):
    s = tn.scene(name)
    packed = packed_both([s])
    for mode in tn.MODES:
        for samples in (1, 4):
            gpu, host = both(packed, s["cam"][None], s["H"], s["W"], s["yfov"], mode, samples)
            assert (host[1] >= 0).sum() > 20
            assert_same(gpu, host, f"{name}, {mode}, {samples} sample(s)")


def smooth_meshes():
    """tests/test_gpu_mip.three_meshes with corner normals: random ones, a face without, one with an inf; the middle mesh has none."""
    meshes = three_meshes()
    for k, s in enumerate(meshes):
        s["vn"] = tn.random_normals(s["faces"].shape[0], 70 + k)
    meshes[0]["vn"][30] = tn.NAN
    meshes[0]["vn"][31, 2, 1] = float("inf")
    meshes[1]["vn"][:] = tn.NAN
    return meshes


@pytest.mark.parametrize("samples", [1, 4])
def test_batching_with_every_offset_different(samples):
    meshes = smooth_meshes()
    cam = torch.stack([s["cam"] for s in meshes])
    packed, singles = packed_both(meshes), [tn.pack([s], DEV) for s in meshes]
    for mode in tn.MODES:
        gpu, host = both(packed, cam, 32, 48, R.YFOV, mode, samples)
        assert_same(gpu, host, f"three meshes, {mode}, {samples} sample(s)")
        for n, s in enumerate(meshes):
            alone = tn.render(singles[n], s["cam"][None], 32, 48, R.YFOV, mode, samples, singles[n].face_vn)
            assert torch.equal(alone[0][0], gpu[0][n]) and torch.equal(alone[1][0], gpu[1][n]), f"mesh {n} alone, {mode}"


def ulps(a, b):
    """The distance of two finite fp32 tensors in units in the last place (their bit patterns as ordered integers)."""
    def key(t):
        i = t.contiguous().view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return (key(a) - key(b)).abs()


def test_vertex_normals_match_the_restatement():
    sphere, soup, cone = tn.vertex_meshes()
    empty = (torch.zeros((0, 3)), torch.zeros((0, 3), dtype=torch.int64))
    meshes = [sphere, soup, empty, cone]
    given = tn.random_normals(sum(m[1].shape[0] for m in meshes), 5)
    given[::4] = tn.NAN
    for what, vn, fill in (("all faces", None, "missing"), ("fill missing", given, "missing"), ("fill all", given, "all")):
        gpu, host = tn.normals_of(meshes, DEV, vn, fill), tn.normals_of(meshes, "cpu", vn, fill)
        nan = torch.isnan(host)
        assert torch.equal(torch.isnan(gpu), nan) and torch.equal(nan.all(dim=2).all(dim=1), nan.any(dim=2).any(dim=1)), what
        off = ulps(gpu[~nan], host[~nan])
        print(f"{what}: {int((~nan).sum())} values, {int(nan[:, 0, 0].sum())} faces without, {int((off > 0).sum())} values differ, largest {int(off.max())} ulp")
        assert int(off.max()) <= 1, what
        if vn is not None and fill == "missing":
            kept = ~torch.isnan(vn[:, 0, 0])
            assert torch.equal(tn.bits(gpu[kept]), tn.bits(vn[kept]))


def test_the_cpu_checks_on_the_device():
    tn.check_face_order_and_repeats(DEV)
    tn.check_fill(DEV)
    tn.check_identities(DEV)
    tn.check_refusals(DEV)


def test_a_bad_vertex_index_takes_the_clamp_on_the_device():
    verts, faces = nr.sphere()[:2]
    V = verts.shape[0]
    off = (torch.tensor([0, V], device=DEV), torch.tensor([0, faces.shape[0]], device=DEV))
    good = faces.to(torch.int32).clone()
    good[7, 1], good[9, 2] = V - 1, V - 1
    bad = good.clone()
    bad[7, 1], bad[9, 2] = V + 50, -3
    assert torch.equal(tn.bits(ops.mesh_vertex_normals(verts.to(DEV), bad.to(DEV), *off)), tn.bits(ops.mesh_vertex_normals(verts.to(DEV), good.to(DEV), *off)))


@pytest.mark.parametrize("samples", [1, 4])
def test_guard_bands_around_the_smooth_render(samples):
    meshes = smooth_meshes()
    host = tn.pack(meshes)
    cam = torch.stack([s["cam"] for s in meshes])
    results = []
    for fill in (gb.POISON, gb.ZERO):
        with gb.guarded_ops(fill) as g:
            mesh = [g.put(t) for t in host.tensors]
            tex = [g.put(t) for t in host.texture_tensors]
            mips = tuple(g.put(t) for t in host.mip_tensors)
            vn, c = g.put(host.face_vn), g.put(cam)
            plain = ops.render_views(*mesh, c, 32, 48, return_visibility=True, samples=samples, normals=vn)
            mip = ops.render_views_textured(*mesh, *tex, c, 32, 48, return_visibility=True, samples=samples, mips=mips, normals=vn)
            results.append([t.cpu() for t in plain + mip])
        assert "tri_raster_render" in g.launched and len(g.raster_calls) == 2                    # normals declared, mat_pbr not: the SMOOTH resolve
        assert all(fields & _C.TRI_MESH_NORMALS and not fields & _C.TRI_MESH_PBR and n == samples for fields, n in g.raster_calls)
    assert all(gb.same_bytes(a, b) for a, b in zip(*results))
    want = tn.render(host, cam, 32, 48, mode="plain", samples=samples, normals=host.face_vn)
    assert torch.equal(results[0][1], want[1]) and int((results[0][0].to(torch.int32) - want[0].to(torch.int32)).abs().max()) <= 1


def test_guard_bands_around_the_vertex_normals():
    sphere, soup, cone = tn.vertex_meshes()
    host = tn.MeshBatch.pack([m[0] for m in (sphere, soup, cone)], [m[1] for m in (sphere, soup, cone)])
    given = tn.random_normals(host.faces.shape[0], 6)
    given[::2] = tn.NAN
    results = []
    for fill in (gb.POISON, gb.ZERO):
        with gb.guarded_ops(fill) as g:
            args = [g.put(t) for t in (host.verts, host.faces, host.vert_off, host.face_off)]
            vn = g.put(given)
            results.append([ops.mesh_vertex_normals(*args).cpu(), ops.mesh_vertex_normals(*args, vn, "missing").cpu(),
                            ops.mesh_vertex_normals(*args, vn, "all").cpu()])
        assert "tri_mesh_vertex_normals" in g.launched
    assert all(gb.same_bytes(a, b) for a, b in zip(*results))
    assert gb.same_bytes(results[0][0], results[0][2]) and not gb.same_bytes(results[0][0], results[0][1])
