"""GPU: the metallic-roughness BRDF on the device - tri_raster_render with TRI_MESH_PBR (the BRDF resolve kernels of csrc/raster.hip) against its
torch restatement, which tests/test_brdf_cpu.py ties to float64 and to closed forms.  The scenes are that file's.  Visibility must be
equal; colours may differ by 1 LSB, the allowance of tests/test_gpu_raster.py (the device's fp32 operations are the restatement's,
each rounded on its own, so in practice they are equal; the count of differing values is printed and 0 is expected).  The same
comparison runs at the extremes of the two factors and of Kd, with NaN factors and for the mesh without materials; batching, the
unchanged visibility, the closed forms, the clamps, the fallback, the face order and the refusals of the CPU file run here on the
device; the entry point runs between guard bands under both fills, and refuses a null mat_pbr before anything is launched."""
import pytest
import torch

from tests import guard_bands as gb
from tests import test_brdf_cpu as tb
from tests import test_normals_cpu as tn
from tricolo_amd import _C, ops
from tricolo_amd.data import render as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAN = float("nan")


def assert_same(gpu, host, what):
    assert torch.equal(gpu[1], host[1]), f"{what}: visibility differs in {int((gpu[1] != host[1]).sum())} entries"
    diff = (gpu[0].to(torch.int32) - host[0].to(torch.int32)).abs()
    print(f"{what}: {int((host[1] >= 0).sum())} covered, {int((diff > 0).sum())} colour values differ, largest difference {int(diff.max())}")
    assert int(diff.max()) <= 1, what


def both(packed, cam, H, W, yfov, mode, samples, smooth, pbr=None):
    """packed: (the batch on the device, the batch on the host), packed once per scene; pbr: a host tensor in place of the batch's."""
    return tuple(tb.render(b, cam, H, W, yfov, mode, samples, smooth, brdf="batch" if pbr is None else pbr.to(b.verts.device)) for b in packed)


@pytest.mark.parametrize("name", ["triangle", "soup", "quads", "sphere"])
def test_device_matches_the_restatement(name):
    s = tn.scene(name)
    packed = tb.pack([s], DEV), tb.pack([s])
    for mode in tb.MODES:
        for smooth in (False, True):
            for samples in (1, 4):
                gpu, host = both(packed, s["cam"][None], s["H"], s["W"], s["yfov"], mode, samples, smooth)
                assert (host[1] >= 0).sum() > 20
                assert_same(gpu, host, f"{name}, {mode}, {'smooth' if smooth else 'flat'}, {samples} sample(s)")
                plain = tn.render(packed[0], s["cam"][None], s["H"], s["W"], s["yfov"], mode, samples)
                assert torch.equal(plain[1], gpu[1]) and not torch.equal(plain[0], gpu[0]), "the visibility of the plain call, another picture"


def test_the_extremes():
    s = tn.scene("soup")
    s["cam"] = s["cam"][:1]
    M = s["kd"].shape[0]
    packed = tb.pack([s], DEV), tb.pack([s])
    factors = {"r = 0.04, m = 0": (0.0, 0.04), "r = 0.04, m = 1": (1.0, 0.04), "r = 1, m = 0": (0.0, 1.0), "r = 1, m = 1": (1.0, 1.0),
               "NaN factors": (NAN, NAN), "beyond the clamps": (-2.0, 9.0)}
    for what, (m, r) in factors.items():
        pbr = torch.tensor([[m, r]] * M)
        for mode, samples, smooth in (("plain", 1, False), ("mip", 4, True)):
            gpu, host = both(packed, s["cam"][None], s["H"], s["W"], s["yfov"], mode, samples, smooth, pbr)
            assert_same(gpu, host, f"{what}, {mode}, {samples} sample(s)")
    for kd in (0.0, 1.0):
        flat = dict(s, kd=torch.full_like(s["kd"], kd))
        pair = tb.pack([flat], DEV), tb.pack([flat])
        for mode, samples, smooth in (("plain", 4, True), ("textured", 1, False)):
            gpu, host = both(pair, s["cam"][None], s["H"], s["W"], s["yfov"], mode, samples, smooth)
            assert_same(gpu, host, f"Kd = {kd}, {mode}, {samples} sample(s)")
    sphere = tn.scene("sphere")
    for samples in (1, 4):
        out = []
        for dev in (DEV, "cpu"):
            batch, t, pbr = tb.without_materials(sphere, dev)
            img, vis = ops.render_views(*t, sphere["cam"][None].to(dev), sphere["H"], sphere["W"], sphere["yfov"], R.ZNEAR, return_visibility=True,
                                        samples=samples, normals=batch.face_vn, brdf=pbr)
            out.append((img.cpu(), vis.cpu()))
        assert_same(out[0], out[1], f"no materials, {samples} sample(s)")


def test_batching_with_every_offset_different():
    tb.check_batching(DEV)                                                               # batched against alone on the device, equal bits
    meshes = tb.brdf_meshes()
    cam = torch.stack([s["cam"] for s in meshes])
    packed = tb.pack(meshes, DEV), tb.pack(meshes)
    for samples in (1, 4):
        gpu, host = both(packed, cam, 32, 48, R.YFOV, "mip", samples, True)
        assert_same(gpu, host, f"three meshes, mip, smooth, {samples} sample(s)")


def test_the_cpu_checks_on_the_device():
    tb.check_identities(DEV)                                                             # brdf=None is the call as it was; visibility never changes
    tb.check_closed_forms(DEV)
    tb.check_clamps(DEV)
    tb.check_degenerate(DEV)
    tb.check_face_order(DEV)
    tb.check_refusals(DEV)


@pytest.mark.parametrize("samples", [1, 4])
def test_guard_bands_around_the_brdf_render(samples):
    meshes = tb.brdf_meshes()
    host = tb.pack(meshes)
    cam = torch.stack([s["cam"] for s in meshes])
    results = []
    for fill in (gb.POISON, gb.ZERO):
        with gb.guarded_ops(fill) as g:
            mesh = [g.put(t) for t in host.tensors]
            tex = [g.put(t) for t in host.texture_tensors]
            mips = tuple(g.put(t) for t in host.mip_tensors)
            vn, pbr, c = g.put(host.face_vn), g.put(host.mat_pbr), g.put(cam)
            flat = ops.render_views(*mesh, c, 32, 48, return_visibility=True, samples=samples, brdf=pbr)                 # no face_vn, no textures
            smooth = ops.render_views(*mesh, c, 32, 48, return_visibility=True, samples=samples, normals=vn, brdf=pbr)
            tx = ops.render_views_textured(*mesh, *tex, c, 32, 48, return_visibility=True, samples=samples, brdf=pbr)    # textures, no pyramid
            mip = ops.render_views_textured(*mesh, *tex, c, 32, 48, return_visibility=True, samples=samples, mips=mips, normals=vn, brdf=pbr)
            assert all(hasattr(y, "_band") for y in flat + smooth + tx + mip)
            results.append([t.cpu() for t in flat + smooth + tx + mip])
        assert set(g.launched) == {"tri_raster_render"} and len(g.raster_calls) == 4
        assert all(fields & _C.TRI_MESH_PBR and n == samples for fields, n in g.raster_calls)     # every call declared mat_pbr: the BRDF resolve
    assert all(gb.same_bytes(a, b) for a, b in zip(*results))
    for k, (mode, smooth) in enumerate((("plain", False), ("plain", True), ("textured", False), ("mip", True))):
        want = tb.render(host, cam, 32, 48, mode=mode, samples=samples, smooth=smooth)
        assert torch.equal(results[0][2 * k + 1], want[1]) and int((results[0][2 * k].to(torch.int32) - want[0].to(torch.int32)).abs().max()) <= 1


def test_a_null_mat_pbr_is_refused_and_nothing_is_launched():
    s = tn.scene("triangle")
    batch = tb.pack([s], DEV)
    cam = s["cam"][None].to(DEV)
    image = torch.full((1, 1, 3, 16, 16), 77, dtype=torch.uint8, device=DEV)
    ws = torch.zeros((max(16, _C.lib().tri_raster_workspace(1, 1, 1, 16, 16, 1)),), dtype=torch.uint8, device=DEV)
    ptr = _C.ptr
    desc = _C.TriMeshBatch(*(ptr(t) for t in batch.tensors), 1, fields=_C.TRI_MESH_PBR)          # mat_pbr declared, and null
    tail = [ptr(cam), 1, 1, 16, 16, R.YFOV, R.ZNEAR, 1, ptr(ws), ptr(image), None, None]
    assert _C.lib().tri_raster_render(desc, *tail) == _C.TRI_ERR_ARG
    assert "mat_pbr" in _C.lib().tri_last_error().decode()
    torch.cuda.synchronize()
    assert bool((image == 77).all()) and bool((ws == 0).all())
    desc.mat_pbr = ptr(batch.mat_pbr)
    assert _C.lib().tri_raster_render(desc, *tail) == 0                                 # the same call with it runs
    torch.cuda.synchronize()
    assert torch.equal(image.cpu(), ops.render_views(*batch.tensors, cam, 16, 16, brdf=batch.mat_pbr).cpu())


@pytest.mark.parametrize("samples", [1, 4])
def test_an_undeclared_group_is_not_read(samples):
    """One triangle, one view, 16 x 16 (an edge pixel is partly covered, so four samples differ from one).  The descriptor carries
    valid face_vn and mat_pbr pointers - banded allocations of their own - in its slots: with fields = 0 the call is the plain one,
    byte for byte; with TRI_MESH_PBR declared it is brdf='s; with both groups declared it is normals= with brdf=."""
    s = tn.scene("triangle")
    batch = tb.pack([s], DEV)
    cam = s["cam"][None].to(DEV)
    vn, pbr = gb.banded(batch.face_vn, gb.POISON), gb.banded(batch.mat_pbr, gb.POISON)
    lib, ptr = _C.lib(), _C.ptr
    desc = _C.TriMeshBatch(*(ptr(t) for t in batch.tensors), 1, face_vn=ptr(vn), mat_pbr=ptr(pbr), fields=0)
    want = {0: ops.render_views(*batch.tensors, cam, 16, 16, return_visibility=True, samples=samples),
            _C.TRI_MESH_PBR: ops.render_views(*batch.tensors, cam, 16, 16, return_visibility=True, samples=samples, brdf=batch.mat_pbr),
            _C.TRI_MESH_NORMALS | _C.TRI_MESH_PBR: ops.render_views(*batch.tensors, cam, 16, 16, return_visibility=True, samples=samples,
                                                                    normals=batch.face_vn, brdf=batch.mat_pbr)}
    assert not torch.equal(want[0][0], want[_C.TRI_MESH_PBR][0])
    ws = torch.empty((max(16, lib.tri_raster_workspace(1, 1, 1, 16, 16, samples)),), dtype=torch.uint8, device=DEV)
    for fields, (image, vis) in want.items():
        desc.fields = fields
        got, seen = torch.full_like(image, 77), torch.full_like(vis, -7)
        assert lib.tri_raster_render(desc, ptr(cam), 1, 1, 16, 16, R.YFOV, R.ZNEAR, samples, ptr(ws), ptr(got), ptr(seen), _C.stream()) == 0
        torch.cuda.synchronize()
        assert gb.same_bytes(got, image) and gb.same_bytes(seen, vis), fields
    assert not vn._band.damage() and not pbr._band.damage()
    if samples == 4:
        one = ops.render_views(*batch.tensors, cam, 16, 16)
        assert want[0][1].shape == (1, 1, 16, 16, 4) and not torch.equal(one, want[0][0])        # the four-sample path is another picture
