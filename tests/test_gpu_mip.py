"""GPU: the pyramid kernel and the two mip resolve kernels of csrc/raster.hip through ops.texture_mips and
ops.render_views_textured(..., mips=) against their torch restatements (the same calls on CPU tensors, compared with integers and
with float64 in tests/test_mip_cpu.py): every byte of the pyramid equal - the arithmetic is integer, there is no allowance - the
visibility equal on every pixel or sample, the colours equal or within 1 LSB as tests/test_gpu_texture.py allows; batching with
face, material, texture, texel and pyramid offsets, the clamp of a bad texture index onto the last texture's chain, the
byte-for-byte identities and the refusals on the device, and the guard bands around every operand and output."""
import pytest
import torch

from tests import test_mip_cpu as tm
from tests import test_texture_cpu as tc
from tests.guard_bands import POISON, ZERO, guarded_ops, same_bytes
from tricolo_amd import _C, ops
from tricolo_amd.data import render as R
from tricolo_amd.meshes import MeshBatch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def both(scenes, cam, H, W, yfov=R.YFOV, samples=1, **fields):
    """(image, vis) of the same batch, mip-mapped, on the GPU and on the host - each with the pyramid built on its own device."""
    out = []
    for dev in (DEV, torch.device("cpu")):
        batch = tc.pack(scenes, dev)
        out.append(tm.mipped(batch, cam, H, W, yfov, samples, **{k: v.to(dev) for k, v in fields.items()}))
    return out


def assert_same(gpu, host, what):
    (gi, gv), (hi, hv) = gpu, host
    assert gi.shape == hi.shape and gv.shape == hv.shape and gi.dtype == torch.uint8 and gv.dtype == torch.int32, what
    diff = int((gv != hv).sum())
    lsb = int((gi.to(torch.int16) - hi.to(torch.int16)).abs().max())
    print(f"{what}: {int((hv >= 0).sum())} covered, {diff} visibility differences, largest colour difference {lsb}")
    assert diff == 0 and lsb <= 1, what


def test_pyramids_equal_the_restatement_byte_for_byte():
    tm.check_pyramids(DEV)                                                               # against the integer reference, on the device
    texs = tm.mip_textures(7) + tc.noise_textures(8, [(3, 11), (9, 1), (40, 24)])
    gpu, host = tm.packed_textures(texs, DEV), tm.packed_textures(texs)
    (gm, go), (hm, ho) = ops.texture_mips(gpu.texels, gpu.tex_off, gpu.tex_size), ops.texture_mips(host.texels, host.tex_off, host.tex_size)
    assert gm.is_cuda and go.is_cuda and torch.equal(go.cpu(), ho) and torch.equal(gm.cpu(), hm)


@pytest.mark.parametrize("samples", [1, 4])
@pytest.mark.parametrize("shift", [0, 1, 2, 3, 4, 5])
def test_one_triangle(shift, samples):
    s = tm.scene("triangle", shift)
    gpu, host = both([s], s["cam"][None], 16, 16, samples=samples)
    assert_same(gpu, host, f"one triangle, texture {tm.MIP_SIZES[shift]}, {samples} sample(s)")
    assert 10 < int((gpu[1] == 0).sum()) < 800


@pytest.mark.parametrize("samples", [1, 4])
def test_random_soup(samples):
    s = tm.scene("soup", 3)
    s["uv"][5] = float("nan")
    s["uv"][7, 2, 1] = float("inf")                                                      # not the marker: untextured where (u, v) is not finite
    gpu, host = both([s], s["cam"][None], 32, 48, samples=samples)
    assert_same(gpu, host, f"soup, {samples} sample(s)")
    seen = set(gpu[1].unique().tolist())
    assert gpu[0].shape == (1, 3, 3, 32, 48) and seen & {14, 15, 16, 17} and not seen & {12, 13}          # queued faces show, zero-area ones never


@pytest.mark.parametrize("samples", [1, 4])
def test_flat_quads(samples):
    s = tm.scene("quads", 4)
    gpu, host = both([s], s["cam"][None], 16, 16, s["yfov"], samples)
    assert_same(gpu, host, f"quads, {samples} sample(s)")


def three_meshes():
    """Textured (5 x 7 and 2 x 3), untextured, textured (3 x 11, 64 x 64 and 1 x 1): offsets of faces, materials, textures, texels and
    pyramid chains all differ."""
    a, b, c = tc.scene("soup", 0), tc.scene("triangle", 0), tc.scene("soup", 2)
    a["texs"] = tc.noise_textures(31, [(5, 7), (2, 3)])
    a["mt"] = torch.tensor([0, 1, -1], dtype=torch.int32)
    b["texs"], b["mt"] = [], torch.tensor([-1], dtype=torch.int32)
    c["texs"] = tc.noise_textures(32, [(3, 11), (64, 64), (1, 1)])
    c["mt"] = torch.tensor([1, 0, 2], dtype=torch.int32)
    for s in (a, b, c):
        s["cam"] = R.pack_cameras([R.bbox_center(s["verts"])], 2)[0]
    return [a, b, c]


@pytest.mark.parametrize("samples", [1, 4])
def test_batching_with_pyramid_offsets(samples):
    meshes = three_meshes()
    cam = torch.stack([s["cam"] for s in meshes])
    gpu, host = both(meshes, cam, 32, 48, samples=samples)
    assert_same(gpu, host, f"three meshes, {samples} sample(s)")
    packed = tc.pack(meshes).with_texture_mips()
    assert packed.mat_tex.tolist() == [0, 1, -1, -1, 3, 2, 4] and packed.tex_off.tolist() == [0, 35, 41, 74, 4170, 4171]
    assert packed.mip_off.tolist() == [0, 42, 49, 49 + 33 + 5 + 2 + 1, 90 + tm.CHAIN[5], 91 + tm.CHAIN[5]]
    for n, s in enumerate(meshes):
        alone, _ = both([s], s["cam"][None], 32, 48, samples=samples)
        assert torch.equal(alone[0][0], gpu[0][n]) and torch.equal(alone[1][0], gpu[1][n]), f"mesh {n} alone"
        assert (gpu[1][n] >= 0).any()


def test_a_bad_texture_index_reads_the_last_textures_chain():
    s = tm.scene("soup", 0)                                                              # six textures; material 1 -> T + 5, material 2 -> a negative one
    bad = torch.tensor([0, 6 + 5, -7], dtype=torch.int32)
    last = torch.tensor([0, 5, 5], dtype=torch.int32)
    for samples in (1, 4):
        gpu, host = both([s], s["cam"][None], 32, 48, samples=samples, mat_tex=bad)
        assert_same(gpu, host, f"mat_tex beyond T, {samples} sample(s)")
        want = tm.mipped(tc.pack([s], DEV), s["cam"][None], 32, 48, samples=samples, mat_tex=last.to(DEV))
        assert torch.equal(gpu[0], want[0]) and torch.equal(gpu[1], want[1])
        other = tm.mipped(tc.pack([s], DEV), s["cam"][None], 32, 48, samples=samples, mat_tex=torch.tensor([0, 4, 4], dtype=torch.int32, device=DEV))
        assert not torch.equal(gpu[0], other[0])                                         # and the last chain is not the one before it


def test_the_checker_on_the_gpu():
    tm.check_checker(DEV)


def test_identities_on_the_gpu():
    tm.check_mip_identities(DEV)                                                         # rho <= 1, untextured, T == 0, constant, winding, face order


def test_refusals_on_the_gpu():
    tm.check_refusals(DEV, elsewhere="cpu")                                              # a host pyramid for a device batch among them


def test_guard_bands():
    """Every operand and output of the pyramid build and of both mip renders between 1 MiB margins, under both fills: the margins
    come back intact and the results do not depend on what they hold."""
    meshes = three_meshes()
    host = tc.pack(meshes)
    cam = torch.stack([s["cam"] for s in meshes])
    out = []
    for fill in (POISON, ZERO):
        with guarded_ops(fill) as g:
            t = [g.put(x) for x in host.tensors]
            x = [g.put(x) for x in host.texture_tensors]
            mip_texels, mip_off = ops.texture_mips(*x[2:])
            assert hasattr(mip_texels, "_band")                                          # the pyramid is banded too
            mips = (mip_texels, g.put(mip_off.cpu()))
            c = g.put(cam)
            one = ops.render_views_textured(*t, *x, c, 32, 48, return_visibility=True, mips=mips)
            four = ops.render_views_textured(*t, *x, c, 32, 48, return_visibility=True, samples=4, mips=mips)
            assert all(hasattr(y, "_band") for y in one + four)
        assert {"tri_texture_mips", "tri_raster_render"} <= set(g.launched)
        assert [n for _, n in g.raster_calls] == [1, 4] and all(fields & _C.TRI_MESH_MIPS for fields, _ in g.raster_calls)      # the pyramid declared
        out.append((mip_texels.clone(), one[0].clone(), one[1].clone(), four[0].clone(), four[1].clone()))
    for a, b in zip(*out):
        assert same_bytes(a, b)
    want = host.with_texture_mips()
    assert torch.equal(out[0][0].cpu(), want.mip_texels)
    for k, samples in ((1, 1), (3, 4)):
        img, vis = tm.mipped(want, cam, 32, 48, samples=samples, mips=want.mip_tensors)
        assert torch.equal(out[0][k + 1].cpu(), vis) and int((out[0][k].cpu().to(torch.int16) - img.to(torch.int16)).abs().max()) <= 1
    assert isinstance(want, MeshBatch)
