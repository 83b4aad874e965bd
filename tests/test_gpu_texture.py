"""GPU: the textured resolve kernel and the face-colour kernel of csrc/raster.hip through ops.render_views_textured and
ops.mesh_face_colours against their torch restatements (the same calls on CPU tensors, compared with a float64 brute force in
tests/test_texture_cpu.py): the visibility buffer equal on every pixel, the colours equal or within 1 LSB on every pixel - the
restatement gives the kernel's bits, the LSB is the allowance tests/test_gpu_raster.py makes; batching with texture offsets, the
clamp of a bad texture index, a batch without textures, the byte-for-byte identities, and the guard bands around every operand."""
import numpy as np
import pytest
import torch

from tests import test_texture_cpu as tc
from tests.guard_bands import POISON, ZERO, guarded_ops, same_bytes
from tricolo_amd import _C, ops
from tricolo_amd.data import render as R
from tricolo_amd.meshes import MeshBatch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def both(scenes, cam, H, W, yfov=R.YFOV, **fields):
    """(image, vis) of the same textured batch on the GPU and on the host."""
    out = []
    for dev in (DEV, torch.device("cpu")):
        batch = tc.pack(scenes, dev)
        assert batch.texels.device.type == dev.type
        out.append(tc.textured(batch, cam, H, W, yfov, **{k: v.to(dev) for k, v in fields.items()}))
    return out


def assert_same(gpu, host, what):
    (gi, gv), (hi, hv) = gpu, host
    assert gi.shape == hi.shape and gv.shape == hv.shape and gi.dtype == torch.uint8 and gv.dtype == torch.int32, what
    diff = int((gv != hv).sum())
    lsb = int((gi.to(torch.int16) - hi.to(torch.int16)).abs().max())
    print(f"{what}: {int((hv >= 0).sum())} covered pixels, {diff} visibility differences, largest colour difference {lsb}")
    assert diff == 0 and lsb <= 1, what


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_one_triangle(shift):
    s = tc.scene("triangle", shift)
    gpu, host = both([s], s["cam"][None], 16, 16)
    assert_same(gpu, host, f"one triangle, texture {tc.TEXTURE_SIZES[shift]}")
    assert 10 < int((gpu[1] == 0).sum()) < 200


def test_random_soup():
    s = tc.scene("soup", 1)
    s["uv"][5] = float("nan")
    s["uv"][7, 2, 1] = float("inf")                                                      # not the marker: untextured where (u, v) is not finite
    gpu, host = both([s], s["cam"][None], 32, 48)
    assert_same(gpu, host, "soup")
    seen = set(gpu[1].unique().tolist())
    assert gpu[0].shape == (1, 3, 3, 32, 48) and seen & {14, 15, 16, 17} and not seen & {12, 13}          # queued faces show, zero-area ones never


def test_flat_quads():
    s = tc.scene("quads", 2)
    gpu, host = both([s], s["cam"][None], 16, 16, s["yfov"])
    assert_same(gpu, host, "quads")


def three_meshes():
    """Textured (5 x 7 and 2 x 3), untextured, textured (3 x 11 and 1 x 1): offsets of faces, materials, textures and texels all differ."""
    a, b, c = tc.scene("soup", 0), tc.scene("triangle", 0), tc.scene("soup", 2)
    a["texs"] = tc.noise_textures(31, [(5, 7), (2, 3)])
    a["mt"] = torch.tensor([0, 1, -1], dtype=torch.int32)
    b["texs"], b["mt"] = [], torch.tensor([-1], dtype=torch.int32)
    c["texs"] = tc.noise_textures(32, [(3, 11), (1, 1)])
    c["mt"] = torch.tensor([1, 0, 0], dtype=torch.int32)
    for s in (a, b, c):
        s["cam"] = R.pack_cameras([R.bbox_center(s["verts"])], 2)[0]
    return [a, b, c]


def test_batching_with_texture_offsets():
    meshes = three_meshes()
    cam = torch.stack([s["cam"] for s in meshes])
    gpu, host = both(meshes, cam, 32, 48)
    assert_same(gpu, host, "three meshes")
    assert tc.pack(meshes).mat_tex.tolist() == [0, 1, -1, -1, 3, 2, 2] and tc.pack(meshes).tex_off.tolist() == [0, 35, 41, 74, 75]
    for n, s in enumerate(meshes):
        alone, _ = both([s], s["cam"][None], 32, 48)
        assert torch.equal(alone[0][0], gpu[0][n]) and torch.equal(alone[1][0], gpu[1][n]), f"mesh {n} alone"
        assert (gpu[1][n] >= 0).any()


def test_a_bad_texture_index_reads_the_last_texture():
    s = tc.scene("soup", 0)                                                              # four textures; material 1 -> T + 5, material 2 -> a negative one
    bad = torch.tensor([0, 4 + 5, -7], dtype=torch.int32)
    last = torch.tensor([0, 3, 3], dtype=torch.int32)
    gpu, host = both([s], s["cam"][None], 32, 48, mat_tex=bad)
    assert_same(gpu, host, "mat_tex beyond T")
    want = tc.textured(tc.pack([s], DEV), s["cam"][None], 32, 48, mat_tex=last.to(DEV))
    assert torch.equal(gpu[0], want[0]) and torch.equal(gpu[1], want[1])
    other = tc.textured(tc.pack([s], DEV), s["cam"][None], 32, 48, mat_tex=torch.tensor([0, 2, 2], dtype=torch.int32, device=DEV))
    assert not torch.equal(gpu[0], other[0])                                             # and the last texture is not the one before it


def test_identities_on_the_gpu():
    tc.check_identities(DEV)                                                             # T == 0 among them


def face_colour_scene():
    s = tc.scene("soup", 0)
    s["kd"] = torch.cat([s["kd"], torch.tensor([[0.2, 0.5, 0.7]])])
    s["mt"] = torch.tensor([0, 2, 3, -1], dtype=torch.int32)
    s["fm"][100:150] = 3
    s["uv"][20:30] = float("nan")
    s["uv"][30:33, 1, 0] = float("inf")
    return s


def test_face_colours():
    meshes = three_meshes() + [face_colour_scene()]
    got = ops.mesh_face_colours(tc.pack(meshes, DEV))
    want = ops.mesh_face_colours(tc.pack(meshes))
    assert got.is_cuda and got.shape == want.shape == (601, 3) and got.dtype == torch.float32
    g, w = got.cpu(), want
    ulp = torch.maximum(w.abs(), torch.tensor(2.0 ** -126)).log2().floor().sub(23).exp2()
    worst = float(((g - w).abs() / ulp).max())
    print(f"face colours, GPU against the restatement: largest difference {worst:g} ulp of fp32, {int((g != w).sum())} of {w.numel()} values differ")
    assert torch.isfinite(g).all() and worst <= 1.0
    plain = torch.isnan(meshes[3]["uv"][:, 0, 0]) | (meshes[3]["fm"] == 3) | torch.isinf(meshes[3]["uv"][:, 1, 0])
    assert torch.equal(g[401:][plain], meshes[3]["kd"][meshes[3]["fm"].long()][plain])   # Kd itself where there is no texture
    assert torch.equal(g[200:201], torch.tensor([[0.9, 0.6, 0.8]]))                      # the mesh in the middle has none


def test_guard_bands():
    """Every operand of both calls - texels, face_uv and the outputs among them - between 1 MiB margins, under both fills: the margins
    come back intact and the results do not depend on what they hold."""
    meshes = three_meshes()
    host = tc.pack(meshes)
    cam = torch.stack([s["cam"] for s in meshes])
    out = []
    for fill in (POISON, ZERO):
        with guarded_ops(fill) as g:
            t = [g.put(x) for x in host.tensors]
            x = [g.put(x) for x in host.texture_tensors]
            banded = MeshBatch(*t, host.max_faces, host.boxes, *x)
            img, vis = ops.render_views_textured(*t, *x, g.put(cam), 32, 48, return_visibility=True)
            colours = ops.mesh_face_colours(banded)
            assert hasattr(img, "_band") and hasattr(vis, "_band") and hasattr(colours, "_band")              # the outputs are banded too
        assert {"tri_raster_render", "tri_mesh_face_colours"} <= set(g.launched)
        assert g.raster_calls == [(_C.TRI_MESH_TEXTURES, 1)]                                 # textures and no pyramid declared, one sample
        out.append((img.clone(), vis.clone(), colours.clone()))
    for a, b in zip(*out):
        assert same_bytes(a, b)
    want = tc.textured(host, cam, 32, 48)
    assert torch.equal(out[0][1].cpu(), want[1]) and int((out[0][0].cpu().to(torch.int16) - want[0].to(torch.int16)).abs().max()) <= 1
