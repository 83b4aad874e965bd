"""GPU: the six modes of csrc/raster.hip - plain, textured and mip-mapped, with one and with four samples - are one launch sequence
over shared set-up, (u, v), sampling and colour code, so what one mode promises about another has to hold on the device: the same
visibility in every mode of a sample count, a batch whose materials name no texture rendered byte for byte as ops.render_views
renders it, and an untextured face coloured by the one-sample rule in every sample.  The scene is the three meshes of
tests/test_gpu_mip.py at 32 x 48 (lane-sized and queued faces, an untextured mesh, NaN and inf UVs).  The same identities on the
soup-and-triangle batch are tests/test_mip_cpu.check_mip_identities and tests/test_texture_cpu.check_identities, called here on the
device, not restated."""
import pytest
import torch

from tests import test_mip_cpu as tm
from tests import test_texture_cpu as tc
from tests.test_gpu_mip import three_meshes

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
H, W = 32, 48
MODES = {"plain": tm.plain, "textured": tm.textured, "mip": tm.mipped}


def nan_and_inf(meshes):
    meshes[0]["uv"][5] = float("nan")                                                    # the marker: a face without texture coordinates
    meshes[0]["uv"][7, 2, 1] = float("inf")                                              # not the marker: untextured where (u, v) is not finite
    return meshes


@pytest.fixture(scope="module")
def scene():
    meshes = nan_and_inf(three_meshes())
    return tc.pack(meshes, DEV), torch.stack([s["cam"] for s in meshes])


@pytest.fixture(scope="module")
def six(scene):
    """(image, vis) of every mode at both sample counts, rendered once."""
    batch, cam = scene
    return {(mode, samples): fn(batch, cam, H, W, samples=samples) for mode, fn in MODES.items() for samples in (1, 4)}


@pytest.mark.parametrize("samples", [1, 4])
def test_visibility_is_the_same_in_every_mode(six, samples):
    plain, textured, mip = (six[mode, samples] for mode in MODES)
    assert plain[1].shape == (3, 2, H, W) + ((4,) if samples == 4 else ()) and plain[0].shape == (3, 2, 3, H, W)
    assert all((plain[1][n] >= 0).sum() > 50 for n in range(3))
    assert torch.equal(textured[1], plain[1]) and torch.equal(mip[1], plain[1])
    assert not torch.equal(textured[0], plain[0]) and not torch.equal(mip[0], textured[0])       # three modes, three pictures
    assert torch.equal(textured[0][1], plain[0][1]) and torch.equal(mip[0][1], plain[0][1])      # the mesh in the middle has no texture


@pytest.mark.parametrize("samples", [1, 4])
def test_a_batch_whose_materials_name_no_texture_renders_as_render_views(scene, six, samples):
    batch, cam = scene
    none = torch.full_like(batch.mat_tex, -1)
    want = six["plain", samples]
    for mode in ("textured", "mip"):
        got = MODES[mode](batch, cam, H, W, samples=samples, mat_tex=none)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), f"{mode}, {samples} sample(s)"


def test_the_identities_of_the_texture_and_mip_tests_on_the_device():
    tc.check_identities(DEV)
    tm.check_mip_identities(DEV)


def test_every_sample_of_an_untextured_face_takes_the_one_sample_colour():
    """One slanted face that covers the whole image, untextured by its material in a batch that has a texture: the four samples of a
    pixel are four times the pixel's one-sample colour, so their rounded mean is that colour - in every mode."""
    s = tc.scene("triangle", 0)
    s["verts"] = torch.tensor([[-8.0, -8.0, 0.0], [8.0, -8.0, 0.3], [0.0, 8.0, -0.2]])
    s["mt"], s["texs"] = torch.tensor([-1], dtype=torch.int32), tc.noise_textures(5, [(4, 4)])
    cam = torch.tensor([[[0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]]])          # at z = 1, looking down -z
    batch = tc.pack([s], DEV)
    want = tm.plain(batch, cam, H, W)
    assert batch.tex_size.shape[0] == 1 and bool((want[1] == 0).all()) and int(want[0].min()) < 255
    assert len({tuple(c) for c in want[0][0, 0].reshape(3, -1).T.tolist()}) == 1                 # flat shading: one colour
    for mode, fn in MODES.items():
        one, four = fn(batch, cam, H, W), fn(batch, cam, H, W, samples=4)
        assert bool((four[1] == 0).all()) and torch.equal(one[1], want[1]), mode
        assert torch.equal(one[0], want[0]) and torch.equal(four[0], want[0]), mode
