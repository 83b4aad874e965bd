"""GPU: csrc/voxelize.hip through ops.voxelize_meshes against its torch restatement (the same call on CPU tensors): grids and
labels equal on every byte; the row words of the fill at V = 32, 64 and 128, the in-lane and the queue path, batching, order
independence, surface-only mode, the full-size mesh once, and python -m tricolo_amd.data.preprocess --voxels mesh end to end into
PackedDataset.

The scenes are those of tests/test_voxelize.py, where the restatement is compared with the exact rational reference on every voxel."""
import numpy as np
import pytest
import torch

from tests import raster_reference as rr
from tests import test_voxelize as tv
from tests import voxelize_reference as vr
from tricolo_amd.data import voxelize as VX

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def both(scenes, V, fill="carve", what=""):
    """(grid, labels) from the GPU after asserting that the host gives the same bytes."""
    gpu, host = tv.run(scenes, V, fill, DEV), tv.run(scenes, V, fill, "cpu")
    diff = int((gpu[1] != host[1]).sum()), int((gpu[0] != host[0]).sum())
    print(f"{what}: {int((host[1] == 1).sum())} surface and {int((host[1] == 2).sum())} interior voxels, {diff[0]} label and {diff[1]} grid bytes differ")
    assert diff == (0, 0), what
    tv.check_invariants(*gpu)
    return gpu


def candidates(scene, V):
    """The (face, voxel) pairs the scene expands to, the largest candidate box, and the faces whose box holds at most 8 voxels."""
    ok, G = VX.snap_vertices(scene[0], scene[4])
    _, nrm, b0, b1 = VX.face_setup(G, scene[1], V)
    cnt = (b1 - b0 + 1).clamp(min=0).prod(1) * (ok[scene[1]].all(1) & (nrm != 0).any(1))
    return int(cnt.sum()), int(cnt.max()), int(((cnt > 0) & (cnt <= 8)).sum())


def test_one_triangle():
    grid, labels = both([vr.one_triangle()], 32, what="one triangle")
    assert 20 < int((labels == 1).sum()) < 400


UNIT = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float32)


def scaled_soup(V, frame=None):
    """The soup spread over the whole grid of V, so that the rays of the fill cross the 32-bit words of a row."""
    frame = torch.tensor([-0.1, 0.05, -0.2, 1.0 / V], dtype=torch.float32) if frame is None else frame
    return vr.soup(n=60 * V // 32, seed=21 + V, frame=frame, span=V - 3.0, size=0.02 * V)


@pytest.mark.parametrize("V", [32, 64, 128])
def test_random_soup(V):
    scene = vr.soup() if V == 32 else scaled_soup(V)
    grid, labels = both([scene], V, what=f"soup at {V}")
    assert int((labels == 1).sum()) > 200
    inner, shell = scaled_soup(V, UNIT), vr.box_shell((1.5, 2.5, 0.5), (V - 2.5, V - 1.5, V - 0.5), UNIT, top_material=1)
    merged = (torch.cat([inner[0], shell[0]]), torch.cat([inner[1], shell[1] + inner[0].shape[0]]), torch.cat([inner[2], shell[2]]), inner[3], UNIT)
    _, labels = both([merged], V, what=f"soup in a shell at {V}")                      # interior rays that stop at the soup, in every word
    assert int((labels == 2).sum()) > 0.5 * (V - 6) ** 3


def test_spanning_face_and_small_faces():
    for V in (32, 128):
        scene = vr.spanning(V)
        total, largest, small = candidates(scene, V)
        assert largest > 4096 and small > 150                                            # the queue path and the in-lane path both run
        grid, labels = both([scene], V, what=f"one spanning face, 300 small ones at {V}")
        assert (labels[0, 0] == 1).any() and (labels[0, V - 1] == 1).any()


def test_boundary_plane_and_zero_area():
    grid, labels = both([vr.boundary_plane()], 32, what="boundary plane")
    assert torch.equal(labels[0, 2] == 1, labels[0, 3] == 1) and (labels[0, 2] == 1).any()
    both([vr.zero_area()], 32, what="zero area")
    both([vr.outside()], 32, what="outside the frame")
    both([vr.beyond_snap()], 32, what="beyond the snap bound")


def test_batching():
    scenes = tv.batch_of_three()
    grid, labels = both(scenes, 32, what="three meshes")
    assert not grid[1].any() and not labels[1].any()
    for n in (0, 2):
        g, l = tv.run([scenes[n]], 32, device=DEV)
        assert torch.equal(g[0], grid[n]) and torch.equal(l[0], labels[n]), f"mesh {n} alone"


def test_order_independence():
    scene = scaled_soup(64)
    a, b = tv.run([scene], 64, device=DEV), tv.run([scene], 64, device=DEV)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    p = torch.from_numpy(np.random.default_rng(5).permutation(scene[1].shape[0]))
    c = tv.run([(scene[0], scene[1][p], scene[2][p], scene[3], scene[4])], 64, device=DEV)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


def test_surface_only():
    shell = vr.box_shell((4.5, 4.5, 4.5), (12.5, 12.5, 12.5), UNIT, top_material=1)
    grid, labels = both([shell, vr.soup()], 32, "surface", what="surface only")
    assert int((labels[0] == 1).sum()) == 9 ** 3 - 7 ** 3 and int((labels == 2).sum()) == 0
    solid, _ = both([shell], 32, what="the same shell, carved")
    assert int((solid[0, 3] == 255).sum()) == 9 ** 3


def test_full_size_once():
    pv, pf, pm, pk = rr.procedural_mesh(100)
    assert 19000 < pf.shape[0] < 21000
    scene = (pv, pf, pm, pk, VX.default_frames([pv], 128)[0])
    total, largest, _ = candidates(scene, 128)
    print(f"procedural mesh, {pf.shape[0]} faces at 128: {total} candidate pairs, the largest box {largest}")
    grid, labels = both([scene], 128, what="procedural mesh at 128")
    assert int((labels == 2).sum()) > 100000 and largest > 4096


def test_end_to_end(tmp_path):
    tv.check_preprocess_from_meshes(str(tmp_path), "cuda")
