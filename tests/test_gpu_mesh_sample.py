"""GPU: csrc/mesh_sample.hip through tricolo_amd.evaluation.mesh and tricolo_amd.ops - conditions A-D of tests/mesh_reference.py on
every test mesh and sample count, mixed batches, agreement with the CPU fallback away from the CDF boundaries, bit reproducibility,
the bounding boxes and the CDF against numpy, compare_meshes, rejected inputs, and nearest.jsonl from OBJ files."""
import numpy as np
import pytest
import torch

from tests import mesh_reference as mr
from tests.test_mesh_sample import SEED, run_end_to_end, sample, tmesh

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def packed(names):
    from tricolo_amd.evaluation import mesh as M
    ms = [tmesh(n) for n in names]
    return M.pack_meshes([m[0] for m in ms], [m[1] for m in ms], DEV)


@pytest.mark.parametrize("name", list(mr.MESHES))
def test_conditions_on_the_device(name):
    v, f = mr.mesh(name)
    for S in mr.SAMPLE_COUNTS:
        p, i = sample([name], S, device=DEV)
        mr.check_samples(v, f, mr.oracle_named(name, 0, SEED), p[0], i[0], f"{name} S={S}")


@pytest.mark.parametrize("N", [1, 3, 70])
def test_mixed_batches(N):
    pool = ["torus_64x40_degenerate", "empty", "chain_chunk_plus_1", "cube", "triangle", "torus_8x4", "chain_257"]
    names = [pool[k % len(pool)] for k in range(N)]
    p, i = sample(names, 257, device=DEV, scale=1.7)
    for n, name in enumerate(names):
        v, f = mr.mesh(name)
        mr.check_samples(v, f, mr.oracle(v, f, n, 257, SEED, 1.7), p[n], i[n], f"batch of {N}, mesh {n} ({name})")


@pytest.mark.parametrize("name", mr.SMALL)
def test_agrees_with_the_fallback(name):
    """The same faces as the CPU fallback wherever the oracle's t is farther than tau from every CDF boundary, and points within
    condition C of the fallback's face (checked against the float64 combination for the kernel's own face by check_samples)."""
    v, f = mr.mesh(name)
    o = mr.oracle_named(name, 0, SEED)
    pg, ig = sample([name], mr.S_MAX, device=DEV)
    pc, ic = sample([name], mr.S_MAX)
    if not o["A"] > 0:
        assert np.array_equal(pg, pc) and np.array_equal(ig, ic)
        return
    far = ~mr.near_boundary(o)
    assert far.mean() >= 0.99
    assert np.array_equal(ig[0][far], ic[0][far])
    same = ig[0] == ic[0]
    m = np.abs(o["vs"][f[ic[0]]].astype(np.float64)).max(axis=(1, 2))
    err = np.abs(pg[0].astype(np.float64) - pc[0].astype(np.float64)).max(axis=1)
    print(f"{name}: {same.mean():.4f} of the faces equal, worst point difference {np.max(err[same] / m[same]) / 2.0 ** -24:.2f} x 2^-24 m")
    assert (err[same] <= 16 * 2.0 ** -24 * m[same]).all()


def test_bit_identical_over_two_runs_and_stream_properties():
    from tricolo_amd import ops
    names = ["torus_200x100", "cube", "chain_chunk_plus_1"]
    verts, faces, voff, foff, mf = packed(names)
    runs = []
    for _ in range(2):
        cdf, total = ops.mesh_face_cdf(verts, faces, voff, foff, None, mf)
        p, i = ops.mesh_sample_points(verts, faces, voff, foff, cdf, total, 10000, SEED, None, True)
        runs.append((cdf, total, p, i))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    _, _, p, i = runs[0]
    alone, ialone = sample(["torus_200x100"], 10000, device=DEV)                   # the same mesh at n = 0 without the others
    assert np.array_equal(alone[0], p[0].cpu().numpy()) and np.array_equal(ialone[0], i[0].cpu().numpy())
    other, _ = sample(["cube"], 10000, device=DEV)                                 # the cube sat at n = 1 there
    assert not np.array_equal(other[0], p[1].cpu().numpy())
    short, ishort = sample(names, 100, device=DEV)
    assert np.array_equal(short, p[:, :100].cpu().numpy()) and np.array_equal(ishort, i[:, :100].cpu().numpy())
    p1025, _ = sample(names, 1025, device=DEV)                                     # one sample into a second workgroup
    assert np.array_equal(p1025, p[:, :1025].cpu().numpy())


def test_bbox_against_amin_amax():
    from tricolo_amd import ops
    rng = np.random.default_rng(3)
    clouds = [rng.standard_normal((n, 3)).astype(np.float32) * 5 for n in (1, 63, 257, 1000, 4099)]
    v, f = mr.mesh("two_1_3")                                                      # vertex 4 is referenced by no face
    clouds.append(v)
    off = np.concatenate([[0], np.cumsum([c.shape[0] for c in clouds])])
    bbox = ops.mesh_bbox(torch.from_numpy(np.concatenate(clouds)).to(DEV), torch.from_numpy(off).to(DEV)).cpu().numpy()
    for n, c in enumerate(clouds):
        assert np.array_equal(bbox[n, :, 0], c.min(0)) and np.array_equal(bbox[n, :, 1], c.max(0))
    assert bbox[-1, 2, 1] == 2.0


def test_face_cdf_against_numpy_cumsum():
    from tricolo_amd import ops
    names = ["torus_200x100", "empty", "chain_chunk_minus_1", "chain_chunk", "chain_chunk_plus_1", "torus_64x40_degenerate", "triangle"]
    verts, faces, voff, foff, mf = packed(names)
    scale = torch.tensor([1.0, 1.0, 0.5, 2.0, 3.0, 1.0, 7.0], device=DEV)
    cdf, total = ops.mesh_face_cdf(verts, faces, voff, foff, scale, mf)
    cdf2, total2 = ops.mesh_face_cdf(verts, faces, voff, foff, scale)              # the grid hint read from face_off instead
    assert torch.equal(cdf, cdf2) and torch.equal(total, total2)
    cdf, total, foff = cdf.cpu().numpy(), total.cpu().numpy(), foff.cpu().numpy()
    for n, name in enumerate(names):
        v, f = mr.mesh(name)
        got = cdf[foff[n]:foff[n + 1]]
        if f.shape[0] == 0:
            assert total[n] == 0.0
            continue
        area = mr.areas32(mr.scaled_verts(v, float(scale[n])), f)
        want = np.cumsum(area.astype(np.float64))
        print(f"{name}: worst CDF difference {np.abs(got - want).max() / want[-1]:.3e} of the total (bound 2^-40 = {2.0 ** -40:.3e})")
        assert np.abs(got - want).max() <= 2.0 ** -40 * want[-1]
        assert got[-1] == total[n]
        assert (np.diff(got) >= 0).all()
        assert np.array_equal(np.diff(got) == 0, area[1:] == 0)                    # a face of area 0 repeats its predecessor, no other does


def test_compare_meshes_on_the_device():
    from tricolo_amd.evaluation import mesh as M
    from tricolo_amd.evaluation import shape_f1 as sf
    cube = tmesh("cube")
    f1 = M.compare_meshes([cube], cube, num_samples=10000, scale="gt-10", seed=(3, 4), device=DEV)["F1@0.100000"]
    v, f = mr.mesh("cube")
    a, b = mr.oracle(v, f, 0, 10000, 3, 10.0), mr.oracle(v, f, 0, 10000, 4, 10.0)                   # the cube's longest edge is 1
    want = sf.f1_score(torch.from_numpy(a["points"].astype(np.float32))[None], torch.from_numpy(b["points"].astype(np.float32))[None])
    print("cube against itself, seeds 3 / 4: F1", float(f1[0]), "oracle", float(want[0]))
    assert float(f1[0]) > float(want[0]) - 0.5
    moved = (cube[0] + 5.0, cube[1])
    assert float(M.compare_meshes([moved], cube, num_samples=10000, device=DEV)["F1@0.100000"][0]) < 100.0


def test_rejected_inputs():
    from tricolo_amd import ops
    from tricolo_amd.evaluation import mesh as M
    verts, faces, voff, foff, mf = packed(["cube", "torus_8x4"])
    cdf, total = ops.mesh_face_cdf(verts, faces, voff, foff)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.mesh_bbox(verts.cpu(), voff)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.mesh_face_cdf(verts, faces.cpu(), voff, foff)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.mesh_sample_points(verts, faces, voff, foff, cdf.cpu(), total, 10)
    wide = torch.zeros((verts.shape[0], 4), device=DEV)[:, :3]
    with pytest.raises(ValueError, match="contiguous"):
        ops.mesh_bbox(wide, voff)
    with pytest.raises(ValueError, match="contiguous"):
        ops.mesh_face_cdf(verts, faces.t().contiguous().t(), voff, foff)
    with pytest.raises(ValueError, match="int32"):
        ops.mesh_face_cdf(verts, faces.long(), voff, foff)
    with pytest.raises(ValueError, match="int32"):
        ops.mesh_sample_points(verts, faces.long(), voff, foff, cdf, total, 10)
    v, f = tmesh("cube")
    with pytest.raises(ValueError, match="span"):                                  # caught on the host, before any launch
        M.sample_points_from_meshes([v], [f + 1], 10, device=DEV)
    out = M.sample_points_from_meshes([v, v], [f, f], 0, device=DEV)
    assert out.shape == (2, 0, 3) and out.is_cuda


def test_nearest_jsonl_from_obj_files_on_the_device(tmp_path):
    r, *_ = run_end_to_end(tmp_path / "gpu", DEV)
    c, *_ = run_end_to_end(tmp_path / "cpu", torch.device("cpu"))
    assert np.array_equal(np.float32(r["f1"]), np.float32(c["f1"]))
