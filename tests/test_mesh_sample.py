"""CPU: the mesh front half of the shape F1 (tricolo_amd.evaluation.mesh) without a GPU - Philox against the Random123 vectors,
load_obj on files written to tmp_path, the torch fallback under conditions A-D of tests/mesh_reference.py on every test mesh,
statistical checks of the specification itself, the stream properties, the scale rules, and nearest.jsonl from OBJ files to a mean F1."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import mesh_reference as mr

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 5                 # with this seed the float64 oracle passes the statistical checks below (any seed should, at 4 sigma)
KAT = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd")]


def tmesh(name):
    v, f = mr.mesh(name)
    return torch.from_numpy(v.copy()), torch.from_numpy(f.copy())


def sample(names, S, seed=SEED, device=None, **kw):
    from tricolo_amd.evaluation import mesh as M
    ms = [tmesh(n) for n in names]
    p, i = M.sample_points_from_meshes([m[0] for m in ms], [m[1] for m in ms], S, seed, return_face_idx=True, device=device, **kw)
    return p.cpu().numpy(), i.cpu().numpy()


# ------------------------------------------------------------------------------------------------ Philox
@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    from tricolo_amd.evaluation import mesh as M
    got = mr.philox4x32_10([np.array([c], dtype=np.uint64) for c in counter], key)
    assert " ".join("%08x" % int(w[0]) for w in got) == want
    got = M.philox4x32_10([torch.tensor([c], dtype=torch.int64) for c in counter], key)
    assert " ".join("%08x" % int(w[0]) for w in got) == want


def test_philox_fallback_equals_oracle_stream():
    from tricolo_amd.evaluation import mesh as M
    for n, seed in ((0, 0), (3, SEED), (69, 2 ** 40 + 17), (2 ** 20, 2 ** 64 - 1)):
        a, b = M._uniforms(n, 300, seed), mr.uniforms(n, 300, seed)
        for x, y in zip(a, b):
            assert np.array_equal(x.numpy().astype(np.float64), y)


# ------------------------------------------------------------------------------------------------ load_obj
def _obj(tmp_path, text, name="m.obj", newline=None):
    p = tmp_path / name
    with open(p, "w", newline="") as f:
        f.write(text if newline is None else text.replace("\n", newline))
    return str(p)


def test_load_obj_triangles(tmp_path):
    from tricolo_amd.evaluation import mesh as M
    v, f = mr.cube()
    p = str(tmp_path / "cube.obj")
    mr.write_obj(p, v, f)
    lv, lf = M.load_obj(p)
    assert lv.dtype == torch.float32 and lf.dtype == torch.int64
    assert np.array_equal(lv.numpy(), v) and np.array_equal(lf.numpy(), f)


def test_load_obj_polygons_token_forms_negative_indices_and_noise(tmp_path):
    from tricolo_amd.evaluation import mesh as M
    text = ("# a comment\nmtllib x.mtl\no thing\ng grp\n"
            "v 0 0 0\nv 1 0 0 0.5 0.5 0.5\nv 1 1 0\nvt 0.5 0.5\nvn 0 0 1\nv 0 1 0\nv 0.5 1.5 0\n"
            "usemtl m\ns off\n"
            "f 1 2 3 4\n"                          # a quad: (0, 1, 2), (0, 2, 3)
            "f 1/1 2/1 3/1\n"
            "f 1/1/1 2/1/1 4/1/1\n"
            "f 1//1 3//1 4//1\n"
            "f 1 2 3 5 4\n"                        # a pentagon: (0,1,2), (0,2,4), (0,4,3)
            "f -1 -2 -5\n"                         # five vertices read: 4, 3, 0
            "v 2 2 2\n"
            "f -1 1 2\n"                           # six vertices read: 5, 0, 1
            "\n")
    want = [[0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 1, 3], [0, 2, 3], [0, 1, 2], [0, 2, 4], [0, 4, 3], [4, 3, 0], [5, 0, 1]]
    for newline in (None, "\r\n"):
        v, f = M.load_obj(_obj(tmp_path, text, newline=newline))
        assert v.shape == (6, 3) and v[1].tolist() == [1.0, 0.0, 0.0] and v[5].tolist() == [2.0, 2.0, 2.0]      # the colours are dropped
        assert f.tolist() == want


def test_load_obj_rejects_indices_outside_the_vertices(tmp_path):
    from tricolo_amd.evaluation import mesh as M
    for bad in ("f 1 2 4", "f 1 2 0", "f 1 2 -4"):
        with pytest.raises(ValueError, match="line 5"):
            M.load_obj(_obj(tmp_path, "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n" + bad + "\n"))


def test_load_obj_without_faces(tmp_path):
    from tricolo_amd.evaluation import mesh as M
    v, f = M.load_obj(_obj(tmp_path, "v 0 0 0\nv 1 0 0\n"))
    assert v.shape == (2, 3) and f.shape == (0, 3) and f.dtype == torch.int64


# ------------------------------------------------------------------------------------------------ the fallback under A-D
@pytest.mark.parametrize("name", list(mr.MESHES))
def test_fallback_meets_the_conditions(name):
    v, f = mr.mesh(name)
    for S in mr.SAMPLE_COUNTS:
        p, i = sample([name], S)
        mr.check_samples(v, f, mr.oracle_named(name, 0, SEED), p[0], i[0], f"{name} S={S}")


def test_fallback_with_scale_meets_the_conditions():
    v, f = mr.mesh("torus_64x40_plus50")
    p, i = sample(["torus_64x40_plus50"], 257, scale=0.37)
    mr.check_samples(v, f, mr.oracle_named("torus_64x40_plus50", 0, SEED, 0.37), p[0], i[0], "scaled torus")


def test_specification_statistics_and_fallback_counts():
    """The float64 oracle alone (seed 5): the 1 : 3 mesh puts 2,500 +- 4 sigma samples on the small face, the samples of one triangle
    average to its centroid within 4 sigma / sqrt(S) per coordinate; then the fallback's face counts equal the oracle's."""
    o = mr.oracle_named("two_1_3", 0, SEED)
    small = int((o["face"] == 0).sum())
    print("samples on the small face:", small)
    assert abs(small - 2500) <= 4 * 43.3
    v, f = mr.mesh("triangle")
    o1 = mr.oracle_named("triangle", 0, SEED)
    centroid = v[f[0]].astype(np.float64).mean(0)
    sigma = o1["points"].std(0)
    dev = np.abs(o1["points"].mean(0) - centroid)
    print("centroid deviation / (sigma / sqrt S):", dev / (sigma / 100.0))
    assert (dev <= 4 * sigma / np.sqrt(mr.S_MAX)).all()
    for name, oo in (("two_1_3", o), ("triangle", o1)):
        _, i = sample([name], mr.S_MAX)
        assert np.array_equal(np.bincount(i[0], minlength=2), np.bincount(oo["face"], minlength=2))


@pytest.mark.parametrize("name", mr.SMALL)
def test_seed_leaves_few_samples_near_a_boundary(name):
    """The GPU agreement test compares face indices away from the CDF boundaries; with this seed at most 1 % of the samples lie nearer
    than tau to one (meshes up to 5,140 faces; at 40,000 faces the expected share is 2 F 2^-22 = 2 %)."""
    o = mr.oracle_named(name, 0, SEED)
    if o["A"] > 0:
        assert mr.near_boundary(o).mean() <= 0.01


# ------------------------------------------------------------------------------------------------ stream properties
def test_same_seed_same_bits_other_seed_other_points():
    a, ia = sample(["torus_8x4"], 257)
    b, ib = sample(["torus_8x4"], 257)
    c, _ = sample(["torus_8x4"], 257, seed=SEED + 1)
    assert np.array_equal(a, b) and np.array_equal(ia, ib) and not np.array_equal(a, c)


def test_batch_row_equals_the_mesh_alone_only_at_the_same_index():
    """Row (n, s) depends on (seed, n, s) and mesh n: a mesh sampled alone (n = 0) equals its row in a batch where it sits at n = 0,
    whatever follows it - and differs where it sits at another index."""
    alone, ialone = sample(["cube"], 300)
    first, ifirst = sample(["cube", "torus_64x40", "empty"], 300)
    last, _ = sample(["torus_64x40", "empty", "cube"], 300)
    assert np.array_equal(alone[0], first[0]) and np.array_equal(ialone[0], ifirst[0])
    assert not np.array_equal(alone[0], last[2])
    assert (first[2] == 0).all() and (ifirst[2] == -1).all()


def test_prefix_of_a_longer_run():
    long, ilong = sample(["torus_64x40"], 10000)
    short, ishort = sample(["torus_64x40"], 100)
    assert np.array_equal(long[0, :100], short[0]) and np.array_equal(ilong[0, :100], ishort[0])


def test_num_samples_zero_and_rejected_inputs():
    from tricolo_amd.evaluation import mesh as M
    v, f = tmesh("cube")
    assert M.sample_points_from_meshes([v, v], [f, f], 0).shape == (2, 0, 3)
    with pytest.raises(ValueError, match="span"):
        M.sample_points_from_meshes([v], [f + 1], 10)
    with pytest.raises(ValueError, match="span"):
        M.sample_points_from_meshes([v], [f - 1], 10)
    with pytest.raises(ValueError, match="float32"):
        M.sample_points_from_meshes([v.double()], [f], 10)
    with pytest.raises(ValueError, match="faces"):
        M.sample_points_from_meshes([v], [f.float()], 10)
    with pytest.raises(ValueError, match="Invalid scale"):
        M.sample_points_from_meshes([v], [f], 10, scale="pred-10")


# ------------------------------------------------------------------------------------------------ scale
def test_gt_scale_sees_unreferenced_vertices_and_number_equals_tensor():
    from tricolo_amd.evaluation import mesh as M
    v, f = tmesh("cube")
    v2 = torch.cat([v, torch.tensor([[4.0, 0.0, 0.0]])])                           # not referenced by any face: longest edge 4, not 1
    p = M.sample_points_from_meshes([v2], [f], 500, SEED, scale="gt-10")
    assert 2.4 < float(p.max()) <= 2.5 * (1 + 2.0 ** -20)                          # the cube's edge became 10 / 4 (fp32 weights: a few ulp)
    q = M.sample_points_from_meshes([v2], [f], 500, SEED, scale=2.5)
    r = M.sample_points_from_meshes([v2], [f], 500, SEED, scale=torch.tensor([2.5]))
    assert torch.equal(p, q) and torch.equal(q, r)
    g = M.sample_points_from_meshes([v2], [f], 500, SEED, scale="gt-10", gt=(v, f))      # the ground truth's box: edge 1 -> factor 10
    assert float(g.max()) > 9.5
    bbox = M.bounding_boxes([v2, v])
    assert bbox.shape == (2, 3, 2) and bbox[0, 0].tolist() == [0.0, 4.0] and bbox[1, 0].tolist() == [0.0, 1.0]


def test_compare_meshes_pair_semantics():
    from tricolo_amd.evaluation import mesh as M
    cube, torus = tmesh("cube"), tmesh("torus_8x4")
    m = M.compare_meshes([cube, torus], cube, num_samples=500, seed=(3, 4))
    f1 = m["F1@0.100000"]
    assert f1.shape == (2,) and float(f1[0]) > float(f1[1])
    moved = (cube[0] + 5.0, cube[1])
    assert float(M.compare_meshes([moved], cube, num_samples=500)["F1@0.100000"][0]) < 100.0


# ------------------------------------------------------------------------------------------------ end to end
def make_mesh_root(tmp_path):
    """cube and torus OBJ files under a mesh root, the category map as the reference's val_map.json, and a nearest.jsonl: record 0
    retrieves the ground truth itself, record 1 the other shape, record 2 names a shape with neither a cloud nor a mesh."""
    root = tmp_path / "ShapeNetCore.v2"
    cats = {"cubeid": "0001", "torusid": "0002"}
    for mid, name in (("cubeid", "cube"), ("torusid", "torus_8x4")):
        d = root / cats[mid] / mid / "models"
        os.makedirs(d)
        mr.write_obj(str(d / "model_normalized.obj"), *mr.mesh(name))
    val_map = tmp_path / "val_map.json"
    val_map.write_text(json.dumps([{"model_id": k, "category": v} for k, v in cats.items()] + [{"model_id": "ghost", "category": "0003"}]))
    nearest = tmp_path / "nearest.jsonl"
    recs = [{"groundtruth": "cubeid-0", "retrieved_models": ["cubeid", "torusid"]},
            {"groundtruth": "cubeid-1", "retrieved_models": ["torusid", "cubeid"]},
            {"groundtruth": "torusid-0", "retrieved_models": ["ghost", "cubeid"]}]
    nearest.write_text("".join(json.dumps(r) + "\n" for r in recs))
    return str(root), str(val_map), str(nearest), cats


def run_end_to_end(tmp_path, device):
    from tricolo_amd.evaluation import shape_f1 as sf
    root, val_map, nearest, cats = make_mesh_root(tmp_path)
    cache, S = str(tmp_path / "point_cache"), 700
    r = sf.shape_f1_from_nearest(nearest, cache, device=device, mesh_root=root, category_map=val_map, num_samples=S, seed=SEED)
    assert sorted(os.listdir(cache)) == ["cubeid.npy", "torusid.npy"]
    for mid in cats:
        a = np.load(os.path.join(cache, mid + ".npy"))
        assert a.shape == (1, S, 3) and a.dtype == np.float32
        assert abs((a[0].max(0) - a[0].min(0)).max() - 10.0) < 0.5                  # its own gt-10 factor: longest edge 10
    assert r["records"] == [0, 1] and r["skipped"] == 1
    assert r["f1"][0] == 100.0 and r["f1"][1] < 100.0
    again = sf.shape_f1_from_nearest(nearest, cache, device=device)                # from the cache alone
    assert again["f1"] == r["f1"] and again["skipped"] == 1
    asdict = sf.shape_f1_from_nearest(nearest, str(tmp_path / "cache2"), device=device, mesh_root=root, category_map=cats, num_samples=S,
                                      seed=SEED)
    assert asdict["f1"] == r["f1"]
    return r, root, val_map, nearest, cache


def test_nearest_jsonl_from_obj_files(tmp_path):
    r, root, val_map, nearest, cache = run_end_to_end(tmp_path, torch.device("cpu"))
    out = subprocess.run([sys.executable, "-m", "tricolo_amd.evaluation.shape_f1", nearest, "--point-cache", str(tmp_path / "cache3"),
                          "--mesh-root", root, "--category-map", val_map, "--num-samples", "700", "--seed", str(SEED)],
                         cwd=REPO_ROOT, capture_output=True, text=True, timeout=300, env=dict(os.environ, HIP_VISIBLE_DEVICES=""))
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    assert lines[0].startswith("skipped 1 of 3 records") and float(lines[-1]) == pytest.approx(r["mean_f1"], rel=1e-6)


def test_prefilled_cache_without_the_new_arguments_is_unchanged(tmp_path):
    """Without mesh_root the call reads the cache and nothing else: the values are compute_sampling_metrics' on the stored clouds."""
    from tricolo_amd.evaluation import shape_f1 as sf
    rng = np.random.default_rng(0)
    cache = tmp_path / "pc"
    os.makedirs(cache)
    a, b = rng.standard_normal((1, 300, 3)).astype(np.float32), rng.standard_normal((280, 3)).astype(np.float32) * 0.9
    np.save(cache / "a.npy", a), np.save(cache / "b.npy", b)
    nearest = tmp_path / "n.jsonl"
    nearest.write_text(json.dumps({"groundtruth": "a-0", "retrieved_models": ["b"]}) + "\n" +
                       json.dumps({"groundtruth": "a-1", "retrieved_models": ["c"]}) + "\n")
    r = sf.shape_f1_from_nearest(str(nearest), str(cache), threshold=0.3, device=torch.device("cpu"))
    want = sf.compute_sampling_metrics(torch.from_numpy(b)[None], torch.from_numpy(a), thresholds=(0.3,))["F1@0.300000"]
    assert r["f1"] == want.tolist() and r["skipped"] == 1 and sorted(os.listdir(cache)) == ["a.npy", "b.npy"]
