"""CPU: the host pieces of tricolo_amd.data.preprocess (cameras, materials, NRRD, caption mapping, packing) and the torch
restatement of csrc/raster.hip (ops.render_views on CPU tensors): exact coverage under the top-left rule, and its visibility buffer
against the float64 brute force of tests/raster_reference.py on the scenes the GPU tests use.

The brute force tests every face against every pixel, so the procedural mesh is compared where that stays quick: the full
19,860-face mesh in one view at 48 x 48, and its 1,360-face version in one view at 160 x 160.  The full mesh in all 12 views at
224 x 224 (1.2e10 face-pixel tests, ten minutes) was run once by hand: 4 ambiguous of 388,268 covered pixels, equal elsewhere."""
import gzip
import json
import math
import os
import pickle

import numpy as np
import pytest
import torch

from tests import raster_reference as rr
from tricolo_amd import config as tcfg
from tricolo_amd import ops
from tricolo_amd.data import render as R
from tricolo_amd.data.materials import load_obj_materials
from tricolo_amd.data.nrrd import read_nrrd
from tricolo_amd.data import preprocess as pp


# ---------------------------------------------------------------------------------------------------- cameras
def test_camera_poses():
    c = np.array([0.1, -0.2, 0.05])
    eye, rot = R.camera_poses(c, 12)
    assert eye.shape == (12, 3) and rot.shape == (12, 3, 3) and eye.dtype == np.float64
    v0 = 0.85 * np.array([0.0, math.sin(math.pi / 5), math.cos(math.pi / 5)])
    np.testing.assert_allclose(eye[0], c + v0, atol=1e-14)
    np.testing.assert_allclose(eye[3], c + np.array([v0[2], v0[1], 0.0]), atol=1e-14)          # a quarter turn about +y: z -> x
    fx, fy = R.projection_scales(224, 224, R.YFOV)
    for k in range(12):
        np.testing.assert_allclose(rot[k] @ rot[k].T, np.eye(3), atol=1e-14)
        assert abs(np.linalg.det(rot[k]) - 1.0) < 1e-14
        np.testing.assert_allclose(rot[k][2], (eye[k] - c) / 0.85, atol=1e-14)                   # the camera's +z points back at the eye
        p = rot[k] @ (c - eye[k])
        np.testing.assert_allclose(p, [0.0, 0.0, -0.85], atol=1e-14)
        assert abs((fx * p[0] / -p[2] + 1) * 112 - 112.0) < 1e-12 and abs((1 - fy * p[1] / -p[2]) * 112 - 112.0) < 1e-12   # the image centre
    cam = R.pack_cameras([c], 12)
    assert cam.shape == (1, 12, 12) and cam.dtype == torch.float32
    np.testing.assert_array_equal(cam[0, :, :3].numpy(), eye.astype(np.float32))
    np.testing.assert_array_equal(cam[0, :, 3:].numpy(), rot.reshape(12, 9).astype(np.float32))


# ---------------------------------------------------------------------------------------------------- coverage
FLAT_YFOV = math.pi / 2                              # f = 1: a vertex at z = 0 seen from (0, 0, 1) lands on xs = (x + 1) W / 2 exactly
FLAT_CAM = torch.tensor([[[0.0, 0.0, 1.0, 1, 0, 0, 0, 1, 0, 0, 0, 1]]], dtype=torch.float32)


def flat_vertices(points, H, W):
    """Screen positions (multiples of 1/256 pixel) -> world vertices at z = 0 that project exactly there."""
    p = np.asarray(points, dtype=np.float64)
    return torch.from_numpy(np.stack([p[:, 0] / (W / 2) - 1.0, 1.0 - p[:, 1] / (H / 2), np.zeros(len(p))], 1).astype(np.float32))


def flat_coverage(meshes, H=16, W=16, device="cpu"):
    """meshes: [(screen points, faces)] -> bool [N, H, W], each mesh seen by the flat camera."""
    from tricolo_amd.evaluation.mesh import pack_meshes
    verts, faces, voff, foff, _ = pack_meshes([flat_vertices(p, H, W) for p, _ in meshes],
                                              [torch.tensor(f, dtype=torch.int64).reshape(-1, 3) for _, f in meshes], device)
    N = len(meshes)
    fm = torch.zeros((faces.shape[0],), dtype=torch.int32, device=device)
    kd = torch.full((N, 3), 0.5, dtype=torch.float32, device=device)
    moff = torch.arange(N + 1, dtype=torch.int64, device=device)
    img, vis = ops.render_views(verts, faces, voff, foff, fm, kd, moff, FLAT_CAM.expand(N, 1, 12).contiguous().to(device), H, W, FLAT_YFOV,
                                0.05, return_visibility=True)
    assert ((img[:, 0, 0] != 255) == (vis[:, 0] >= 0)).all()
    return (vis[:, 0] >= 0).cpu().numpy()


QUADS = {"axis aligned": [(3, 2), (11, 2), (11, 9), (3, 9)], "turned": [(2, 5), (9, 1), (13, 8), (6, 13)], "thin": [(1, 1), (14, 3), (14.5, 4), (1.5, 2)]}
OFFSETS = [(0.0, 0.0), (0.5, 0.5), (1 / 256, 3 / 256), (0.25, 0.75), (0.5, 0.0)]      # (0.5, 0.5): integer corners sit ON pixel centres


def check_quad_splits(device="cpu"):
    for name, quad in QUADS.items():
        for ox, oy in OFFSETS:
            for flip in (False, True):                                                   # both windings
                q = [(x + ox, y + oy) for x, y in (quad[::-1] if flip else quad)]
                cov = flat_coverage([(q, [(0, 1, 2)]), (q, [(0, 2, 3)]), (q, [(1, 2, 3)]), (q, [(1, 3, 0)]), (q, [(0, 1, 2), (0, 2, 3)])], device=device)
                what = f"{name} quad, offset ({ox}, {oy}), flipped {flip}"
                assert not (cov[0] & cov[1]).any() and not (cov[2] & cov[3]).any(), what  # no pixel twice, along either diagonal
                assert np.array_equal(cov[0] | cov[1], cov[2] | cov[3]), what             # and none lost: both splits cover the same set
                assert np.array_equal(cov[0] | cov[1], cov[4]) and cov[4].sum() > 0, what
                if name == "axis aligned":                                                # top and left edges in, bottom and right out
                    ys, xs = np.nonzero(cov[4])
                    cx, cy = xs + 0.5, ys + 0.5
                    want = np.zeros((16, 16), bool)
                    for py in range(16):
                        for px in range(16):
                            want[py, px] = 3 + ox <= px + 0.5 < 11 + ox and 2 + oy <= py + 0.5 < 9 + oy
                    assert np.array_equal(cov[4], want), what


def check_empty_faces(device="cpu"):
    between = [(2.6, 2.6), (3.4, 2.6), (2.6, 3.4)]                                       # no pixel centre inside: (2.5, 2.5) and (3.5, 3.5) are out
    line = [(1, 1), (5, 5), (9, 9)]
    twice = [(2, 2), (9, 3), (9, 3)]
    cov = flat_coverage([(between, [(0, 1, 2)]), (line, [(0, 1, 2)]), (twice, [(0, 1, 2)])], device=device)
    assert not cov.any()


def test_quad_splits_cover_every_pixel_once():
    check_quad_splits()


def test_faces_without_a_pixel_centre_or_an_area_cover_nothing():
    check_empty_faces()


# ---------------------------------------------------------------------------------------------------- the independent reference
def render_scene(verts, faces, face_mat, kd, views, H, W, device="cpu", pick=None):
    """-> (image, vis, cam) of one mesh; pick: the views of the `views`-camera ring to render."""
    cam = R.pack_cameras([R.bbox_center(verts)], views)
    if pick is not None:
        cam = cam[:, pick].contiguous()
    from tricolo_amd.evaluation.mesh import pack_meshes
    v, f, voff, foff, _ = pack_meshes([verts], [faces], device)
    fm, k, moff = R.pack_materials([face_mat], [kd], device)
    img, vis = ops.render_views(v, f, voff, foff, fm, k, moff, cam.to(device), H, W, return_visibility=True)
    return img[0], vis[0], cam[0]


def soup_scene(device="cpu"):
    verts, faces = rr.soup()
    g = np.random.default_rng(3)
    return render_scene(verts, faces, torch.from_numpy(g.integers(0, 3, faces.shape[0]).astype(np.int32)),
                        torch.from_numpy(g.uniform(0, 1, (3, 3)).astype(np.float32)), 3, 32, 48, device) + (verts, faces)


def test_fallback_matches_the_brute_force():
    """Visibility equal to the float64 brute force on every pixel whose two nearest depths differ by 1e-5 relative or more; such
    pixels are at most 1 % of the covered ones in every scene (asserted by rr.compare).  The counts are printed; by hand, 19,860 faces in 12 views at
    224 x 224: 4 of 388,268."""
    img, vis, cam, verts, faces = soup_scene()
    amb, cov = rr.compare(vis, verts, faces, cam, 32, 48, "soup")
    assert cov > 100
    for rings, S, view in ((100, 48, 0), (26, 160, 1)):
        pv, pf, pm, pk = rr.procedural_mesh(rings)
        img, vis, cam = render_scene(pv, pf, pm, pk, 12, S, S, pick=[view])
        amb, cov = rr.compare(vis, pv, pf, cam, S, S, f"procedural mesh, {pf.shape[0]} faces, view {view} at {S} x {S}")
        assert cov > 0.2 * S * S


def test_soup_holds_what_the_gpu_test_needs():
    verts, faces = rr.soup()
    cam = R.pack_cameras([R.bbox_center(verts)], 3)[0]
    big = dropped = 0
    for k in range(3):
        keep, X, Y, d, A2 = R.project_faces(verts, faces, cam[k], 32, 48, R.YFOV, R.ZNEAR)
        bw = ((X.amax(1) - 128) >> 8).clamp(max=47) - ((X.amin(1) + 127) >> 8).clamp(min=0)
        bh = ((Y.amax(1) - 128) >> 8).clamp(max=31) - ((Y.amin(1) + 127) >> 8).clamp(min=0)
        big = max(big, int((keep & (bw >= 0) & (bh >= 0) & ((bw >= 8) | (bh >= 8))).sum()))
        assert int((~keep).sum()) >= 2                                                   # the two zero-area faces at least
        off = keep & ((bw < 0) | (bh < 0))
        dropped += int(off.sum())
        assert not keep[12] and not keep[13]
    assert big >= 2 and dropped > 0                                                      # the queue path runs; faces off screen or between centres


def test_render_views_refuses_bad_input_before_running():
    verts, faces = rr.soup()
    from tricolo_amd.evaluation.mesh import pack_meshes
    v, f, voff, foff, _ = pack_meshes([verts], [faces])
    fm, kd, moff = R.pack_materials([torch.zeros(200, dtype=torch.int32)], [torch.ones(1, 3)])
    cam = R.pack_cameras([np.zeros(3)], 2)
    with pytest.raises(ValueError, match="2\\^31 pixels"):
        ops.render_views(v, f, voff, foff, fm, kd, moff, cam, 40000, 40000)
    with pytest.raises(ValueError, match="cam"):
        ops.render_views(v, f, voff, foff, fm, kd, moff, cam[0], 8, 8)
    with pytest.raises(ValueError, match="face_mat"):
        ops.render_views(v, f, voff, foff, fm[:5], kd, moff, cam, 8, 8)
    with pytest.raises(ValueError, match="material indices"):
        R.pack_materials([torch.ones(3, dtype=torch.int32)], [torch.ones(1, 3)])


# ---------------------------------------------------------------------------------------------------- materials
OBJ = """mtllib scene.mtl missing.mtl
v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
v 0.5 1.5 0
f 1 2 3
usemtl red
f 1/1/1 2/2/1 3/3/1 4/4/1
usemtl blue
f 1//1 2//1 3//1 5//1 4//1
usemtl nobody_defined_this
f 3 5 4
"""
MTL = """newmtl red
Ka 0 0 0
Kd 0.8 0.1 0.05
map_Kd texture.jpg
newmtl unused
Kd 0.3 0.3 0.3
newmtl blue
Kd 0.0 0.25 1.0
"""


@pytest.mark.parametrize("newline", ["\n", "\r\n"], ids=["lf", "crlf"])
def test_obj_materials(tmp_path, newline):
    (tmp_path / "m.obj").write_bytes(OBJ.replace("\n", newline).encode())
    (tmp_path / "scene.mtl").write_bytes(MTL.replace("\n", newline).encode())
    verts, faces, fm, kd, names = load_obj_materials(str(tmp_path / "m.obj"))
    assert verts.shape == (5, 3) and faces.shape == (7, 3) and fm.dtype == torch.int32 and kd.dtype == torch.float32
    assert names == [None, "red", "unused", "blue"]
    assert fm.tolist() == [0, 1, 1, 3, 3, 3, 0]                                          # before any usemtl; quad; pentagon; unknown name
    assert faces[1:3].tolist() == [[0, 1, 2], [0, 2, 3]] and faces[3:6].tolist() == [[0, 1, 2], [0, 2, 4], [0, 4, 3]]
    np.testing.assert_array_equal(kd.numpy(), np.array([[0.4, 0.4, 0.4], [0.8, 0.1, 0.05], [0.3, 0.3, 0.3], [0.0, 0.25, 1.0]], np.float32))
    os.remove(tmp_path / "scene.mtl")                                                    # no MTL file at all: everything is material 0
    verts, faces, fm, kd, names = load_obj_materials(str(tmp_path / "m.obj"))
    assert fm.tolist() == [0] * 7 and kd.tolist() == [[pytest.approx(0.4)] * 3] and names == [None]


# ---------------------------------------------------------------------------------------------------- NRRD
def cell(V):
    c, x, y, z = np.meshgrid(np.arange(4), np.arange(V), np.arange(V), np.arange(V), indexing="ij")
    return ((c * 64 + x * 16 + y * 4 + z) % 251).astype(np.uint8)                        # a known function of (c, x, y, z), V = 4: all distinct


def write_nrrd(path, grid, encoding="raw", magic="NRRD0004", type_="uint8", dimension=None, sizes=None, crlf=False):
    dimension = grid.ndim if dimension is None else dimension
    sizes = " ".join(str(s) for s in grid.shape) if sizes is None else sizes
    head = [magic, "# written by the test", f"type: {type_}", f"dimension: {dimension}", "space: left-posterior-superior", f"sizes: {sizes}",
            "space directions: none (1,0,0) (0,1,0) (0,0,1)", f"encoding: {encoding}", "", ""]
    body = grid.tobytes(order="F")                                                       # the first axis runs fastest
    if encoding in ("gzip", "gz"):
        body = gzip.compress(body)
    with open(path, "wb") as f:
        f.write(("\r\n" if crlf else "\n").join(head).encode() + body)


def test_nrrd_reads_back_with_cxyz_indexing(tmp_path):
    want = cell(4)
    for k, (enc, type_, crlf) in enumerate([("raw", "uint8", False), ("gzip", "unsigned char", False), ("gz", "uchar", True)]):
        path = str(tmp_path / f"g{k}.nrrd")
        write_nrrd(path, want, enc, type_=type_, crlf=crlf)
        got = read_nrrd(path)
        assert got.dtype == np.uint8 and got.shape == (4, 4, 4, 4) and np.array_equal(got, want), enc
        assert got[2, 1, 3, 0] == (2 * 64 + 16 + 12) % 251
        assert np.array_equal(read_nrrd(path, 4), want)


def test_nrrd_rejects_what_it_does_not_support(tmp_path):
    path = str(tmp_path / "bad.nrrd")
    for field, kw in [("magic", {"magic": "NRRX0004"}), ("type", {"type_": "float"}), ("dimension", {"dimension": 3}), ("sizes", {"sizes": "3 4 4 4"}),
                      ("sizes", {"sizes": "4 4 4 5"}), ("encoding", {"encoding": "bzip2"})]:
        write_nrrd(path, cell(4), **kw)
        with pytest.raises(ValueError, match=f"bad.nrrd: {field}"):
            read_nrrd(path)
    write_nrrd(path, cell(4))
    with pytest.raises(ValueError, match="sizes"):
        read_nrrd(path, 32)                                                              # not the grid the caller asked for
    with open(path, "wb") as f:
        f.write(b"NRRD0004\ntype: uint8\ndimension: 4\nsizes: 4 4 4 4\nencoding: raw\n\n" + b"\0" * 100)
    with pytest.raises(ValueError, match="sizes"):
        read_nrrd(path)                                                                  # truncated data


# ---------------------------------------------------------------------------------------------------- captions, packing
WORDS = {str(i): w for i, w in enumerate(["<pad>", "a", "red", "chair", "round", "table\n", "wooden", "tall"])}
MODELS = [("03001627", "chairA"), ("04379243", "tableB"), ("03001627", "chairC"), ("04379243", "ignoredD")]
CAPTION_ROWS = [([1, 2, 3, 0, 0, 0], 0), ([1, 4, 5, 0, 0, 0], 1), ([7, 3, 0, 2, 0, 0], 0), ([1, 6, 5, 0, 0, 0], 3), ([6, 3, 0, 0, 0, 0], 2),
                ([1, 7, 6, 4, 5, 2], 1)]


def write_captions(dataset_path, split="train"):
    tuples = [(np.array(tok, dtype=np.int64), MODELS[m][0], MODELS[m][1] + ".nrrd") for tok, m in CAPTION_ROWS]
    os.makedirs(dataset_path, exist_ok=True)
    with open(os.path.join(dataset_path, f"processed_captions_{split}.p"), "wb") as f:
        pickle.dump({"caption_tuples": tuples}, f)
    with open(os.path.join(dataset_path, "shapenet.json"), "w") as f:
        json.dump({"idx_to_word": WORDS, "word_to_idx": {w: int(i) for i, w in WORDS.items()}}, f)


EXPECTED_MAP = [
    {"model_id": "chairA", "category": "03001627", "caption": "a red chair", "tokens": [1, 2, 3, 0, 0, 0]},
    {"model_id": "tableB", "category": "04379243", "caption": "a round table", "tokens": [1, 4, 5, 0, 0, 0]},
    {"model_id": "chairA", "category": "03001627", "caption": "tall chair", "tokens": [7, 3, 0, 2, 0, 0]},
    {"model_id": "chairC", "category": "03001627", "caption": "wooden chair", "tokens": [6, 3, 0, 0, 0, 0]},
    {"model_id": "tableB", "category": "04379243", "caption": "a tall wooden round table red", "tokens": [1, 7, 6, 4, 5, 2]},
]


def test_caption_mapping(tmp_path):
    root = str(tmp_path / "chair_table")
    write_captions(root)
    out = str(tmp_path / "out" / "train_map.json")
    keys = pp.create_model_id_caption_mapping(os.path.join(root, "processed_captions_train.p"), os.path.join(root, "shapenet.json"), out,
                                              ["04379243/ignoredD", "04379243/somebody_else"])
    assert keys == (("03001627", "chairA"), ("04379243", "tableB"), ("03001627", "chairC"))
    with open(out) as f:
        assert json.load(f) == EXPECTED_MAP
    assert pp.read_model_ids(out) == keys


def write_model(obj_root, data_root, cat, mid, k):
    """A tiny OBJ + MTL (a tilted quad over a triangle, two materials) and sparse NRRD grids at 32 / 64 / 128."""
    d = os.path.join(obj_root, cat, mid, "models")
    os.makedirs(d, exist_ok=True)
    s = 0.2 + 0.05 * k
    with open(os.path.join(d, "model_normalized.obj"), "w") as f:
        f.write(f"mtllib model_normalized.mtl\nv {-s} -0.1 {-s}\nv {s} -0.1 {-s}\nv {s} 0.1 {s}\nv {-s} 0.1 {s}\nv 0 0.3 0\n"
                "usemtl top\nf 1 2 3 4\nusemtl side\nf 1 2 5\n")
    with open(os.path.join(d, "model_normalized.mtl"), "w") as f:
        f.write(f"newmtl top\nKd 0.9 {0.2 * k} 0.1\nnewmtl side\nKd 0.1 0.5 0.8\n")
    g = np.random.default_rng(k)
    for V in pp.VOXEL_SIZES:
        grid = np.zeros((4, V, V, V), np.uint8)
        grid[:, 3:9, 2:7, 4:8] = g.integers(1, 255, (4, 6, 5, 4))
        os.makedirs(os.path.join(data_root, f"nrrd_256_filter_div_{V}_solid", mid), exist_ok=True)
        write_nrrd(os.path.join(data_root, f"nrrd_256_filter_div_{V}_solid", mid, f"{mid}.nrrd"), grid, "gzip")


def write_dataset(root, views=4, image_size=32):
    """The tree preprocess.main reads, three models and one ignored one -> the overrides that point a config at it."""
    dataset_path = os.path.join(root, "text2shape-data", "chair_table")
    for split in pp.SPLITS:
        write_captions(dataset_path, split)
    for k, (cat, mid) in enumerate(MODELS[:3]):
        write_model(os.path.join(root, "text2shape-data", "ShapeNetCore.v2"), dataset_path, cat, mid, k)
    return ["data=text2shape_chair_table", f"data.dataset_root_path={root}", f"data.num_views={views}", f"data.image_size={image_size}",
            "data.voxel_size=32", "data.batch_size=4", "data.ignored_models=[04379243/ignoredD]", "model.text_encoder=BiGRUEncoder",
            "model.image_encoder=MVCNNEncoder", "model.voxel_encoder=SparseCNNEncoder"]


def check_end_to_end(root, device):
    from tricolo_amd.data.dataset import PackedDataset
    overrides = write_dataset(root)
    dev = ["--device", device, "--batch-meshes", "2"]
    stats = pp.main(overrides + dev, log=lambda *a: None)
    assert stats == {s: {"models": 3, "written": 3 if s == "train" else 0, "skipped": 0 if s == "train" else 3} for s in pp.SPLITS}
    cfg = tcfg.compose(overrides=overrides)
    exp = cfg.data.exp_data_root_path
    with open(cfg.data.train_lang_data_path) as f:
        assert json.load(f) == EXPECTED_MAP
    files = sorted(os.path.join(c, n) for c in os.listdir(exp) if os.path.isdir(os.path.join(exp, c)) for n in os.listdir(os.path.join(exp, c)))
    assert files == ["03001627/chairA.npz", "03001627/chairC.npz", "04379243/tableB.npz"]                 # and no temporary file left
    meshes = [load_obj_materials(os.path.join(root, "text2shape-data", "ShapeNetCore.v2", c, m, "models", "model_normalized.obj")) for c, m in MODELS[:3]]
    want = R.render_meshes([m[0] for m in meshes], [m[1] for m in meshes], [m[2] for m in meshes], [m[3] for m in meshes], num_views=4, device=device)
    assert want.shape == (3, 4, 3, 224, 224) and (want != 255).any(dim=-1).any(dim=-1).all()
    for k, (c, m) in enumerate(MODELS[:3]):
        with np.load(os.path.join(exp, c, f"{m}.npz")) as z:
            assert sorted(z.files) == ["images", "voxel128", "voxel32", "voxel64"]
            assert z["images"].dtype == np.uint8 and np.array_equal(z["images"], want[k].cpu().numpy())
            for V in pp.VOXEL_SIZES:
                assert np.array_equal(z[f"voxel{V}"], read_nrrd(os.path.join(cfg.data.dataset_path, f"nrrd_256_filter_div_{V}_solid", m, f"{m}.nrrd")))
    ds = PackedDataset(cfg, "train", device=device)
    assert len(ds) == 5 and ds.shape_keys == [MODELS[0], MODELS[1], MODELS[2]]
    batch = next(iter(ds.batches(4)(0)))
    assert batch["model_id"] == ["chairA", "tableB", "chairA", "chairC"] and batch["tokens"].shape == (4, 6) and batch["tokens"].dtype == torch.int32
    assert batch["images"].shape == (4, 4, 3, 32, 32) and batch["images"].dtype == torch.uint8
    assert batch["voxels"]["rgba"].shape == (4, 4, 32, 32, 32) and batch["voxels"]["rgba"].dtype == torch.uint8
    assert torch.equal(batch["images"], ops.resize_bicubic_aa_u8(want, 32)[[0, 1, 0, 2]])
    mtimes = {f: os.stat(os.path.join(exp, f)).st_mtime_ns for f in files}
    again = pp.main(overrides + dev, log=lambda *a: None)
    assert all(v == {"models": 3, "written": 0, "skipped": 3} for v in again.values())                      # a second run writes nothing
    assert mtimes == {f: os.stat(os.path.join(exp, f)).st_mtime_ns for f in files}
    return overrides, cfg


def test_end_to_end_on_the_host(tmp_path):
    overrides, cfg = check_end_to_end(str(tmp_path), "cpu")
    os.remove(os.path.join(cfg.data.exp_data_root_path, "04379243", "tableB.npz"))                          # an interrupted run resumes
    stats = pp.main(overrides + ["--device", "cpu", "--jpeg-roundtrip"], log=lambda *a: None)
    assert stats["train"] == {"models": 3, "written": 1, "skipped": 2}
    with np.load(os.path.join(cfg.data.exp_data_root_path, "04379243", "tableB.npz")) as z, \
            np.load(os.path.join(cfg.data.exp_data_root_path, "03001627", "chairA.npz")) as clean:
        jpg = z["images"]
        assert jpg.shape == (4, 3, 224, 224) and jpg.dtype == np.uint8
        assert 0 < np.abs(jpg.astype(int) - 255).max() and (jpg[:, :, 0, 0] > 250).all()                    # decoded pixels, a white corner
        assert (clean["images"] != 255).any()
