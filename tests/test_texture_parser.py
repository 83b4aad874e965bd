"""CPU: tricolo_amd.data.materials.load_obj_textured - `vt` lines, the f tokens i/j, i/j/k and i//k, negative vt indices, polygon
fans, map_Kd lines with options and backslashes, images of every PIL mode, missing files, shared files, the size reduction - and
python -m tricolo_amd.data.preprocess --textures on, end to end on the host beside the default run."""
import os

import numpy as np
import pytest
import torch

pytest.importorskip("PIL")
from PIL import Image  # noqa: E402

from tests import test_preprocess as tp  # noqa: E402
from tricolo_amd import config as tcfg  # noqa: E402
from tricolo_amd.data import preprocess as pp  # noqa: E402
from tricolo_amd.data.materials import load_obj_materials, load_obj_textured, load_texture  # noqa: E402

OBJ = """mtllib scene.mtl
v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
v 0.5 1.5 0
vt 0 0
vt 1 0 0.5
vt 1 1
f 1/1 2/2 3/3
usemtl wood
vt 0 1
f 1/1/1 2/2/1 3/3/1 4/4/1
usemtl cloth
vt 0.5 1.5
f 1/-5 2/-4 3/-3 5/-1 4/-2
usemtl grey
f 1//1 2//1 3//1
f 1 2 3
f 1/1 2/2 3
usemtl gone
f 1/1 2/2 3/9
f 1/1 2/2 3/3
usemtl twin
f 3/3 2/2 1/1
"""
MTL = """newmtl wood
Kd 0.8 0.6 0.4
map_Kd -s 1 1 1 ..\\images\\t.png
newmtl cloth
Kd 1 1 1
map_Kd grey.png
newmtl grey
Kd 0.3 0.3 0.3
newmtl gone
map_Kd nowhere.jpg
newmtl twin
map_Kd ../images/t.png
newmtl rgba
map_Kd -clamp on rgba.png
"""


def write_scene(root):
    d = root / "models"
    os.makedirs(d)
    os.makedirs(root / "images")
    (d / "m.obj").write_text(OBJ)
    (d / "scene.mtl").write_text(MTL)
    g = np.random.default_rng(5)
    rgb = g.integers(0, 256, (3, 5, 3), dtype=np.uint8)
    Image.fromarray(rgb).save(root / "images" / "t.png")
    grey = g.integers(0, 256, (4, 2), dtype=np.uint8)
    Image.fromarray(grey).save(d / "grey.png")
    rgba = g.integers(0, 256, (2, 2, 4), dtype=np.uint8)
    Image.fromarray(rgba).save(d / "rgba.png")
    return str(d / "m.obj"), rgb, grey, rgba


def test_load_obj_textured(tmp_path):
    path, rgb, grey, rgba = write_scene(tmp_path)
    verts, faces, fm, kd, names, uv, mat_tex, textures, warnings = load_obj_textured(path)
    plain = load_obj_materials(path)
    assert torch.equal(verts, plain[0]) and torch.equal(faces, plain[1]) and torch.equal(fm, plain[2]) and torch.equal(kd, plain[3]) and names == plain[4]
    assert names == [None, "wood", "cloth", "grey", "gone", "twin", "rgba"]
    assert uv.shape == (12, 3, 2) and uv.dtype == torch.float32 and mat_tex.dtype == torch.int32
    vt = {1: [0, 0], 2: [1, 0], 3: [1, 1], 4: [0, 1], 5: [0.5, 1.5]}
    assert fm.tolist() == [0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 5]
    assert uv[0].tolist() == [vt[1], vt[2], vt[3]]                                       # v/vt, before any usemtl
    assert uv[1].tolist() == [vt[1], vt[2], vt[3]] and uv[2].tolist() == [vt[1], vt[3], vt[4]]           # v/vt/vn, a quad
    assert [r.tolist() for r in uv[3:6]] == [[vt[1], vt[2], vt[3]], [vt[1], vt[3], vt[5]], [vt[1], vt[5], vt[4]]]    # negative indices, a pentagon fan
    assert torch.isnan(uv[6:10]).all()                                                   # v//vn, v, one corner without, an index beyond the vt lines
    assert uv[10].tolist() == [vt[1], vt[2], vt[3]] and uv[11].tolist() == [vt[3], vt[2], vt[1]]
    # wood and twin share one file (loaded once), cloth is greyscale, gone's file is missing, rgba is used by no face but loads all the same
    assert mat_tex.tolist() == [-1, 0, 1, -1, -1, 0, 2] and len(textures) == 3
    assert len(warnings) == 1 and "nowhere.jpg" in warnings[0]
    assert all(t.dtype == np.uint8 and t.shape[2] == 4 and (t[:, :, 3] == 255).all() for t in textures)
    assert np.array_equal(textures[0][:, :, :3], rgb) and textures[0].shape == (3, 5, 4)                  # row 0 is the top row of the image
    assert np.array_equal(textures[1][:, :, :3], np.repeat(grey[:, :, None], 3, 2))
    assert np.array_equal(textures[2][:, :, :3], rgba[:, :, :3])
    (tmp_path / "models" / "grey.png").write_bytes(b"not an image")
    again = load_obj_textured(path)
    assert again[6].tolist() == [-1, 0, -1, -1, -1, 0, 1] and len(again[8]) == 2 and len(again[7]) == 2   # unreadable: a warning, never an exception


def test_large_textures_are_reduced(tmp_path):
    g = np.random.default_rng(6)
    big = g.integers(0, 256, (300, 600, 3), dtype=np.uint8)                              # 600 wide, 300 high
    Image.fromarray(big).save(tmp_path / "big.png")
    tex = load_texture(str(tmp_path / "big.png"), 256)
    assert tex.shape == (100, 200, 4)                                                    # (H, W) after the box factor 3
    want = big.reshape(100, 3, 200, 3, 3).astype(np.float64).mean((1, 3))
    assert np.abs(tex[:, :, :3].astype(np.float64) - want).max() <= 1.0
    assert load_texture(str(tmp_path / "big.png"), 600).shape == (300, 600, 4) and load_texture(str(tmp_path / "big.png"), 599).shape == (150, 300, 4)
    pal = Image.fromarray(big[:8, :8]).convert("P", palette=Image.ADAPTIVE, colors=16)
    pal.save(tmp_path / "pal.png")
    assert np.array_equal(load_texture(str(tmp_path / "pal.png"))[:, :, :3], np.asarray(pal.convert("RGB")))


# ---------------------------------------------------------------------------------------------------- the command line
def textured_model(obj_root, cat, mid):
    """Give write_model's chair texture coordinates, a map_Kd on its `top` material and the image one directory up."""
    d = os.path.join(obj_root, cat, mid, "models")
    with open(os.path.join(d, "model_normalized.obj")) as f:
        obj = f.read()
    obj = obj.replace("usemtl top\nf 1 2 3 4\n", "vt 0 0\nvt 2 0\nvt 2 2\nvt 0 2\nusemtl top\nf 1/1 2/2 3/3 4/4\n")
    assert "f 1/1" in obj
    with open(os.path.join(d, "model_normalized.obj"), "w") as f:
        f.write(obj)
    with open(os.path.join(d, "model_normalized.mtl"), "a") as f:
        f.write("newmtl extra\nmap_Kd missing.png\n")
    with open(os.path.join(d, "model_normalized.mtl")) as f:
        mtl = f.read()
    with open(os.path.join(d, "model_normalized.mtl"), "w") as f:
        f.write(mtl.replace("newmtl side", "map_Kd ../images/texture0.png\nnewmtl side"))
    os.makedirs(os.path.join(obj_root, cat, mid, "images"))
    Image.fromarray(np.random.default_rng(2).integers(0, 256, (6, 4, 3), dtype=np.uint8)).save(os.path.join(obj_root, cat, mid, "images", "texture0.png"))


def test_preprocess_with_textures_end_to_end(tmp_path):
    """Two models, chairA textured and tableB not, voxels from the meshes: --textures on changes chairA's images and grids and
    leaves tableB's exactly as the default run writes them."""
    runs = {}
    for mode in ("off", "on"):
        root = str(tmp_path / mode)
        overrides = [o for o in tp.write_dataset(root) if not o.startswith("data.ignored_models")]
        overrides.append("data.ignored_models=[04379243/ignoredD,03001627/chairC]")
        textured_model(os.path.join(root, "text2shape-data", "ShapeNetCore.v2"), *tp.MODELS[0])
        logged = []
        stats = pp.main(overrides + ["--device", "cpu", "--voxels", "mesh"] + (["--textures", "on"] if mode == "on" else []), log=logged.append)
        extra = {"textured_models": 1, "texture_failures": 1} if mode == "on" else {}        # chairA; its missing.png
        assert stats["train"] == {"models": 2, "written": 2, "skipped": 0, **extra}
        assert any("map_Kd" in line for line in logged) == (mode == "on")
        exp = tcfg.compose(overrides=overrides).data.exp_data_root_path
        runs[mode] = {m: dict(np.load(os.path.join(exp, c, f"{m}.npz"))) for c, m in tp.MODELS[:2]}
    for name in ("images", "voxel32", "voxel64", "voxel128"):
        assert np.array_equal(runs["on"]["tableB"][name], runs["off"]["tableB"][name]), name
        assert runs["on"]["chairA"][name].shape == runs["off"]["chairA"][name].shape
        assert not np.array_equal(runs["on"]["chairA"][name], runs["off"]["chairA"][name]), name
    assert np.array_equal(runs["on"]["chairA"]["voxel32"][3], runs["off"]["chairA"]["voxel32"][3])       # the same occupancy, other colours
