"""CPU: the host path of ops.resize_bicubic_aa_u8 against the float64 model of tests/resize_reference.py (and the measurement that
model's TAU rests on), torchvision's Resize(int) size rule, PackedDataset on a tiny packed tree (tricolo_amd/data/dataset.py against
an in-test restatement of general_dataset.py:47-54,79-93), and tricolo_amd.train.main reaching the dataset for the Text2Shape sets."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import resize_reference as rr
from tricolo_amd import config as tcfg
from tricolo_amd.data import synthetic as syn

N_VIEWS_ON_DISK, SRC, N_VIEWS, IMAGE_SIZE, VOXEL = 12, 24, 5, 17, 32
# (category, model id) of the 11 captions: 5 shapes in 2 categories, cat_a/m0 captioned three times, non-contiguously
CAPTIONS = [("cat_a", "m0"), ("cat_b", "m1"), ("cat_a", "m0"), ("cat_a", "m2"), ("cat_b", "m3"), ("cat_b", "m1"), ("cat_a", "m0"),
            ("cat_b", "m4"), ("cat_a", "m2"), ("cat_b", "m3"), ("cat_b", "m4")]
SHAPES = [("cat_a", "m0"), ("cat_b", "m1"), ("cat_a", "m2"), ("cat_b", "m3"), ("cat_b", "m4")]          # order of first occurrence
TOKEN_LEN = 12


def write_tree(root, src=SRC):
    """The packed layout of data/preprocess_all_data.py:85-106 under `root`; returns {(cat, mid): (grid, images)} and the token rows."""
    rng = np.random.default_rng(77)
    shapes = {}
    for cat, mid in SHAPES:
        grid = syn.make_voxel_grid_u8(rng, VOXEL)
        imgs = syn.make_images_u8(rng, N_VIEWS_ON_DISK, src)
        os.makedirs(os.path.join(root, cat), exist_ok=True)
        np.savez(os.path.join(root, cat, f"{mid}.npz"), **{f"voxel{VOXEL}": grid, "images": imgs})
        shapes[(cat, mid)] = (grid, imgs)
    tokens = []
    for split in ("train", "val"):
        items = []
        for k, (cat, mid) in enumerate(CAPTIONS):
            tok = np.zeros(TOKEN_LEN, dtype=np.int64)
            n = 3 + k % 7
            tok[:n] = rng.integers(1, syn.DEFAULT_VOCAB, size=n)
            items.append({"model_id": mid, "category": cat, "tokens": [int(t) for t in tok], "caption": f" caption {k} of {mid} "})
            if split == "train":
                tokens.append(tok.astype(np.int32))
        with open(os.path.join(root, f"{split}_map.json"), "w") as f:
            json.dump(items, f)
    return shapes, np.stack(tokens)


def tree_overrides(root, image_size=IMAGE_SIZE):
    return ["data=text2shape_chair_table", f"data.exp_data_root_path={root}", f"data.train_lang_data_path={root}/train_map.json",
            f"data.val_lang_data_path={root}/val_map.json", f"data.test_lang_data_path={root}/val_map.json", f"data.voxel_size={VOXEL}",
            f"data.num_views={N_VIEWS}", f"data.image_size={image_size}", "data.batch_size=4", "model.text_encoder=BiGRUEncoder",
            "model.image_encoder=MVCNNEncoder", "model.voxel_encoder=SparseCNNEncoder"]


def torch_expression(x_u8, size):
    y = F.interpolate(torch.from_numpy(np.array(x_u8)).to(torch.float32), size=size, mode="bicubic", align_corners=False,
                      antialias=True)
    return y, y.clamp(0, 255).round().to(torch.uint8)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("exp_data"))
    shapes, tokens = write_tree(root)
    return root, shapes, tokens


# ---------------------------------------------------------------------------------------------------- the resize
def test_tau_rests_on_torchs_own_fp32_error():
    """The measurement behind resize_reference.TAU, over the full geometry list: torch's fp32 result against the float64 model with the
    random and the stripe contents, and torch's u8 result under the acceptance rule."""
    worst = 0.0
    for g in rr.GEOMETRIES:
        for content in ("random", "stripes"):
            x, y64 = rr.case(g, 3, content)
            y32, u8 = torch_expression(x, g[2:])
            dev = float(np.abs(y32.numpy().astype(np.float64) - y64).max())
            near, off = rr.check(u8.numpy(), y64, f"torch {rr.geom_id(g)} {content}")
            print(f"{rr.geom_id(g)} {content}: max |fp32 - y64| {dev:.2e}, {near} pixel(s) in the band, {off} of them off by 1")
            worst = max(worst, dev)
    print(f"largest deviation {worst:.2e}")
    assert worst < rr.TAU_REFERENCE_LIMIT


@pytest.mark.parametrize("geom", rr.GEOMETRIES, ids=rr.geom_id)
def test_host_path_obeys_the_acceptance_rule_and_is_the_torch_expression(geom):
    from tricolo_amd import ops
    for planes in rr.PLANES:
        for content in rr.CONTENTS:
            x, y64 = rr.case(geom, planes, content)
            got = ops.resize_bicubic_aa_u8(torch.from_numpy(x.copy()), geom[2:])
            rr.check(got.numpy(), y64, f"{rr.geom_id(geom)} x{planes} {content}")
            assert torch.equal(got, torch_expression(x, geom[2:])[1])
            if geom[:2] == geom[2:]:
                assert np.array_equal(got.numpy(), x)


def test_size_rule_and_argument_checks():
    from tricolo_amd import ops
    x = torch.from_numpy(rr.make_image("random", 3, 20, 30))
    assert ops.resize_bicubic_aa_u8(x, 8).shape == (1, 3, 8, 12)                      # short edge -> 8, long edge int(8 * 30 / 20)
    assert ops.resize_bicubic_aa_u8(x.transpose(-1, -2), 8).shape == (1, 3, 12, 8)
    assert ops.resize_bicubic_aa_u8(x, (7, 9)).shape == (1, 3, 7, 9)
    assert ops.resize_bicubic_aa_u8(x[0, 0], 8).shape == (8, 12)                      # [..., H, W]: a bare plane, and a 5-D stack
    assert ops.resize_bicubic_aa_u8(x[None].expand(2, 1, 3, 20, 30), 8).shape == (2, 1, 3, 8, 12)
    assert torch.equal(ops.resize_bicubic_aa_u8(x[None], 8)[0], ops.resize_bicubic_aa_u8(x, 8))
    assert ops.resize_output_size(20, 30, 8) == (8, 12) and ops.resize_output_size(224, 224, 128) == (128, 128)
    with pytest.raises(ValueError, match="uint8"):
        ops.resize_bicubic_aa_u8(x.to(torch.float32), 8)


# ---------------------------------------------------------------------------------------------------- the dataset
def reference_item(shapes, tokens, idx, image_size):
    """general_dataset.py:47-54 (COO conversion, view choice), :63-65 (resize), :79-93 (item), restated on the test's own arrays."""
    cat, mid = CAPTIONS[idx]
    dense, images = shapes[(cat, mid)]
    grid = np.transpose(dense, (1, 2, 3, 0))
    flat = grid.reshape(-1, grid.shape[3])
    solid = flat[:, -1].nonzero()
    coords = (np.indices(grid.shape[:3], dtype=np.uint8).reshape(3, -1).T)[solid]
    feats = flat[:, :3][solid]
    sub_idx = np.round(np.linspace(0, len(images) - 1, N_VIEWS)).astype(int)
    resized = torch_expression(images[sub_idx], (image_size, image_size))[1]
    mean = torch.tensor((0.48145466, 0.4578275, 0.40821073)).view(3, 1, 1)
    std = torch.tensor((0.26862954, 0.26130258, 0.27577711)).view(3, 1, 1)
    return {"model_id": mid, "category": cat, "tokens": tokens[idx], "images": (resized.to(torch.float32) / 255 - mean) / std,
            "locs": torch.from_numpy(coords.astype(np.int32)), "feats": torch.from_numpy(feats.astype(np.float32) / 255), "sub_idx": sub_idx}


def check_batch(b, idx, ds, tokens, device="cpu", image_size=IMAGE_SIZE):
    n = len(idx)
    assert list(b) == ["model_id", "category", "tokens", "images", "voxels"] and list(b["voxels"]) == ["rgba"]
    assert b["model_id"] == [CAPTIONS[i][1] for i in idx] and b["category"] == [CAPTIONS[i][0] for i in idx]
    assert b["tokens"].dtype == torch.int32 and b["tokens"].shape == (n, TOKEN_LEN) and np.array_equal(b["tokens"].cpu().numpy(), tokens[idx])
    assert b["images"].dtype == torch.uint8 and b["images"].shape == (n, N_VIEWS, 3, image_size, image_size)
    assert b["voxels"]["rgba"].dtype == torch.uint8 and b["voxels"]["rgba"].shape == (n, 4, VOXEL, VOXEL, VOXEL)
    for t in (b["tokens"], b["images"], b["voxels"]["rgba"]):
        assert t.device.type == torch.device(device).type
    sh = [SHAPES.index(CAPTIONS[i]) for i in idx]
    assert torch.equal(b["images"].cpu(), ds.images_u8[sh].cpu()) and torch.equal(b["voxels"]["rgba"].cpu(), ds.rgba_u8[sh].cpu())


def test_packed_dataset_on_the_host(tree):
    from tricolo_amd.data.dataset import PackedDataset
    root, shapes, tokens = tree
    cfg = tcfg.compose(overrides=tree_overrides(root))
    ds = PackedDataset(cfg, "train", device="cpu")
    assert len(ds) == 11 and ds.num_shapes == 5 and ds.shape_keys == SHAPES
    assert ds.shape_of.tolist() == [0, 1, 0, 2, 3, 1, 0, 4, 2, 3, 4]
    assert all(s.tolist() == [0, 3, 6, 8, 11] for s in ds.sub_idx)
    assert ds.texts[3] == "caption 3 of m2"
    assert ds.images_u8.shape == (5, N_VIEWS, 3, IMAGE_SIZE, IMAGE_SIZE) and ds.rgba_u8.shape == (5, 4, VOXEL, VOXEL, VOXEL)
    assert ds.tokens.dtype == torch.int32 and ds.tokens.shape == (11, TOKEN_LEN)
    for idx in range(len(ds)):
        item, want = ds[idx], reference_item(shapes, tokens, idx, IMAGE_SIZE)
        assert set(item) == {"model_id", "category", "tokens", "images", "locs", "feats", "clip_embeddings_img", "clip_embeddings_text"}
        assert (item["model_id"], item["category"]) == (want["model_id"], want["category"])
        assert item["tokens"].dtype == np.int32 and np.array_equal(item["tokens"], want["tokens"])
        assert item["images"].dtype == torch.float32 and torch.equal(item["images"], want["images"])           # bit-equal on the host path
        assert item["locs"].dtype == torch.int32 and torch.equal(item["locs"], want["locs"])
        assert item["feats"].dtype == torch.float32 and torch.equal(item["feats"], want["feats"])
        locs, feats = syn.grid_to_sparse(shapes[CAPTIONS[idx]][0])
        assert np.array_equal(item["locs"].numpy(), locs) and np.array_equal(item["feats"].numpy(), feats)
        assert item["clip_embeddings_img"] is None and item["clip_embeddings_text"] is None

    got = list(ds.batches(4)(0))
    assert [len(b["model_id"]) for b in got] == [4, 4, 3]
    for k, b in enumerate(got):
        check_batch(b, list(range(4 * k, min(4 * k + 4, 11))), ds, tokens)
    assert [len(b["model_id"]) for b in ds.batches(4, drop_last=True)(0)] == [4, 4]
    for epoch in (0, 3):
        order = np.random.default_rng(9 + epoch).permutation(11)
        got = list(ds.batches(4, shuffle_seed=9)(epoch))
        assert len(got) == 3
        for k, b in enumerate(got):
            check_batch(b, [int(i) for i in order[4 * k:4 * k + 4]], ds, tokens)
    host = PackedDataset(cfg, "train", device="cpu", store="host")
    for a, b in zip(ds.batches(4)(0), host.batches(4)(0)):
        assert torch.equal(a["images"], b["images"]) and torch.equal(a["voxels"]["rgba"], b["voxels"]["rgba"]) and torch.equal(a["tokens"], b["tokens"])


def test_batches_follow_the_model_config(tree):
    from tricolo_amd.data.dataset import PackedDataset
    root = tree[0]
    for img, vox in ((None, "SparseCNNEncoder"), ("MVCNNEncoder", None), (None, None)):
        ov = [o for o in tree_overrides(root) if not o.startswith(("model.image_encoder", "model.voxel_encoder"))]
        ov += [f"model.image_encoder={img or 'null'}", f"model.voxel_encoder={vox or 'null'}"]
        b = next(iter(PackedDataset(tcfg.compose(overrides=ov), "val", device="cpu").batches(4)(0)))
        assert ("images" in b) == (img is not None) and ("voxels" in b) == (vox is not None)
        assert {"model_id", "category", "tokens"} <= set(b)


def test_missing_files_and_clip_runs_raise(tree, tmp_path):
    import shutil
    from tricolo_amd.data.dataset import PackedDataset
    root = str(tmp_path / "broken")
    shutil.copytree(tree[0], root)
    cfg = tcfg.compose(overrides=tree_overrides(root))
    gone = os.path.join(root, "cat_b", "m3.npz")
    os.remove(gone)
    with pytest.raises(FileNotFoundError) as e:
        PackedDataset(cfg, "train", device="cpu")
    assert gone in str(e.value)
    np.savez(gone, images=np.zeros((12, 3, SRC, SRC), np.uint8))                      # the file is there, the voxel size is not
    with pytest.raises(KeyError) as e:
        PackedDataset(cfg, "train", device="cpu")
    assert gone in str(e.value) and f"voxel{VOXEL}" in str(e.value)
    clip_cfg = tcfg.compose(overrides=tree_overrides(tree[0]) + ["model.text_encoder=CLIPTextEncoder"])
    with pytest.raises(NotImplementedError, match="CLIPTextEncoder"):
        PackedDataset(clip_cfg, "train", device="cpu")


def test_train_main_builds_the_packed_dataset(tree, monkeypatch):
    """`python -m tricolo_amd.train data=text2shape_chair_table ...` reaches fit() with batch sources of the packed tree (fit itself
    needs the GPU and is captured here)."""
    from tricolo_amd import train
    seen = {}

    def fake_fit(net, cfg, train_batches, val_batches=None, **kw):
        seen.update(net=net, cfg=cfg, train=train_batches, val=val_batches, kw=kw)
        return {"captured": True}
    monkeypatch.setattr(train, "fit", fake_fit)
    assert train.main(tree_overrides(tree[0])) == {"captured": True}
    assert seen["cfg"].data.dataset == "Text2ShapeChairTable"
    tr, va = list(seen["train"](0)), list(seen["val"](0))
    assert [len(b["model_id"]) for b in tr] == [4, 4] and [len(b["model_id"]) for b in va] == [4, 4, 3]      # train: shuffled, drop_last
    order = np.random.default_rng(seen["cfg"].train_seed).permutation(11)
    assert tr[0]["model_id"] == [CAPTIONS[i][1] for i in order[:4]]
    assert va[0]["images"].dtype == torch.uint8 and va[0]["voxels"]["rgba"].dtype == torch.uint8
    with pytest.raises(SystemExit, match="Text2Shape"):
        train.main(tree_overrides(tree[0]) + ["data.dataset=SomethingElse"])
