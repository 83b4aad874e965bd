"""CPU: training on cached CLIP features.  The torch restatement of the counter-based dropout (ops.dropout_apply on host tensors)
against the independent numpy oracle of tests/dropout_reference.py, bit for bit; its edge values, batch independence and stream
separation; PackedDataset serving clip_embeddings_<split>.pth on a tiny packed tree the test writes itself; tricolo_amd.train.main
reaching fit() with such batches; and the checkpoint keys of a Bi(CLIPImageEncoder, CLIPTextEncoder) net."""
import json
import os

import numpy as np
import pytest
import torch

from tests import dropout_reference as dr
from tricolo_amd import config as tcfg
from tricolo_amd.data import synthetic as syn

SEED = 0x9E3779B97F4A7C15                                   # a 64-bit seed: both key words are in use
SHAPES_RC = [(1, 1), (1, 4), (3, 5), (8, 512), (65, 516)]
PS = (0.0, 0.1, 0.5, 1.0)
ROW0S = (0, 4, 2 ** 32 - 2)                                 # the last one wraps inside a batch of 3 rows or more
STEPS = (0, 1, 2 ** 32 + 3)                                 # the last one equals step 3: only the low word is used
TOWERS = (0, 1)


def make_x(rows, cols, seed=0):
    g = torch.Generator().manual_seed(1000 * rows + cols + seed)
    return torch.randn((rows, cols), generator=g)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ---------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("rows,cols", SHAPES_RC, ids=[f"{r}x{c}" for r, c in SHAPES_RC])
def test_restatement_equals_the_numpy_oracle(rows, cols):
    from tricolo_amd import ops
    x = make_x(rows, cols)
    for row0 in ROW0S:
        for step in STEPS:
            for tower in TOWERS:
                bits = dr.uniform_bits(rows, cols, SEED, step, row0, tower)
                used = torch.tensor([step], dtype=torch.int64)
                for p in PS:
                    got = ops.dropout_apply(x, p, SEED, used, row0=row0, tower=tower)
                    want = dr.apply(x.numpy(), p, SEED, step, row0, tower, bits=bits)
                    assert got.dtype == torch.float32 and same_bits(got.numpy(), want), (rows, cols, p, row0, step, tower)
                    mult = ops.dropout_mask(rows, cols, p, SEED, step, row0, tower)
                    assert same_bits(mult.numpy(), dr.multiplier(rows, cols, p, SEED, step, row0, tower, bits=bits))


def test_threshold_scale_and_argument_checks():
    from tricolo_amd import ops
    assert ops.dropout_threshold_scale(0.0) == (0, 1.0) and ops.dropout_threshold_scale(1.0) == (1 << 24, 0.0)
    t, s = ops.dropout_threshold_scale(0.1)
    assert t == dr.threshold(0.1) == 1677722 and np.float32(s) == dr.scale32(0.1) == np.float32(1 / 0.9)
    used = torch.zeros(1, dtype=torch.int64)
    for p in (-0.01, 1.5, float("nan")):
        with pytest.raises(ValueError):
            ops.dropout_apply(make_x(2, 4), p, 1, used)
    with pytest.raises(ValueError):
        ops.dropout_apply(make_x(2, 4).double(), 0.1, 1, used)
    with pytest.raises(ValueError):
        ops.dropout_apply(make_x(2, 4), 0.1, 1, used.to(torch.int32))
    assert ops.dropout_apply(torch.zeros((0, 5)), 0.1, 1, used).shape == (0, 5)


def test_c_abi_refuses_bad_arguments_before_any_launch():
    """threshold > 2^24, cols < 1, rows < 0 or a null pointer: TRI_ERR_ARG; rows == 0: success without a launch (no GPU is needed)."""
    import ctypes
    from tricolo_amd import _C
    lib = _C.lib()
    buf = (ctypes.c_float * 8)()
    used = (ctypes.c_longlong * 1)()
    x, y, u = ctypes.addressof(buf), ctypes.addressof(buf) + 16, ctypes.addressof(used)
    call = lambda x=x, y=y, rows=1, cols=4, thr=1 << 23, u=u: lib.tri_dropout_apply(x, y, rows, cols, thr, 2.0, 1, u, 0, 0, None)   # noqa: E731
    assert call(thr=(1 << 24) + 1) == _C.TRI_ERR_ARG and b"threshold" in lib.tri_last_error()
    assert call(cols=0) == _C.TRI_ERR_ARG and call(rows=-1) == _C.TRI_ERR_ARG
    for null in ("x", "y", "u"):
        assert call(**{null: None}) == _C.TRI_ERR_ARG and b"null" in lib.tri_last_error()
    assert call(rows=0) == 0 and call(rows=0, x=None, y=None) == 0
    assert call(rows=0, thr=(1 << 24) + 1) == _C.TRI_ERR_ARG
    assert lib.tri_dropout_tick(None, u, None) == _C.TRI_ERR_ARG and lib.tri_dropout_tick(u, None, None) == _C.TRI_ERR_ARG


def test_tick_on_the_host():
    from tricolo_amd import ops
    step = torch.tensor([7], dtype=torch.int64)
    a = ops.dropout_tick(step)
    b = ops.dropout_tick(step)
    assert a.tolist() == [7] and b.tolist() == [8] and step.tolist() == [9]


def test_edge_values():
    from tricolo_amd import ops
    x = make_x(8, 37)
    used = torch.tensor([5], dtype=torch.int64)
    assert same_bits(ops.dropout_apply(x, 0.0, SEED, used).numpy(), x.numpy())                          # p = 0: x exactly
    assert not ops.dropout_apply(x, 1.0, SEED, used).any()                                              # p = 1: zeros
    keep = dr.dropped(8, 37, 0.5, SEED, 5) == 0
    assert 0 < keep.sum() < keep.size
    r, c = [int(v[0]) for v in np.nonzero(~keep)]                                                       # a dropped position
    rk, ck = [int(v[0]) for v in np.nonzero(keep)]                                                      # and a kept one
    y = x.clone()
    y[r, c], y[rk, ck] = float("inf"), float("-inf")
    out = ops.dropout_apply(y, 0.5, SEED, used)
    assert torch.isnan(out[r, c]) and out[rk, ck] == float("-inf")                                      # inf * 0 = NaN, as in torch
    assert int(torch.isnan(out).sum()) == 1
    z = y.clone()
    z[r, c] = float("nan")
    assert torch.isnan(ops.dropout_apply(z, 0.5, SEED, used)[r, c])
    # the fraction dropped follows p: 8 x 512 draws at p = 0.1, six binomial standard deviations
    frac = float((ops.dropout_mask(8, 512, 0.1, SEED, 0) == 0).float().mean())
    assert abs(frac - 0.1) < 6 * np.sqrt(0.1 * 0.9 / 4096)


def test_batch_independence_and_stream_separation():
    from tricolo_amd import ops
    x = make_x(8, 512)
    used = torch.tensor([3], dtype=torch.int64)
    full = ops.dropout_apply(x, 0.1, SEED, used, tower=1)
    half = ops.dropout_apply(x[4:], 0.1, SEED, used, row0=4, tower=1)
    assert same_bits(full[4:].numpy(), half.numpy())                                                    # rows [4, 8) of the full batch
    masks = {name: ops.dropout_mask(8, 512, 0.1, seed, step, 0, tower)
             for name, (seed, step, tower) in {"base": (SEED, 3, 1), "tower": (SEED, 3, 0), "step": (SEED, 4, 1), "seed": (SEED + 1, 3, 1),
                                               "seed_hi": (SEED ^ (1 << 40), 3, 1)}.items()}
    for name, m in masks.items():
        if name != "base":
            differ = float((m != masks["base"]).float().mean())
            assert 0.1 < differ < 0.26, (name, differ)                                                  # independent masks differ at 2 p (1 - p) = 0.18
    assert torch.equal(ops.dropout_mask(8, 512, 0.1, SEED, 2 ** 32 + 3, 0, 1), masks["base"])


def test_counter_dropout_module_on_the_host():
    from tricolo_amd.layers import CounterDropout
    torch.manual_seed(77)
    m = CounterDropout(0.1, tower=1)
    assert m.seed == 77 and m.row0 == 0 and m.tower == 1 and list(m.state_dict()) == [] and m.step.dtype == torch.int64
    assert CounterDropout(0.1, tower=0, seed=5).seed == 5
    with pytest.raises(ValueError):
        CounterDropout(1.5, tower=0)
    x = make_x(4, 10).requires_grad_()
    m.eval()
    assert m(x) is x and m.step.tolist() == [0]                                                         # eval: identity, no tick
    m.train()
    y0 = m(x)
    y1 = m(x)
    assert m.step.tolist() == [2]
    y0.sum().backward()                                                                                 # after the later forward ticked
    assert same_bits(x.grad.numpy(), dr.multiplier(4, 10, 0.1, 77, 0, 0, 1))
    assert same_bits(y1.detach().numpy(), dr.apply(x.detach().numpy(), 0.1, 77, 1, 0, 1))
    m.row0 = 4
    assert same_bits(m(x).detach().numpy(), dr.apply(x.detach().numpy(), 0.1, 77, 2, 4, 1))


def test_make_batch_clip_img_moves_no_other_draw():
    a = syn.make_batch(4, 32, 2, 16, clip_text=True, seed=syn.BASE_SEED + 5)
    b = syn.make_batch(4, 32, 2, 16, clip_text=True, clip_img=True, seed=syn.BASE_SEED + 5)
    assert "clip_embeddings_img" not in a and b["clip_embeddings_img"].shape == (4, 768) and b["clip_embeddings_img"].dtype == torch.float32
    for k in ("tokens", "images", "clip_embeddings_text"):
        assert torch.equal(a[k], b[k])
    assert torch.equal(a["voxels"]["locs"], b["voxels"]["locs"]) and torch.equal(a["voxels"]["feats"], b["voxels"]["feats"])
    np.testing.assert_allclose(b["clip_embeddings_img"].norm(dim=1).numpy(), 1.0, rtol=1e-6)
    assert not torch.equal(b["clip_embeddings_img"], b["clip_embeddings_text"])


# ---------------------------------------------------------------------------------------------------- the dataset
CLIP_DIM, VOXEL, N_VIEWS, IMAGE_SIZE, SRC, TOKEN_LEN = 16, 32, 2, 8, 12, 10
# (category, model id) per caption: 6 shapes in 2 categories, two or three captions each, not contiguous
CAPTIONS = [("cat_a", "m0"), ("cat_b", "m3"), ("cat_a", "m1"), ("cat_a", "m0"), ("cat_b", "m4"), ("cat_a", "m2"), ("cat_b", "m5"), ("cat_b", "m3"),
            ("cat_a", "m1"), ("cat_a", "m0"), ("cat_b", "m5"), ("cat_a", "m2"), ("cat_b", "m4"), ("cat_b", "m3")]
SHAPES = [("cat_a", "m0"), ("cat_b", "m3"), ("cat_a", "m1"), ("cat_b", "m4"), ("cat_a", "m2"), ("cat_b", "m5")]       # order of first occurrence
# the "test" split repeats model id m0 under another category: the .pth is keyed by the model id alone
CAPTIONS_TEST = [("cat_a", "m0"), ("cat_b", "m0"), ("cat_b", "m3"), ("cat_a", "m0")]


def clip_table(split, ids, dim=CLIP_DIM):
    """What extract_clip_feats.py would have written for `split`: fp16, unit norm, one img and ONE text vector per model id."""
    rng = np.random.default_rng(["train", "val", "test"].index(split) + 11)
    table = {}
    for mid in ids:
        v = rng.standard_normal((2, dim))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        table[mid] = {"img": torch.from_numpy(v[0]).to(torch.float16), "text": torch.from_numpy(v[1]).to(torch.float16)}
    return table


def write_tree(root, npz=True, dim=CLIP_DIM):
    """A packed tree with the .pth files (vectors of length `dim`); returns {split: table}."""
    rng = np.random.default_rng(5)
    if npz:
        for cat, mid in SHAPES + [("cat_b", "m0")]:
            os.makedirs(os.path.join(root, cat), exist_ok=True)
            np.savez(os.path.join(root, cat, f"{mid}.npz"), **{f"voxel{VOXEL}": syn.make_voxel_grid_u8(rng, VOXEL), "images": syn.make_images_u8(rng, 3, SRC)})
    tables = {}
    for split, caps in (("train", CAPTIONS), ("val", CAPTIONS), ("test", CAPTIONS_TEST)):
        items = []
        for k, (cat, mid) in enumerate(caps):
            tok = np.zeros(TOKEN_LEN, dtype=np.int64)
            tok[:3 + k % 5] = rng.integers(1, syn.DEFAULT_VOCAB, size=3 + k % 5)
            items.append({"model_id": mid, "category": cat, "tokens": [int(t) for t in tok], "caption": f"caption {k} of {mid}"})
        with open(os.path.join(root, f"{split}_map.json"), "w") as f:
            json.dump(items, f)
        tables[split] = clip_table(split, list(dict.fromkeys(m for _, m in caps)), dim)
        torch.save(tables[split], os.path.join(root, f"clip_embeddings_{split}.pth"))
    return tables


def overrides(root, text="CLIPTextEncoder", image="CLIPImageEncoder", voxel=None, extra=()):
    return ["data=text2shape_chair_table", f"data.exp_data_root_path={root}", f"data.train_lang_data_path={root}/train_map.json",
            f"data.val_lang_data_path={root}/val_map.json", f"data.test_lang_data_path={root}/test_map.json", f"data.voxel_size={VOXEL}",
            f"data.num_views={N_VIEWS}", f"data.image_size={IMAGE_SIZE}", "data.batch_size=4", f"model.text_encoder={text}",
            f"model.image_encoder={image or 'null'}", f"model.voxel_encoder={voxel or 'null'}"] + list(extra)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("clip_exp_data"))
    return root, write_tree(root)


def want_rows(table, keys, kind):
    return torch.stack([table[mid][kind].to(torch.float32) for _, mid in keys])


def test_packed_dataset_serves_the_cached_vectors(tree, tmp_path):
    import shutil
    from tricolo_amd.data.dataset import PackedDataset
    root = str(tmp_path / "no_npz")
    shutil.copytree(tree[0], root)
    for cat in ("cat_a", "cat_b"):
        shutil.rmtree(os.path.join(root, cat))                                                          # Bi(CLIP, CLIP) opens no .npz: there is none
    tables = tree[1]
    for store in ("device", "host"):
        ds = PackedDataset(tcfg.compose(overrides=overrides(root)), "train", device="cpu", store=store)
        assert len(ds) == 14 and ds.shape_keys == SHAPES and not ds.with_images and not ds.with_voxels
        for name, kind in (("clip_img", "img"), ("clip_text", "text")):
            t = getattr(ds, name)
            assert t.dtype == torch.float32 and t.shape == (6, CLIP_DIM) and torch.equal(t, want_rows(tables["train"], SHAPES, kind))
        got = list(ds.batches(4)(0))
        assert [len(b["model_id"]) for b in got] == [4, 4, 4, 2]
        for k, b in enumerate(got):
            caps = CAPTIONS[4 * k:4 * k + 4]
            assert list(b) == ["model_id", "category", "tokens", "clip_embeddings_img", "clip_embeddings_text"]          # no renderings, no grids
            assert b["model_id"] == [m for _, m in caps] and b["tokens"].dtype == torch.int32 and b["tokens"].shape == (len(caps), TOKEN_LEN)
            for key, kind in (("clip_embeddings_img", "img"), ("clip_embeddings_text", "text")):
                assert b[key].dtype == torch.float32 and torch.equal(b[key], want_rows(tables["train"], caps, kind))
        order = np.random.default_rng(9).permutation(14)
        b = next(iter(ds.batches(4, shuffle_seed=9)(0)))
        assert torch.equal(b["clip_embeddings_text"], want_rows(tables["train"], [CAPTIONS[i] for i in order[:4]], "text"))
    # one text vector per model id: the three captions of m0 carry the same row
    rows = [ds[i]["clip_embeddings_text"] for i, c in enumerate(CAPTIONS) if c == ("cat_a", "m0")]
    assert len(rows) == 3 and all(torch.equal(r, rows[0]) for r in rows)
    item = ds[1]
    assert set(item) == {"model_id", "category", "tokens", "images", "locs", "feats", "clip_embeddings_img", "clip_embeddings_text"}
    assert (item["model_id"], item["category"]) == ("m3", "cat_b") and item["tokens"].dtype == np.int32
    assert item["images"] is None and item["locs"] is None and item["feats"] is None
    for key, kind in (("clip_embeddings_img", "img"), ("clip_embeddings_text", "text")):
        assert item[key].dtype == torch.float32 and item[key].shape == (CLIP_DIM,) and torch.equal(item[key], tables["train"]["m3"][kind].float())
    # keyed by the model id alone: (cat_a, m0) and (cat_b, m0) are two shapes with one pair of vectors
    ds = PackedDataset(tcfg.compose(overrides=overrides(root)), "test", device="cpu")
    assert ds.shape_keys == [("cat_a", "m0"), ("cat_b", "m0"), ("cat_b", "m3")]
    assert torch.equal(ds.clip_img[0], ds.clip_img[1]) and torch.equal(ds.clip_text[0], tables["test"]["m0"]["text"].float())


def test_towers_load_only_what_they_consume(tree, monkeypatch):
    from tricolo_amd.data import dataset as dsm
    root, tables = tree
    opened = []
    real_load = np.load

    def spy(path, *a, **kw):
        opened.append(path)
        return real_load(path, *a, **kw)
    monkeypatch.setattr(dsm.np, "load", spy)
    b = next(iter(dsm.PackedDataset(tcfg.compose(overrides=overrides(root)), "val", device="cpu").batches(4)(0)))
    assert opened == [] and "images" not in b and "voxels" not in b
    # CLIP image tower + voxel tower + BiGRU: grids are loaded, renderings are not, and both vectors are served
    ds = dsm.PackedDataset(tcfg.compose(overrides=overrides(root, text="BiGRUEncoder", voxel="SparseCNNEncoder")), "val", device="cpu")
    assert len(opened) == 6 and ds.rgba_u8.shape == (6, 4, VOXEL, VOXEL, VOXEL) and ds.images_u8.shape[0] == 0 and ds.sub_idx == []
    b = next(iter(ds.batches(4)(0)))
    assert list(b) == ["model_id", "category", "tokens", "voxels", "clip_embeddings_img", "clip_embeddings_text"]
    assert ds[0]["images"] is None and ds[0]["locs"].dtype == torch.int32
    # CLIP text tower + MVCNN: renderings, no grids
    ds = dsm.PackedDataset(tcfg.compose(overrides=overrides(root, image="MVCNNEncoder")), "val", device="cpu")
    b = next(iter(ds.batches(4)(0)))
    assert list(b) == ["model_id", "category", "tokens", "images", "clip_embeddings_img", "clip_embeddings_text"]
    assert b["images"].shape == (4, N_VIEWS, 3, IMAGE_SIZE, IMAGE_SIZE) and ds.rgba_u8.shape[0] == 0


def test_dataset_errors(tree, tmp_path):
    import shutil
    from tricolo_amd.data.dataset import PackedDataset
    root = str(tmp_path / "broken")
    shutil.copytree(tree[0], root)
    cfg = tcfg.compose(overrides=overrides(root))
    path = os.path.join(root, "clip_embeddings_train.pth")
    good = torch.load(path, weights_only=True)

    table = {k: v for k, v in good.items() if k != "m4"}
    torch.save(table, path)
    with pytest.raises(KeyError) as e:
        PackedDataset(cfg, "train", device="cpu")
    assert path in str(e.value) and "m4" in str(e.value)

    table = dict(good, m2={"img": good["m2"]["img"].view(2, 8), "text": good["m2"]["text"]})
    torch.save(table, path)
    with pytest.raises(ValueError, match="1-D") as e:
        PackedDataset(cfg, "train", device="cpu")
    assert "m2" in str(e.value)

    table = dict(good, m5={"img": good["m5"]["img"], "text": good["m5"]["text"][:12]})
    torch.save(table, path)
    with pytest.raises(ValueError, match="length 12") as e:
        PackedDataset(cfg, "train", device="cpu")
    assert "m5" in str(e.value) and path in str(e.value)

    os.remove(path)
    for ov in (overrides(root), overrides(root, text="BiGRUEncoder"), overrides(root, image=None)):
        with pytest.raises(NotImplementedError) as e:
            PackedDataset(tcfg.compose(overrides=ov), "train", device="cpu")
        assert "CLIPTextEncoder" in str(e.value) and "CLIPImageEncoder" in str(e.value) and path in str(e.value)
    PackedDataset(cfg, "val", device="cpu")                                                             # the other split still has its file


# ---------------------------------------------------------------------------------------------------- the command line, the checkpoint
def test_train_main_reaches_fit_with_clip_batches(tree, monkeypatch):
    from tricolo_amd import train
    from tricolo_amd.layers import CounterDropout
    from tricolo_amd.model.module.img_encoder.clip_img import CLIPImageEncoder
    seen = {}

    def fake_fit(net, cfg, train_batches, val_batches=None, **kw):
        seen.update(net=net, cfg=cfg, train=train_batches, val=val_batches)
        return {"captured": True}
    monkeypatch.setattr(train, "fit", fake_fit)
    args = overrides(tree[0], extra=["model.modules.CLIPTextEncoder.dropout=counter", "model.out_dim=32", "experiment_name=clip_cpu"])
    assert train.main(args) == {"captured": True}
    net, cfg = seen["net"], seen["cfg"]
    assert isinstance(net.image_encoder, CLIPImageEncoder) and net.voxel_encoder is None and net.image_encoder.num_views == N_VIEWS
    drops = [net.text_encoder.mlp[2], net.image_encoder.mlp[2]]
    assert all(isinstance(d, CounterDropout) for d in drops) and [d.tower for d in drops] == [0, 1]
    assert [d.seed for d in drops] == [cfg.train_seed] * 2                                               # torch.manual_seed(cfg.train_seed) fixes the masks
    tr, va = list(seen["train"](0)), list(seen["val"](0))
    assert [len(b["model_id"]) for b in tr] == [4, 4, 4] and [len(b["model_id"]) for b in va] == [4, 4, 4, 2]
    order = np.random.default_rng(cfg.train_seed).permutation(14)
    assert tr[0]["model_id"] == [CAPTIONS[i][1] for i in order[:4]]
    assert torch.equal(tr[0]["clip_embeddings_img"], want_rows(tree[1]["train"], [CAPTIONS[i] for i in order[:4]], "img"))
    assert "images" not in va[0] and va[0]["clip_embeddings_text"].shape == (4, CLIP_DIM)
    assert net._images(va[0]) is None                                                                    # what the image tower is handed
    with pytest.raises(SystemExit, match="synthetic"):
        train.main(["data=synthetic", "model.text_encoder=CLIPTextEncoder"])
    # the default text head stays on torch's dropout
    train.main(overrides(tree[0]))
    assert isinstance(seen["net"].text_encoder.mlp[2], torch.nn.Dropout) and isinstance(seen["net"].image_encoder.mlp[2], CounterDropout)


def test_checkpoint_keys(tree, tmp_path):
    from tricolo_amd import test as inference
    from tricolo_amd.checkpoint import extract_state_dict, load_reference_checkpoint, save_reference_checkpoint
    from tricolo_amd.model.tricolo_net import TriCoLoNet
    mlp = [f"mlp.{i}.{w}" for i in (0, 3) for w in ("weight", "bias")]
    clip_state = {"visual.proj": torch.ones(2, 3), "text_encoder.clip_model.logit_scale": torch.tensor(4.6)}
    clip_keys = ["visual.proj", "logit_scale"]
    cfg = tcfg.compose(overrides=overrides(tree[0], extra=["model.out_dim=32", "model.modules.CLIPTextEncoder.dropout=counter"]))
    net = TriCoLoNet(cfg)
    assert sorted(net.state_dict()) == sorted([f"image_encoder.{k}" for k in mlp] + [f"text_encoder.{k}" for k in mlp])
    assert net.image_encoder.mlp[0].weight.shape == (32, 768) and not hasattr(net.image_encoder, "clip_model")
    path = str(tmp_path / "bi_clip.ckpt")
    save_reference_checkpoint(net, path, clip_state=clip_state)
    sd = extract_state_dict(path)
    assert sorted(sd) == sorted(list(net.state_dict()) + [f"{t}.clip_model.{k}" for t in ("text_encoder", "image_encoder") for k in clip_keys])
    assert torch.equal(sd["image_encoder.clip_model.visual.proj"], clip_state["visual.proj"])
    assert sorted(inference.select_checkpoint_keys(sd, cfg)) == sorted(net.state_dict())                # dropped again on load
    other = TriCoLoNet(cfg)
    assert load_reference_checkpoint(other, path) == ([], [], [])
    assert all(torch.equal(a, b) for a, b in zip(other.state_dict().values(), net.state_dict().values()))
    hp = torch.load(path, weights_only=False)["hyper_parameters"]["cfg"]
    assert hp["model"]["modules"]["CLIPImageEncoder"]["_target_"] == "tricolo.model.module.img_encoder.clip_img.CLIPImageEncoder"
    # without a CLIP image tower the CLIP weights go under the text tower alone, as before
    cfg_t = tcfg.compose(overrides=overrides(tree[0], image=None, extra=["model.out_dim=32"]))
    path_t = str(tmp_path / "text_only.ckpt")
    save_reference_checkpoint(TriCoLoNet(cfg_t), path_t, clip_state=clip_state)
    assert sorted(k for k in extract_state_dict(path_t) if ".clip_model." in k) == [f"text_encoder.clip_model.{k}" for k in sorted(clip_keys)]
