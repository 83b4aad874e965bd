"""The reference's packed Text2Shape data as a resident u8 store that hands out ready batches.

Restates /root/reference/tricolo/data/dataset/general_dataset.py:11-98 and the collate function of data_module.py:40-65 for the
files data/preprocess_all_data.py:85-106 writes: `<exp_data_root_path>/<category>/<model_id>.npz` (keys `voxel32` / `voxel64` /
..., u8 [4,V,V,V] RGBA, and `images`, u8 [n,3,224,224]) plus `{train,val,test}_map.json`, a list of
{model_id, category, tokens, caption}.  What differs is where the work happens:

  * the reference resizes every shape's renderings on the CPU at start-up (Resize(image_size, BICUBIC, antialias=True) on the u8
    tensor, general_dataset.py:63-65); here the picked views are uploaded as u8 a few hundred shapes at a time and resized by
    ops.resize_bicubic_aa_u8 on `device` (csrc/resize.hip on a GPU, the same torch expression on the host);
  * the reference keeps COO voxels and f32 images per item and collates on the host; here the renderings and the RGBA grids stay
    u8 end to end: a batch is an index_select from the store, and the towers derive mask / RGB/255 / CLIP Normalize on the device
    (MVCNNEncoder.forward on u8 images, SparseCNNEncoder.forward on {'rgba': ...}: bit-identical to the host-prepared inputs).

Memory of the store, per shape: images Nv * 3 * S * S bytes = 0.29 MB at 6 views of 128 x 128; voxels 4 * V^3 bytes = 0.13 MB at
32^3, 1.05 MB at 64^3.  Text2Shape chair/table, ~15 k shapes: 4.4 GB of images + 2 GB (32^3) or 15.7 GB (64^3) of voxels - resident
in the 288 GB of an MI355X with store="device" (the default); store="host" keeps both in (pinned, when a GPU is present) host memory
and copies each batch.  Captions cost 4 * L bytes each.

Only what a tower consumes is loaded: renderings are opened, resized and batched for MVCNNEncoder, grids for SparseCNNEncoder; a run
without either opens no .npz at all.

CLIP-feature runs (CLIPTextEncoder / CLIPImageEncoder) read `<exp_data_root_path>/clip_embeddings_<split>.pth`, the plain torch.save
dict `model_id -> {"img": Tensor[C], "text": Tensor[C]}` that the reference's extract_clip_feats.py writes; it loads without CLIP
(torch.load(weights_only=True)).  The reference's semantics are kept (general_dataset.py:24-28,56-58), quirks included:
  * the file is keyed by model_id alone, not by (category, model_id): two categories that share a model id share its vectors;
  * there is ONE text vector per model - extract_clip_feats.py:38-40 lets the model's last caption overwrite the earlier ones - so
    every caption of a shape gets the same `clip_embeddings_text`;
  * values are converted to float32 (CLIP writes fp16).
They are stored as clip_img / clip_text f32 [Ns, C] beside the u8 stores and a batch carries both keys, `clip_embeddings_img` and
`clip_embeddings_text`, f32 [B, C].  A model id the file lacks raises KeyError; a vector that is not 1-D, or whose length differs
from the others of its kind, raises ValueError; a missing file raises NotImplementedError naming the path (the file cannot be made
here: running CLIP is out of scope).  One difference: for CLIPTextEncoder the reference's items carry clip.tokenize(caption) as
`tokens`; here they stay the stored int32 captions.  No tower reads them (CLIPTextEncoder ignores its tokens); only the `tokens` of
inference's output.p differ.
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from .. import ops
from . import synthetic as syn

CHUNK_SHAPES = 256                                  # shapes uploaded and resized per call (256 * 6 views * 3 * 224 * 224 B = 231 MB of u8)


class PackedDataset:
    def __init__(self, cfg, split: str, device="cuda", store: str = "device"):
        if store not in ("device", "host"):
            raise ValueError(f"store must be 'device' or 'host', got {store!r}")
        self.cfg, self.split, self.device, self.store = cfg, split, torch.device(device), store
        self.voxel_size, self.num_views = int(cfg.data.voxel_size), int(cfg.data.num_views)
        self.with_images, self.with_voxels = cfg.model.image_encoder == "MVCNNEncoder", cfg.model.voxel_encoder == "SparseCNNEncoder"
        self.with_clip = cfg.model.text_encoder == "CLIPTextEncoder" or cfg.model.image_encoder == "CLIPImageEncoder"
        self.clip_path = os.path.join(cfg.data.exp_data_root_path, f"clip_embeddings_{split}.pth")
        if self.with_clip and not os.path.exists(self.clip_path):
            raise NotImplementedError(f"PackedDataset({split}): CLIPTextEncoder / CLIPImageEncoder runs read the cached CLIP vectors of the "
                                      f"reference's extract_clip_feats.py and {self.clip_path} does not exist (CLIP itself is not run here); "
                                      "write that file, or use BiGRUEncoder / MVCNNEncoder / SparseCNNEncoder")
        path = getattr(cfg.data, f"{split}_lang_data_path")
        with open(path, "r") as f:
            raw = json.load(f)
        # general_dataset.py:30-37: captions in file order, shapes numbered by first occurrence of (category, model_id)
        self.model_ids = [it["model_id"] for it in raw]
        self.categories = [it["category"] for it in raw]
        self.texts = [it["caption"].strip() for it in raw]
        toks = [np.asarray(it["tokens"], dtype=np.int16).astype(np.int32) for it in raw]
        if len({t.shape for t in toks}) > 1:
            raise ValueError(f"{path}: captions are padded to different lengths {sorted({t.shape[0] for t in toks})}")
        tokens = np.stack(toks) if toks else np.zeros((0, 0), np.int32)
        self.shape_index: dict = {}
        self.shape_keys: list = []
        shape_of = np.empty((len(raw),), dtype=np.int64)
        for i, key in enumerate(zip(self.categories, self.model_ids)):
            if key not in self.shape_index:
                self.shape_index[key] = len(self.shape_keys)
                self.shape_keys.append(key)
            shape_of[i] = self.shape_index[key]
        self.sub_idx: list = []                     # per shape: the views picked from its `images` (general_dataset.py:53)
        self._load_shapes()
        self.clip_img = self.clip_text = None
        if self.with_clip:
            self._load_clip()
        keep = self.device if store == "device" else torch.device("cpu")
        self.tokens = torch.from_numpy(tokens).to(keep)
        self.shape_of = torch.from_numpy(shape_of).to(keep)
        self._shape_of_np = shape_of

    # ------------------------------------------------------------------------------------------------ loading
    def _pin(self, t):
        return t.pin_memory() if (self.store == "host" and torch.cuda.is_available()) else t

    def _load_shapes(self):
        root = self.cfg.data.exp_data_root_path
        vkey = f"voxel{self.voxel_size}"
        grids, images, pending = [], [], []

        def flush():
            if pending:
                x = torch.from_numpy(np.stack(pending)).to(self.device)                          # u8 [n, Nv, 3, H, W]
                y = ops.resize_bicubic_aa_u8(x, int(self.cfg.data.image_size))
                images.append(y if self.store == "device" else y.cpu())
                pending.clear()

        wanted = ((vkey,) if self.with_voxels else ()) + (("images",) if self.with_images else ())
        for cat, mid in self.shape_keys if wanted else ():
            path = os.path.join(root, cat, f"{mid}.npz")
            if not os.path.exists(path):
                raise FileNotFoundError(f"PackedDataset({self.split}): missing shape file {path}")
            with np.load(path) as npz:
                for key in wanted:
                    if key not in npz.files:
                        raise KeyError(f"PackedDataset({self.split}): {path} has no array {key!r} (it holds {sorted(npz.files)})")
                grid = npz[vkey] if self.with_voxels else None
                views = npz["images"] if self.with_images else None
            V = self.voxel_size
            if grid is not None:
                if grid.dtype != np.uint8 or grid.shape != (4, V, V, V):
                    raise ValueError(f"{path}: {vkey} must be uint8 [4,{V},{V},{V}], got {grid.dtype} {grid.shape}")
                grids.append(grid)
            if views is None:
                continue
            if views.dtype != np.uint8 or views.ndim != 4 or views.shape[1] != 3 or views.shape[0] < 1:
                raise ValueError(f"{path}: images must be uint8 [n,3,H,W], got {views.dtype} {views.shape}")
            sub = np.round(np.linspace(0, len(views) - 1, self.num_views)).astype(int)
            self.sub_idx.append(sub)
            picked = views[sub]
            if pending and (picked.shape != pending[0].shape or len(pending) == CHUNK_SHAPES):
                flush()
            pending.append(picked)
        flush()
        if images and len({tuple(y.shape[1:]) for y in images}) > 1:
            raise ValueError(f"PackedDataset({self.split}): renderings resize to different sizes {sorted({tuple(y.shape[-2:]) for y in images})}")
        S = int(self.cfg.data.image_size)
        V = self.voxel_size
        self.images_u8 = torch.cat(images) if images else torch.zeros((0, self.num_views, 3, S, S), dtype=torch.uint8, device=self.device)
        rgba = torch.from_numpy(np.stack(grids)) if grids else torch.zeros((0, 4, V, V, V), dtype=torch.uint8)
        if self.store == "device":
            self.rgba_u8 = rgba.to(self.device)
        else:
            self.images_u8, self.rgba_u8 = self._pin(self.images_u8), self._pin(rgba)

    def _load_clip(self):
        """clip_embeddings_<split>.pth -> clip_img / clip_text f32 [Ns, C], one row per shape of shape_keys (module docstring)."""
        table = torch.load(self.clip_path, map_location="cpu", weights_only=True)
        rows = {"img": [], "text": []}
        for _, mid in self.shape_keys:
            if mid not in table:
                raise KeyError(f"{self.clip_path}: no entry for model id {mid!r}")
            for kind, out in rows.items():
                v = table[mid][kind]
                if not torch.is_tensor(v) or v.dim() != 1:
                    raise ValueError(f"{self.clip_path}: {kind!r} of model id {mid!r} must be a 1-D tensor, got "
                                     f"{tuple(v.shape) if torch.is_tensor(v) else type(v).__name__}")
                if out and v.shape != out[0].shape:
                    raise ValueError(f"{self.clip_path}: {kind!r} of model id {mid!r} has length {v.shape[0]}, the others {out[0].shape[0]}")
                out.append(v.to(torch.float32))                                                      # general_dataset.py:57-58
        stacked = [torch.stack(r) if r else torch.zeros((0, 0), dtype=torch.float32) for r in (rows["img"], rows["text"])]
        if self.store == "device":
            self.clip_img, self.clip_text = (t.to(self.device) for t in stacked)
        else:
            self.clip_img, self.clip_text = (self._pin(t) for t in stacked)

    # ------------------------------------------------------------------------------------------------ the reference's per-item view
    def __len__(self):
        return len(self.model_ids)

    @property
    def num_shapes(self):
        return len(self.shape_keys)

    def __getitem__(self, idx):
        """general_dataset.py:74-98, from the same store: CLIP-normalised f32 images, COO voxels, the cached CLIP vectors (f32 [C]),
        host tensors.  What the configured towers do not consume was not loaded and is None."""
        s = int(self._shape_of_np[idx])
        locs, feats = syn.grid_to_sparse(self.rgba_u8[s].cpu().numpy()) if self.with_voxels else (None, None)
        return {"model_id": self.model_ids[idx], "category": self.categories[idx], "tokens": self.tokens[idx].cpu().numpy(),
                "images": syn.normalise_images(self.images_u8[s].cpu().numpy()) if self.with_images else None,
                "locs": None if locs is None else torch.from_numpy(locs), "feats": None if feats is None else torch.from_numpy(feats),
                "clip_embeddings_img": self.clip_img[s].cpu() if self.with_clip else None,
                "clip_embeddings_text": self.clip_text[s].cpu() if self.with_clip else None}

    # ------------------------------------------------------------------------------------------------ batches
    def batches(self, batch_size: int, shuffle_seed=None, drop_last: bool = False):
        """-> callable epoch -> iterable of batch dicts for train.fit: model_id / category (lists of str), tokens i32 [B,L], images u8
        [B,Nv,3,S,S] (when cfg.model.image_encoder is MVCNNEncoder), voxels {'rgba': u8 [B,4,V,V,V]} (when cfg.model.voxel_encoder is
        SparseCNNEncoder), clip_embeddings_img / clip_embeddings_text f32 [B,C] (when either CLIP encoder is configured), the tensors
        on `device`.  shuffle_seed: the order of epoch e is np.random.default_rng(shuffle_seed + e).permutation(len(self))."""
        B, n = int(batch_size), len(self)
        if B < 1:
            raise ValueError("batch_size must be positive")

        def gen(epoch):
            order = np.arange(n) if shuffle_seed is None else np.random.default_rng(shuffle_seed + epoch).permutation(n)
            stop = n - n % B if drop_last else n
            for i in range(0, stop, B):
                yield self._batch(order[i:i + B])
        return gen

    def _batch(self, cap_idx):
        idx = torch.from_numpy(np.ascontiguousarray(cap_idx, dtype=np.int64)).to(self.tokens.device)
        sidx = self.shape_of.index_select(0, idx)
        move = (lambda t: t) if self.store == "device" else (lambda t: self._pin(t).to(self.device, non_blocking=True))
        d = {"model_id": [self.model_ids[i] for i in cap_idx], "category": [self.categories[i] for i in cap_idx],
             "tokens": move(self.tokens.index_select(0, idx))}
        if self.with_images:
            d["images"] = move(self.images_u8.index_select(0, sidx))
        if self.with_voxels:
            d["voxels"] = {"rgba": move(self.rgba_u8.index_select(0, sidx))}
        if self.with_clip:
            d["clip_embeddings_img"] = move(self.clip_img.index_select(0, sidx))
            d["clip_embeddings_text"] = move(self.clip_text.index_select(0, sidx))
        return d
