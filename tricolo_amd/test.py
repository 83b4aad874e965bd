"""Run a checkpoint over a split: the reference's test.py (`python test.py ... +ckpt_path=FILE`) without Lightning.

    python -m tricolo_amd.test data=text2shape_chair_table data.dataset_root_path=/path/to/data model.text_encoder=BiGRUEncoder \
        model.image_encoder=MVCNNEncoder model.voxel_encoder=SparseCNNEncoder experiment_name=chair_table +ckpt_path=chair_table_tri.ckpt

Same steps as the reference's test.py:11-32: seed with cfg.test_seed, build TriCoLoNet(cfg), load the checkpoint's state dict without
the towers the config switches off (a Tri(I+V) checkpoint serves a Bi(I) or Bi(V) run), then cfg.inference.split in file order through
net.eval() / no_grad / test_step and on_test_epoch_end.  With inference.evaluate the `RR@1 RR@5 NDCG@5 MRR` line is printed and
<inference.output_dir>/nearest.jsonl written (the file evaluation.shape_f1 reads; records in caption order, not the reference's random
order); with inference.save_predictions <inference.output_dir>/output.p is written (the file tricolo_amd.eval reads).  With
+inference.direction=s2t|both the shape -> text direction is scored too (evaluation.eval_retrieval.compute_metrics: a second line
`S2T RR@1 RR@5 NDCG@5 MRR`, records in nearest_s2t.jsonl, the numbers under "s2t" of the returned dict); output.p is the same file.  Data sources are
train.main's: data=synthetic (its held-out set) and the packed Text2Shape sets - with model.text_encoder=CLIPTextEncoder and / or
model.image_encoder=CLIPImageEncoder the latter need their clip_embeddings_<split>.pth (data/dataset.py).  main() returns the metrics dict (None without
inference.evaluate).
"""
from __future__ import annotations

import os
import sys

import torch

from . import config as tcfg
from .checkpoint import extract_state_dict
from .train import check_dataset, split_batches

MISSING_CHECKPOINT = "Error: Checkpoint path does not exists."          # test.py:18


def select_checkpoint_keys(state_dict, cfg) -> dict:
    """The entries of a checkpoint's state dict that the net of `cfg` loads: without `image_encoder` / `voxel_encoder` keys when the
    config has no such tower (test.py:21-27), and without the frozen CLIP weights a CLIP-text checkpoint carries (`.clip_model.`,
    checkpoint.py)."""
    out = {}
    loss_cfg = cfg.loss.get(cfg.loss.name) if cfg.get("loss") is not None else None
    learnable = bool(loss_cfg.get("learnable_temperature", False)) if loss_cfg is not None else False
    for key, value in state_dict.items():
        if cfg.model.image_encoder is None and "image_encoder" in key:
            continue
        if cfg.model.voxel_encoder is None and "voxel_encoder" in key:
            continue
        if ".clip_model." in key:
            continue
        if key == "loss_fn.logit_scale" and not learnable:            # a learned temperature plays no part in retrieval
            continue
        out[key] = value
    return out


def main(argv=None):
    from .model.tricolo_net import TriCoLoNet
    cfg = tcfg.compose(overrides=list(argv if argv is not None else sys.argv[1:]))
    check_dataset(cfg, "tricolo_amd.test")
    torch.manual_seed(cfg.test_seed)
    ckpt_path = cfg.get("ckpt_path")
    if not ckpt_path or not os.path.exists(ckpt_path):
        raise FileNotFoundError(MISSING_CHECKPOINT)
    net = TriCoLoNet(cfg)
    net.load_state_dict(select_checkpoint_keys(extract_state_dict(ckpt_path), cfg), strict=True)
    if not torch.cuda.is_available():
        raise RuntimeError("tricolo_amd.test runs the towers and the ranking on the GPU and there is no CPU fallback: no MI355X visible")
    os.makedirs(cfg.inference.output_dir, exist_ok=True)
    net = net.to("cuda").eval()
    with torch.no_grad():
        for i, batch in enumerate(split_batches(cfg, cfg.inference.split)(0)):
            net.test_step(batch, i)
        return net.on_test_epoch_end(nearest_path=os.path.join(cfg.inference.output_dir, "nearest.jsonl"))


if __name__ == "__main__":
    main()
