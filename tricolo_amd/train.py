"""Minimal fit loop for TriCoLoNet when PyTorch-Lightning is not installed (it is not on the build / GPU boxes).

The reference drives its step with Lightning (`/root/reference/train.py:26-52`): Trainer.fit + ModelCheckpoint on
`val_eval/RR@5` + LrDecayCallback (`tricolo/callback/lr_decay_callback.py:6-17`).  Orchestration is outside the hot path
this package accelerates, so this is deliberately small: it runs the SAME module hooks (`training_step`,
`validation_step`, `on_validation_epoch_end`, `configure_optimizers`) in the same order, applies the same cosine decay,
keeps the best checkpoint by the same monitor, and resumes from a checkpoint including the optimizer state.  With
Lightning installed, use the reference's own train.py with the `_target_` overrides of INTEGRATION.md instead.

    python -m tricolo_amd.train data=synthetic model.text_encoder=BiGRUEncoder model.voxel_encoder=SparseCNNEncoder \
        experiment_name=demo trainer.max_epochs=4

The packed Text2Shape sets of the reference's data/preprocess_all_data.py are read by tricolo_amd.data.dataset.PackedDataset
(renderings resized on the GPU, u8 store resident on the device):

    python -m tricolo_amd.train data=text2shape_chair_table data.dataset_root_path=/path/to/data model.text_encoder=BiGRUEncoder \
        model.image_encoder=MVCNNEncoder model.voxel_encoder=SparseCNNEncoder experiment_name=chair_table

Runs on cached CLIP features (model.text_encoder=CLIPTextEncoder and / or model.image_encoder=CLIPImageEncoder) read the
clip_embeddings_<split>.pth files of the reference's extract_clip_feats.py from data.exp_data_root_path; data=synthetic has none.
torch.manual_seed(cfg.train_seed) below also fixes the dropout masks of layers.CounterDropout (CLIPImageEncoder, and CLIPTextEncoder
with model.modules.CLIPTextEncoder.dropout=counter).
"""
from __future__ import annotations

import os
import sys
from math import cos, pi

import torch

from . import config as tcfg
from . import ops
from .checkpoint import extract_state_dict, save_reference_checkpoint


def cosine_lr(cfg, epoch: int) -> float | None:
    """lr_decay_callback.py:6-17, evaluated at the END of `epoch`: None before lr_decay.start_epoch."""
    start, end, clip = cfg.lr_decay.start_epoch, cfg.trainer.max_epochs, 1e-6
    if epoch < start:
        return None
    return clip + 0.5 * (cfg.optimizer.lr - clip) * (1 + cos(pi * ((epoch - start) / (end - start))))


def fit(net, cfg, train_batches, val_batches=None, device="cuda", ckpt_path: str | None = None, out_dir: str | None = None,
        log=print):
    """train_batches / val_batches: callables epoch -> iterable of batch dicts (data_module.py:40-65 layout).
    Returns {'epoch', 'global_step', 'best': (monitor value, path) | None, 'history': [...]}."""
    net = net.to(device)
    opt = net.configure_optimizers()
    start_epoch, step = 0, 0
    learnable = getattr(getattr(net, "loss_fn", None), "learnable_temperature", False)     # NTXentLoss(learnable_temperature=True)
    if ckpt_path is not None:                                         # train.py:41-45 -> trainer.fit(ckpt_path=...)
        assert os.path.exists(ckpt_path), "Error: Checkpoint path does not exists."
        doc = torch.load(ckpt_path, map_location="cpu", weights_only=False)
        sd = {k: v for k, v in extract_state_dict(doc).items() if ".clip_model." not in k}
        net.load_state_dict(sd, strict=True)           # (a fixed-temperature checkpoint into a learnable run: NTXentLoss says so and starts from ln(1 / T))
        if doc.get("optimizer_states"):
            osd = doc["optimizer_states"][0]
            if learnable and "loss_fn.logit_scale" not in sd:
                # the new parameter is the LAST one (loss_fn is registered behind the towers): every other index keeps its state, its own
                # moments start from zero
                groups = [dict(g) for g in osd["param_groups"]]
                groups[-1]["params"] = list(groups[-1]["params"]) + [max(i for g in groups for i in g["params"]) + 1]
                osd = dict(osd, param_groups=groups)
            opt.load_state_dict(osd)
        start_epoch, step = int(doc.get("epoch", -1)) + 1, int(doc.get("global_step", 0))
    # Lightning's Trainer(gradient_clip_val=..., gradient_clip_algorithm="norm" | "value"), given as +trainer.gradient_clip_val=...:
    # FusedAdam clips inside its step (on the device, after the data-parallel all-reduce, graph-capturable); any other optimizer
    # gets torch's utilities between backward() and step()
    clip_val, clip_alg = cfg.trainer.get("gradient_clip_val"), cfg.trainer.get("gradient_clip_algorithm", "norm") or "norm"
    if clip_val is not None and float(clip_val) == 0.0:               # (Lightning: 0 does not clip)
        clip_val = None
    torch_clip, clip_norm, clip_count = None, None, None
    if clip_val is not None:
        if clip_alg not in ("norm", "value"):
            raise ValueError(f"trainer.gradient_clip_algorithm={clip_alg!r}: 'norm' or 'value' expected")
        if hasattr(opt, "set_gradient_clip"):
            opt.set_gradient_clip(float(clip_val), clip_alg)
        else:
            if not float(clip_val) > 0.0:
                raise ValueError(f"trainer.gradient_clip_val={clip_val}: a positive value expected")
            torch_clip = torch.nn.utils.clip_grad_norm_ if clip_alg == "norm" else torch.nn.utils.clip_grad_value_
    best, history = None, []
    every = int(cfg.trainer.get("check_val_every_n_epoch", 1) or 1)
    epoch_start_step = step                                           # global step the first epoch of THIS run starts from (resume: the checkpoint's)
    for epoch in range(start_epoch, int(cfg.trainer.max_epochs)):
        net.train()
        last = None
        for batch in train_batches(epoch):
            opt.zero_grad(set_to_none=True)
            loss = net.training_step(batch, step)
            # FusedAdam(loss_scale="dynamic") seeds the backward with its device-side scale; otherwise the seed is the cached one
            loss.backward(gradient=opt.backward_seed() if hasattr(opt, "backward_seed") else ops.one(loss.device))
            if torch_clip is not None:
                total = torch_clip([p for g in opt.param_groups for p in g["params"]], float(clip_val))
                if clip_alg == "norm":                                # kept on the device: read once per epoch below
                    hit = (float(clip_val) / (total.detach() + 1e-6) < 1.0).to(torch.int64)
                    clip_norm, clip_count = total.detach(), hit if clip_count is None else clip_count + hit
            opt.step()
            last, step = loss, step + 1
        rec = {"epoch": epoch, "global_step": step, "train_loss": float(last.item()) if last is not None else None,
               "lr": float(opt.param_groups[0]["lr"])}
        if learnable:                                                 # the trained temperature: one device read per epoch
            rec["train_loss/temperature"] = net.loss_fn.current_temperature()
        if clip_val is not None and clip_alg == "norm":               # norm of the epoch's last step before clipping; steps clipped so far
            if torch_clip is None:
                rec["grad_norm"], rec["clipped_steps"] = opt.grad_norm(), opt.clipped_steps()
            else:
                rec["grad_norm"] = float(clip_norm.item()) if clip_norm is not None else None
                rec["clipped_steps"] = int(clip_count.item()) if clip_count is not None else 0
        # FusedAdam(loss_scale="dynamic"), given as +optimizer.loss_scale=dynamic: the scale the next backward is seeded with, and how often it
        # was halved / doubled so far (device reads, once per epoch); None and no keys with the option off
        scale = opt.loss_scale() if hasattr(opt, "loss_scale") else None
        if scale is not None:
            rec["loss_scale"], rec["scale_backoffs"], rec["scale_growths"] = scale, opt.scale_backoffs(), opt.scale_growths()
        if hasattr(opt, "skipped_steps"):                             # FusedAdam's overflow guard: one device read per epoch
            rec["skipped_steps"], rec["skipped_elements"] = opt.skipped_steps(), opt.nonfinite_skipped()
            seen = (history[-1].get("skipped_steps", 0) + history[-1].get("skipped_elements", 0)) if history else 0
            if rec["skipped_steps"] + rec["skipped_elements"] > seen:
                if scale is None:
                    log(f"[tricolo_amd.train] WARNING: {rec['skipped_steps']} optimizer step(s) / {rec['skipped_elements']} gradient element(s) skipped so far "
                        "because of inf / NaN gradients (f16 activation-gradient overflow?): lower ops.F16_GRAD_SCALE or train in bf16x3")
                else:
                    log(f"[tricolo_amd.train] WARNING: {rec['skipped_steps']} optimizer step(s) / {rec['skipped_elements']} gradient element(s) skipped so far "
                        f"because of inf / NaN gradients; the dynamic loss scale is now {scale:g} after {rec['scale_backoffs']} back-off(s) "
                        f"(floor {opt.loss_scale_min:g})")
            # (a resumed run starts with an empty history: its first epoch counts from the checkpoint's global step - FusedAdam.load_state_dict
            #  zeroes the skip record -, and one skipped step of a one-step epoch is a transient, not a frozen run: ADVICE r5)
            prev_sk, prev_step = (history[-1].get("skipped_steps", 0), history[-1]["global_step"]) if history else (0, epoch_start_step)
            # (with the dynamic loss scale an epoch of skipped steps is the scale on its way down: a frozen run only once it sits at its floor)
            if step - prev_step >= 2 and rec["skipped_steps"] - prev_sk >= step - prev_step and (scale is None or scale <= opt.loss_scale_min):
                # the static scale does not back off like GradScaler: a persistent overflow would freeze the weights silently
                raise RuntimeError(f"every optimizer step of epoch {epoch} was skipped for non-finite gradients"
                                   + ("" if scale is None else f" with the dynamic loss scale at its floor {scale:g}")
                                   + ": lower TRICOLO_F16_GRAD_SCALE (a power of two) or train in bf16x3")
        lr = cosine_lr(cfg, epoch)
        if lr is not None:
            for g in opt.param_groups:
                g["lr"] = lr
            if hasattr(opt, "sync_lr"):
                opt.sync_lr()                                         # device-side scalar of FusedAdam (graph replays follow it)
        if val_batches is not None and (epoch + 1) % every == 0:
            net.eval()
            with torch.no_grad():
                for i, batch in enumerate(val_batches(epoch)):
                    net.validation_step(batch, i)
                m = net.on_validation_epoch_end()
            rec["val_eval/RR@1"], rec["val_eval/RR@5"] = float(m["recall_rate"][0] * 100), float(m["recall_rate"][4] * 100)
            if "s2t" in m:                                            # inference.direction=s2t|both: shape -> text beside it, never the monitor
                s2t = m["s2t"]
                rec["val_eval/S2T_RR@1"], rec["val_eval/S2T_RR@5"] = float(s2t["recall_rate"][0] * 100), float(s2t["recall_rate"][4] * 100)
                rec["val_eval/S2T_NDCG@5"], rec["val_eval/S2T_MRR"] = float(s2t["ndcg"][4] * 100), float(s2t["mrr"] * 100)
            if out_dir is not None and (best is None or rec["val_eval/RR@5"] > best[0]):      # ModelCheckpoint(monitor=RR@5, mode=max)
                os.makedirs(out_dir, exist_ok=True)
                path = os.path.join(out_dir, f"epoch={epoch}-RR5={rec['val_eval/RR@5']:.2f}.ckpt")
                save_reference_checkpoint(net, path, epoch=epoch, global_step=step, optimizer=opt)
                if best is not None and os.path.exists(best[1]):
                    os.remove(best[1])
                best = (rec["val_eval/RR@5"], path)
        if out_dir is not None:
            os.makedirs(out_dir, exist_ok=True)
            save_reference_checkpoint(net, os.path.join(out_dir, "last.ckpt"), epoch=epoch, global_step=step, optimizer=opt)
        history.append(rec)
        log(rec)
    return {"epoch": int(cfg.trainer.max_epochs) - 1, "global_step": step, "best": best, "history": history}


PACKED_DATASETS = ("Text2ShapeChairTable", "Text2ShapeC13")


def check_dataset(cfg, program="tricolo_amd.train"):
    if cfg.data.get("dataset") == "Synthetic" and (cfg.model.text_encoder == "CLIPTextEncoder" or cfg.model.image_encoder == "CLIPImageEncoder"):
        raise SystemExit(f"{program}: data=synthetic has no cached CLIP vectors; CLIPTextEncoder / CLIPImageEncoder run on the packed Text2Shape "
                         f"sets {PACKED_DATASETS} with their clip_embeddings_<split>.pth files")
    if cfg.data.get("dataset") not in ("Synthetic",) + PACKED_DATASETS:
        raise SystemExit(f"{program} reads data=synthetic and the packed Text2Shape sets {PACKED_DATASETS} "
                         f"(data/dataset.py: <exp_data_root_path>/<category>/<model_id>.npz + <split>_map.json), not {cfg.data.get('dataset')!r}")


def split_batches(cfg, split, shuffle_seed=None, drop_last=False):
    """The batch source of one split, as fit() takes it (a callable epoch -> iterable of batch dicts); shared by train.main and
    test.main.  Packed Text2Shape sets: PackedDataset(cfg, split) in file order, or shuffled per epoch with shuffle_seed.  The store
    lives where the step runs; without a GPU it is still built (on the host) so that a data problem shows before anything else.
    data=synthetic: split "train" is the 1024-shape training set, every other split its held-out set of 256 distinct shapes, two
    captions each, in batches of min(data.batch_size, 64) on the GPU."""
    if cfg.data.dataset in PACKED_DATASETS:
        from .data.dataset import PackedDataset
        dev = "cuda" if torch.cuda.is_available() else "cpu"
        return PackedDataset(cfg, split, device=dev).batches(int(cfg.data.batch_size), shuffle_seed=shuffle_seed, drop_last=drop_last)
    from .data import synthetic as syn
    V = cfg.data.voxel_size if cfg.model.voxel_encoder else None
    nv = cfg.data.num_views if cfg.model.image_encoder else None
    B = min(int(cfg.data.get("batch_size", 32)), 64)
    if split == "train":
        items = syn.make_factor_retrieval_set(1024, 2, V or 32, nv, cfg.data.image_size, seed=syn.BASE_SEED + 301, distinct=False)
    else:
        items = syn.make_factor_retrieval_set(256, 2, V or 32, nv, cfg.data.image_size, seed=syn.BASE_SEED + 302, distinct=True)

    def gen(epoch):
        import numpy as np
        order = np.arange(len(items)) if shuffle_seed is None else np.random.default_rng(shuffle_seed + epoch).permutation(len(items))
        stop = len(order) - len(order) % B if drop_last else len(order)
        for i in range(0, stop, B):
            yield syn.batch_to_device(syn.collate_items([items[j] for j in order[i:i + B]], voxel=V is not None, views=nv is not None), "cuda")
    return gen


def main(argv=None):
    from .model.tricolo_net import TriCoLoNet
    cfg = tcfg.compose(overrides=list(argv if argv is not None else sys.argv[1:]))
    check_dataset(cfg)
    torch.manual_seed(cfg.train_seed)
    net = TriCoLoNet(cfg)
    out = os.path.join(cfg.experiment_output_path, "training") if cfg.get("experiment_name") else None
    ckpt = os.path.join(out, cfg.ckpt_name) if (out and cfg.get("ckpt_name")) else None
    # data_module.py:14-31: train split shuffled with drop_last, cfg.inference.split in file order (the synthetic sets have always
    # dropped a ragged last batch of either split)
    synthetic = cfg.data.dataset not in PACKED_DATASETS
    train = split_batches(cfg, "train", shuffle_seed=cfg.train_seed, drop_last=True)
    val = split_batches(cfg, "held_out" if synthetic else cfg.inference.split, drop_last=synthetic)
    return fit(net, cfg, train, val, ckpt_path=ckpt, out_dir=out)


if __name__ == "__main__":
    main()
