"""Generate tests/golden/clip_img.npz from the REAL reference class tricolo.model.module.img_encoder.clip_img.CLIPImageEncoder.
TEST INFRASTRUCTURE.

Runs only where the reference checkout is present (oracle.make_golden.REF); the fixture travels, the reference does not.

    python tools/make_clip_img_golden.py

The weights are oracle.recipe.fill_module(prefix="image_encoder.") and are not stored; the input is
syn.make_batch(8, None, None, clip_img=True, seed=BASE_SEED + 5)["clip_embeddings_img"], stored as its SHA-256.

  eval/   the class in eval mode, float32 (as the other module fixtures): z, the upstream gradient, and for every parameter the L2
          norm and 16 sampled entries of its gradient (oracle.make_golden.grad_probes).
  train/  the same class in float64 with mlp[2] = Dropout(0.1) replaced by a module that multiplies by the counter-based mask of
          (seed 123, step 0, row0 0, tower 1, p 0.1): 0 where dropped, float32(1 / 0.9) elsewhere, computed by
          tests/dropout_reference.py on the numpy Philox of tests/mesh_reference.py.  Same outputs.  The fixture stores the mask's recipe
          and its count of dropped elements, not the mask.
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import make_golden as mg                  # noqa: E402
from oracle.recipe import fill_module                 # noqa: E402
from tests import dropout_reference as dr             # noqa: E402
from tricolo_amd.data import synthetic as syn         # noqa: E402

B, OUT_DIM, NUM_VIEWS = 8, 512, 6
MASK = {"seed": 123, "step": 0, "row0": 0, "tower": 1, "p": 0.1}


class FixedMask(nn.Module):
    def __init__(self, m):
        super().__init__()
        self.m = m

    def forward(self, h):
        return h * self.m


def run(m, x, up, prefix, out):
    z = m(None, {"clip_embeddings_img": x})
    (z * up.to(z.dtype)).sum().backward()
    out[prefix + "z"] = z.detach().numpy()
    mg.grad_probes(m, out, prefix)
    return z


def main():
    mg.install_shims()
    import clip
    from tricolo.model.module.img_encoder.clip_img import CLIPImageEncoder
    batch = syn.make_batch(B, None, None, clip_img=True, seed=syn.BASE_SEED + 5)
    x = batch["clip_embeddings_img"]
    up = torch.randn((B, OUT_DIM), generator=torch.Generator().manual_seed(7))
    out = {"input_sha": np.array(mg.sha(x)), "upstream": up.numpy()}

    m = CLIPImageEncoder(clip.load("ViT-L/14")[0], OUT_DIM, NUM_VIEWS)
    fill_module(m, prefix="image_encoder.")
    m.eval()
    run(m, x, up, "eval/", out)

    m = CLIPImageEncoder(clip.load("ViT-L/14")[0], OUT_DIM, NUM_VIEWS)
    fill_module(m, prefix="image_encoder.")
    mult = dr.multiplier(B, OUT_DIM, MASK["p"], MASK["seed"], MASK["step"], MASK["row0"], MASK["tower"])
    assert isinstance(m.mlp[2], nn.Dropout) and m.mlp[2].p == MASK["p"]
    m.mlp[2] = FixedMask(torch.from_numpy(mult).double())
    m = m.double().train()
    run(m, x.double(), up, "train/", out)
    out.update({f"train/mask_{k}": np.float64(v) if k == "p" else np.int64(v) for k, v in MASK.items()})
    out["train/mask_dropped"] = np.int64(int((mult == 0).sum()))

    path = os.path.join(mg.GOLD, "clip_img.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes; {int(out['train/mask_dropped'])} of {B * OUT_DIM} hidden units dropped")


if __name__ == "__main__":
    main()
