"""CLIPImageEncoder - drop-in for the reference's tricolo/model/module/img_encoder/clip_img.py:6-25.

CLIP itself never runs on the hot path: the reference reads the cached, view-averaged, unit-norm CLIP vector
data_dict["clip_embeddings_img"] (extract_clip_feats.py:19-24, served by data.dataset.PackedDataset from clip_embeddings_<split>.pth)
and applies Linear -> ReLU -> Dropout(0.1) -> Linear (no normalise); its live encode_image path is commented out, so `images` is
ignored (and may be None) and a batch without the cached key is an error, as in the reference.  `clip_model` is only consulted for
`.visual.output_dim` and is NOT registered as a submodule (the reference registers it; checkpoint.py drops and re-adds its keys);
without one `clip_dim` is used.  State-dict keys: image_encoder.mlp.{0,3}.{weight,bias}.

The dropout is layers.CounterDropout(tower=1): its mask is a function of (dropout_seed, step, row, column) that the CPU can restate,
not a draw from the device generator; dropout_seed=None takes torch.initial_seed() at construction.
"""
import torch.nn as nn

from .... import ops
from ....layers import CounterDropout, LinearFn, TriModule, require_gpu


class CLIPImageEncoder(TriModule):
    def __init__(self, out_dim, num_views, clip_model=None, clip_dim=768, precision=None, dropout_seed=None, **kwargs):
        super().__init__()
        in_dim = clip_model.visual.output_dim if clip_model is not None else clip_dim
        self.num_views = num_views
        self.mlp = nn.Sequential(nn.Linear(in_dim, out_dim), nn.ReLU(inplace=True), CounterDropout(0.1, tower=1, seed=dropout_seed),
                                 nn.Linear(out_dim, out_dim))
        self.precision = precision

    def forward(self, images, data_dict):
        if "clip_embeddings_img" not in data_dict:
            raise UnboundLocalError("clip_embeddings_img missing from the batch (clip_img.py:19-24 has no live encode_image path)")
        x = data_dict["clip_embeddings_img"]
        require_gpu(x, "CLIPImageEncoder")
        prec = self.precision or ops.default_precision()
        h = LinearFn.apply(x, self.mlp[0].weight, self.mlp[0].bias, 1, prec)
        h = self.mlp[2](h)
        return LinearFn.apply(h, self.mlp[3].weight, self.mlp[3].bias, 0, prec)
