"""CLIPTextEncoder - drop-in for /root/reference/tricolo/model/module/text_encoder/clip_text.py:6-22.

CLIP itself never runs on the hot path: the reference reads the cached 768-d vector
data_dict["clip_embeddings_text"] and applies Linear -> ReLU -> Dropout(0.1) -> Linear (no normalise).  `clip_model`
is only consulted for `.visual.output_dim`; without one (CLIP weights cannot be downloaded here) `clip_dim` is used.
Like the reference, a batch without the cached key is an error.

dropout="torch" (the default) is F.dropout on the device generator's stream; dropout="counter" routes through
layers.CounterDropout(tower=0), whose mask the CPU can restate (csrc/dropout.hip; dropout_seed=None takes torch.initial_seed() at
construction).  Override: model.modules.CLIPTextEncoder.dropout=counter.  The default stays "torch" because bench.py config 5 times
that path, test_clip_text_train_mode_dropout_with_an_injected_mask patches F.dropout in this module, and
test_every_entry_point_of_a_training_step_has_a_guarded_case fails if a STEP_CASES step launches an entry point its file does not guard.
"""
import torch.nn as nn
import torch.nn.functional as F

from .... import ops
from ....layers import CounterDropout, LinearFn, TriModule, require_gpu

DROPOUTS = ("torch", "counter")


class CLIPTextEncoder(TriModule):
    def __init__(self, out_dim, clip_model=None, clip_dim=768, precision=None, dropout="torch", dropout_seed=None, **kwargs):
        super().__init__()
        if dropout not in DROPOUTS:
            raise ValueError(f"CLIPTextEncoder: dropout must be one of {DROPOUTS}, got {dropout!r}")
        in_dim = clip_model.visual.output_dim if clip_model is not None else clip_dim
        drop = nn.Dropout(0.1) if dropout == "torch" else CounterDropout(0.1, tower=0, seed=dropout_seed)
        self.mlp = nn.Sequential(nn.Linear(in_dim, out_dim), nn.ReLU(inplace=True), drop, nn.Linear(out_dim, out_dim))
        self.precision, self.dropout = precision, dropout

    def forward(self, tokens, data_dict):
        if "clip_embeddings_text" not in data_dict:
            raise UnboundLocalError("clip_embeddings_text missing from the batch (clip_text.py:17-21 has no live encode_text path)")
        x = data_dict["clip_embeddings_text"]
        require_gpu(x, "CLIPTextEncoder")
        prec = self.precision or ops.default_precision()
        h = LinearFn.apply(x, self.mlp[0].weight, self.mlp[0].bias, 1, prec)
        if self.dropout == "torch":
            h = F.dropout(h, self.mlp[2].p, self.mlp[2].training)
        else:
            h = self.mlp[2](h)
        return LinearFn.apply(h, self.mlp[3].weight, self.mlp[3].bias, 0, prec)
