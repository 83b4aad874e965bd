"""NTXentLoss on the fused gfx950 kernel - drop-in for /root/reference/tricolo/loss/nt_xent.py:10-74.

Same constructor (temperature, alpha_weight) and forward(zis, zjs, norm=True) -> 0-d tensor with autograd.  The first
argument is the `alpha_weight` side (row cross-entropy), exactly as the reference (nt_xent.py:71-74).

learnable_temperature=True (not in the reference) trains the temperature as CLIP does: the module owns the 0-d fp32 parameter
`logit_scale` = ln(1 / temperature), the kernels read it on the device - a captured step follows the optimizer's updates - and use
1 / T = exp(clamp(logit_scale, 0, max_logit_scale)), max_logit_scale = ln(100) by default.  Without the switch the module has no
parameter and is what it always was.
"""
import math

import torch

from .. import ops, parallel
from ..layers import TriModule, require_gpu
from .all_pairs import all_pairs


class _NTXentFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, zis, zjs, temperature, alpha, norm, logit_scale=None, max_logit_scale=None):
        zis, zjs = zis.contiguous(), zjs.contiguous()
        ctx.ls = {} if logit_scale is None else {"logit_scale": logit_scale.detach(), "max_logit_scale": max_logit_scale}
        loss, ws = ops.ntxent_fwd(zis, zjs, temperature, alpha, norm, **ctx.ls)
        ctx.save_for_backward(zis, zjs, ws)          # S, the log-sum-exps and the normalised rows stay in the workspace
        ctx.hyper = (temperature, alpha, norm)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        zis, zjs, ws = ctx.saved_tensors
        t, a, n = ctx.hyper
        # one launch; the upstream scalar is folded into the kernel's coefficients (no elementwise grad * dloss passes)
        out = ops.ntxent_bwd(zis, zjs, ws, t, a, n, dloss=dloss.contiguous().to(torch.float32), **ctx.ls)
        return out[0], out[1], None, None, None, (out[2] if ctx.ls else None), None


class NTXentLoss(TriModule):
    def __init__(self, temperature, alpha_weight, learnable_temperature=False, max_logit_scale=None):
        super().__init__()
        self.temperature = temperature               # learnable: the INITIAL temperature (current_temperature() reads the trained one)
        self.alpha_weight = alpha_weight
        self.learnable_temperature = bool(learnable_temperature)
        self.max_logit_scale = ops.MAX_LOGIT_SCALE if max_logit_scale is None else float(max_logit_scale)
        if self.learnable_temperature:
            if not (math.isfinite(self.max_logit_scale) and self.max_logit_scale >= 0.0):
                raise ValueError(f"NTXentLoss: max_logit_scale={max_logit_scale}: a finite value >= 0 expected")
            self.logit_scale = torch.nn.Parameter(torch.tensor(math.log(1.0 / float(temperature)), dtype=torch.float32))

    def _ls(self):
        """The keyword arguments of the learnable temperature ({} without it).  In a data-parallel run the parameter goes through
        parallel.replicated(): every rank differentiates the same global loss, and the ranks' gradients are summed afterwards."""
        return {"logit_scale": parallel.replicated(self.logit_scale), "max_logit_scale": self.max_logit_scale} if self.learnable_temperature else {}

    def current_temperature(self) -> float:
        """The temperature in use, exp(-clamp(logit_scale)).  Reads the device (a host sync): for logging, not for the step."""
        if not self.learnable_temperature:
            return float(self.temperature)
        return math.exp(-min(max(float(self.logit_scale.detach().item()), 0.0), self.max_logit_scale))

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        """A fixed-temperature checkpoint (no `logit_scale` key) loads into a learnable module: the parameter keeps its initial value."""
        key = prefix + "logit_scale"
        if self.learnable_temperature and key not in state_dict:
            print(f"[tricolo_amd] NTXentLoss: the checkpoint has no '{key}' (fixed temperature): starting from "
                  f"ln(1 / {float(self.temperature):g}) = {float(self.logit_scale.detach()):.6f}")
            state_dict = dict(state_dict)
            state_dict[key] = self.logit_scale.detach().clone()
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def forward(self, zis, zjs, norm=True):
        require_gpu(zis, "NTXentLoss")
        if zis.shape != zjs.shape:
            raise RuntimeError(f"mat1 and mat2 shapes cannot be multiplied ({tuple(zis.shape)} vs {tuple(zjs.shape)})")
        if self.learnable_temperature:
            return _NTXentFn.apply(zis, zjs, None, float(self.alpha_weight), bool(norm), *self._ls().values())
        return _NTXentFn.apply(zis, zjs, float(self.temperature), float(self.alpha_weight), bool(norm), None, None)

    def all_pairs(self, embeddings, norm=True):
        """The losses of every pair of `embeddings` (a list in the reference's modality order: the earlier one of a pair is
        the `zis` / alpha side, tricolo_net.py:59-61) and their sum, from ONE autograd node: 4 launches forward, 1 backward
        (2 with a learnable temperature), each embedding's gradient already summed over its pairs.  Returns ([pair losses in
        combination order], total), or None when the shape is outside the fused kernels' range (callers then loop over forward())."""
        hyper = (None if self.learnable_temperature else float(self.temperature), float(self.alpha_weight), bool(norm))
        ls = self._ls()
        return all_pairs(embeddings, ops.ntxent_multi_supported, lambda zs: ops.ntxent_multi_fwd(zs, *hyper, **ls),
                         lambda zs, ws, **up: ops.ntxent_multi_bwd(zs, ws, *hyper, **up, **ls), extra=tuple(ls.values())[:1])
