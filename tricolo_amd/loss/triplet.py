"""TripletLoss on the fused gfx950 kernels - drop-in for /root/reference/tricolo/loss/triplet.py:5-224.

Same constructor (margin) and forward(zis, zls) -> 0-d tensor with autograd: the mean of d[i][i] - d[i][j] + margin over the
semi-hard pairs, over the hard ones when there is no semi-hard pair, with the reference's distance formula (its swapped norms
included).  The reference decides the branch in a Python double loop over B x B device elements; here branch and set sizes stay on
the device (csrc/triplet.hip), so the step remains one captured graph.  One deliberate difference: where the reference raises
ZeroDivisionError (both sets empty) the loss and every gradient are NaN - FusedAdam's guard then skips the step on the device.
"""
import torch

from .. import ops
from ..layers import TriModule, require_gpu
from .all_pairs import all_pairs


class _TripletFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, zis, zls, margin, module):
        zis, zls = zis.contiguous(), zls.contiguous()
        loss, counts, ws = ops.triplet_fwd(zis, zls, margin)
        module.last_counts = counts
        ctx.save_for_backward(zis, zls, ws)          # the distances, the row counts and the branch stay in the workspace
        ctx.margin = margin
        return loss

    @staticmethod
    def backward(ctx, dloss):
        zis, zls, ws = ctx.saved_tensors
        dzis, dzls = ops.triplet_bwd(zis, zls, ws, ctx.margin, dloss.contiguous().to(torch.float32))
        return dzis, dzls, None, None


class TripletLoss(TriModule):
    def __init__(self, margin):
        super().__init__()
        self.margin = margin
        self.last_counts = None                      # device int32 (|S|, |H|) of the last forward ([P, 2] after all_pairs); never read here

    def forward(self, zis, zls):
        require_gpu(zis, "TripletLoss")
        if zis.shape != zls.shape or zis.dim() != 2:
            raise RuntimeError(f"TripletLoss: zis and zls must be [B, D] of one shape ({tuple(zis.shape)} vs {tuple(zls.shape)})")
        return _TripletFn.apply(zis, zls, float(self.margin), self)

    def all_pairs(self, embeddings):
        """The losses of every pair of `embeddings` (a list in the reference's modality order: pair (a, b) is forward(z[a], z[b]),
        tricolo_net.py:59-61) and their sum, from ONE autograd node: 3 launches forward, 1 backward, each embedding's gradient
        already summed over its pairs.  Returns ([pair losses in combination order], total), or None when the shape is outside
        the fused kernels' range (callers then loop over forward())."""
        margin = float(self.margin)

        def fwd(zs):
            losses, self.last_counts, ws = ops.triplet_multi_fwd(zs, margin)
            return losses, ws
        return all_pairs(embeddings, ops.triplet_multi_supported, fwd, lambda zs, ws, **up: ops.triplet_multi_bwd(zs, ws, margin, **up))
