"""What the losses' all_pairs() share: the eligibility test and the one autograd node over the fused all-pairs kernels."""
import torch


class _AllPairsFn(torch.autograd.Function):
    """All pairs of M = 2 / 3 embeddings: outputs (loss_pair_0, ..., loss_pair_{P-1}, total).  fwd(zs) -> (losses [P + 1], workspace)
    and bwd(zs, workspace, dpairs=, dtotal=) -> gradients are the loss's ops.*_multi_fwd / _bwd with its hyper-parameters bound.
    The first `n_extra` tensors behind bwd are further differentiable inputs of the loss (NT-Xent's learnable logit scale): fwd / bwd
    reach them through their own closure, and bwd's list then ends with their gradients, in order.  n_extra = 0: the embeddings only."""

    @staticmethod
    def forward(ctx, fwd, bwd, n_extra, *inputs):
        zs = tuple(z.contiguous() for z in inputs[n_extra:])
        losses, ws = fwd(zs)
        ctx.save_for_backward(ws, *zs)
        ctx.bwd, ctx.n_extra = bwd, n_extra
        ctx.set_materialize_grads(False)             # unused outputs (normally every pair loss) arrive as None, not as zeros
        return tuple(losses[i] for i in range(losses.numel()))

    @staticmethod
    def backward(ctx, *grads):
        ws, *zs = ctx.saved_tensors
        f = lambda g: None if g is None else g.contiguous().to(torch.float32)     # noqa: E731
        dpairs = [f(g) for g in grads[:-1]]
        out = ctx.bwd(zs, ws, dpairs=dpairs if any(d is not None for d in dpairs) else None, dtotal=f(grads[-1]))
        dzs, dextra = out[:len(zs)], out[len(zs):len(zs) + ctx.n_extra]
        return (None, None, None, *dextra, *dzs)


def all_pairs(embeddings, supported, fwd, bwd, extra=()):
    """([pair losses in combination order], total) from ONE autograd node, or None when the embeddings are outside the fused kernels'
    range `supported(B, D, M)`.  `extra`: the loss's own differentiable inputs (see _AllPairsFn)."""
    zs = list(embeddings)
    if not (all(z.is_cuda and z.dtype == torch.float32 and z.dim() == 2 and z.shape == zs[0].shape for z in zs)
            and supported(zs[0].shape[0], zs[0].shape[1], len(zs))):
        return None
    out = _AllPairsFn.apply(fwd, bwd, len(extra), *extra, *zs)
    return list(out[:-1]), out[-1]
