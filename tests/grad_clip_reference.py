"""Float64 restatement of gradient clipping as FusedAdam applies it (include/tricolo_hip.h "Gradient clipping"): the global L2 norm, the
coefficient of torch.nn.utils.clip_grad_norm_, and the Adam loop that scales (or clamps) the gradient before the weight decay joins it.

    total = |gscale| * sqrt(sum over every PRESENT gradient of g^2)          (a parameter without a gradient is not part of it)
    coef  = min(1, max_norm / (total + 1e-6)); 1 when total is inf / NaN      (that step belongs to the overflow guard: it is skipped)
    g'    = clamp(g * gscale * coef, -clip_value, clip_value) + wd * p        (the clamp only with the "value" algorithm)
    m, v, p: torch.optim.Adam (bias corrections 1 - beta^t, eps added after the square root)

`defect` plants one of the mistakes a kernel could make; tests/test_grad_clip_cpu.py shows that each moves the result by far more than
the GPU tests' tolerance at the GPU tests' own shapes, i.e. that those tests would see it.

The shapes, seeds and tolerances of tests/test_gpu_grad_clip.py live here so that the CPU tests examine the same cases.
"""
import math

import numpy as np
import torch

DEFECTS = ("coef_skips_segment", "null_counted", "ragged_dropped", "clamp_after_decay")

# ---- the optimizer-path case (tests/test_gpu_ops.py::test_adam_guard_skips_the_whole_step_on_a_non_finite_gradient's layout)
SHAPES = [(64, 36), (128,), (3, 3, 8)]
SCALES = (1.0, 30.0, 0.1, 30.0, 1.0, 0.1)
LR, WD, MAX_NORM, CLIP_VALUE, SEED = 1e-2, 1e-6, 20.0, 0.5, 9
# the value-algorithm case decays 10^5 times harder: with wd = 1e-6 a clamp on the wrong side of the decay moves a parameter by 1e-8, below
# any fp32 tolerance - the case could not tell the two orders apart
WD_VALUE = 0.1
# Distance of torch.optim.Adam's fp32 CPU loop (clip_grad_norm_ in fp32 too) from its float64 loop on the case above: 4.6e-7
# (test_grad_clip_cpu.py::test_fp32_loop_distance_is_what_the_tolerance_assumes re-measures it).  The kernel rounds in fp32 in another
# order (FMA contraction, the coefficient folded into one scalar), so it gets four times that.
FP32_LOOP_DISTANCE = 4.6e-7
ATOL = 4 * FP32_LOOP_DISTANCE
# rec[0] against float64: the double sums differ by at most n * 2^-53 (relative), the rest is the rounding to fp32 (2^-24) with room for
# the float64 reference's own sqrt and the kernel's
NORM_RTOL = 2.0 ** -22

# ---- the kernel cases
SEG_SIZES = (4, 260, 1024, 8)                                        # the second pointer is NULL
FLAT_SIZES = (0, 4, 1028, 10007, 4096 * 256 * 4 + 1028)              # 10007 sits one float past a 16-byte boundary; the last: one full grid + 1028


def case_tensors(seed=SEED, shapes=SHAPES, scales=SCALES):
    """(initial parameters, [gradients of step 0, ...]) of the optimizer-path case, fp32 on the host."""
    gen = torch.Generator().manual_seed(seed)
    init = [torch.randn(sh, generator=gen) for sh in shapes]
    steps = [[torch.randn(sh, generator=gen) * s for sh in shapes] for s in scales]
    return init, steps


def integer_gradient(n, seed):
    """Integer-valued fp32 gradient, |g| <= 1024: g^2 <= 2^20 and any sum of up to 2^32 of them is exact in double, in every order."""
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(-1024, 1025, (n,), generator=gen).to(torch.float32)


def total_norm(grads, gscale=1.0, defect=None, stale=None):
    """|gscale| * sqrt(sum g^2) over the gradients that are there, in float64.  grads: tensors or None (no gradient).
    defect "null_counted": an absent gradient contributes stale[i], what its pointer's old buffer holds;
    defect "ragged_dropped": every gradient loses the last numel % 4 elements (the scalar tail behind the 16-byte body)."""
    s = 0.0
    for i, g in enumerate(grads):
        if g is None:
            if defect != "null_counted":
                continue
            g = stale[i]
        g = g.detach().reshape(-1).double()
        if defect == "ragged_dropped":
            g = g[:g.numel() - g.numel() % 4]
        s += float((g * g).sum())
    return abs(float(gscale)) * math.sqrt(s)


def coefficient(total, max_norm):
    if not math.isfinite(total):
        return 1.0
    c = float(max_norm) / (total + 1e-6)
    return c if c < 1.0 else 1.0


def rec_fp32(total, max_norm):
    """What tri_grad_clip_coef leaves in rec: (fp32(total), fp32(coef) when coef < 1 else 1.0f)."""
    with np.errstate(over="ignore"):
        return np.float32(total), np.float32(coefficient(total, max_norm))


def adam_loop(init, steps, lr=LR, wd=WD, betas=(0.9, 0.999), eps=1e-8, max_norm=None, clip_value=None, gscale=1.0, defect=None):
    """The clipped Adam loop in float64.  steps: [[gradient or None per parameter], ...].  A step whose norm is not finite is skipped whole
    (the overflow guard).  Returns dict(p, m, v: lists of float64 tensors; norms: the total norm of every step; clipped; applied).
    defect "coef_skips_segment": parameter 1 takes its gradient without the coefficient;
    defect "clamp_after_decay": the clamp is applied to g + wd * p instead of to g."""
    p = [t.detach().double().clone() for t in init]
    m = [torch.zeros_like(t) for t in p]
    v = [torch.zeros_like(t) for t in p]
    b1, b2 = betas
    t, norms, clipped = 0, [], 0
    for grads in steps:
        total = total_norm(grads, gscale)
        norms.append(total)
        if not math.isfinite(total):
            continue
        coef = coefficient(total, max_norm) if max_norm is not None else 1.0
        clipped += coef < 1.0
        t += 1
        bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        for i, g in enumerate(grads):
            if g is None:
                continue
            g = g.detach().double() * gscale
            if not (defect == "coef_skips_segment" and i == 1):
                g = g * coef
            if clip_value is not None and defect != "clamp_after_decay":
                g = g.clamp(-clip_value, clip_value)
            g = g + wd * p[i]
            if clip_value is not None and defect == "clamp_after_decay":
                g = g.clamp(-clip_value, clip_value)
            m[i] = b1 * m[i] + (1.0 - b1) * g
            v[i] = b2 * v[i] + (1.0 - b2) * g * g
            p[i] = p[i] - (lr / bc1) * m[i] / (v[i].sqrt() / math.sqrt(bc2) + eps)
    return dict(p=p, m=m, v=v, norms=norms, clipped=int(clipped), applied=t)


def torch_loop(init, steps, dtype, lr=LR, wd=WD, max_norm=None, clip_value=None):
    """torch.nn.utils.clip_grad_norm_ / clip_grad_value_ + torch.optim.Adam on the host in `dtype`.  Returns (parameters, norms)."""
    w = [torch.nn.Parameter(t.detach().to(dtype).clone()) for t in init]
    opt = torch.optim.Adam(w, lr=lr, weight_decay=wd)
    norms = []
    for grads in steps:
        for q, g in zip(w, grads):
            q.grad = None if g is None else g.detach().to(dtype).clone()
        if max_norm is not None:
            norms.append(float(torch.nn.utils.clip_grad_norm_(w, max_norm)))
        if clip_value is not None:
            torch.nn.utils.clip_grad_value_(w, clip_value)
        opt.step()
    return [q.detach() for q in w], norms


def max_distance(a, b):
    return max(float((x.double() - y.double()).abs().max()) for x, y in zip(a, b))
