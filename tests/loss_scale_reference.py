"""Float64 / Python restatement of dynamic loss scaling as FusedAdam(loss_scale="dynamic") applies it (include/tricolo_hip.h "Dynamic loss
scaling"): the state machine of tri_loss_scale_step and the scaled, clipped Adam loop around it.

    the backward of step t is seeded with s_t, so the optimizer is FED  g_t * s_t  (an overflow is an inf in what it is fed)
    total = |gscale| * (1 / s_t) * sqrt(sum of fed^2);  c = min(1, max_norm / (total + 1e-6)), 1 without norm clipping or when total is inf / NaN
    the update takes  fed * gscale * (c / s_t)  (clamped to +-clip_value with the "value" rule) - the TRUE gradient, clipped
    skipped step (fed holds an inf / NaN): streak = 0; if s > min: s = max(s / 2, min), backoffs += 1
    applied step: streak += 1; if streak >= growth_interval: streak = 0, and if s < max: s = min(2 s, max), growths += 1

The Adam arithmetic itself is tests/grad_clip_reference.py's adam_loop: this file forms the multiplier of every step, hands adam_loop the
gradients the update sees and lets it clamp, decay and skip.  `defect` plants one of the mistakes a kernel could make;
tests/test_loss_scale_cpu.py shows that each moves the result by far more than ATOL at the GPU tests' shapes.

The cases of tests/test_gpu_loss_scale.py live here so that the CPU tests examine what the GPU tests run.  The tolerance against float64 is
grad_clip_reference.ATOL: the kernel path is the clipped path with an exact power-of-two factor in its one multiplier.
"""
import math
from collections import namedtuple

import numpy as np
import torch

from tests import grad_clip_reference as R
from tests.grad_clip_reference import (ATOL, CLIP_VALUE, FLAT_SIZES, LR, MAX_NORM, NORM_RTOL, SEG_SIZES, SHAPES, WD, WD_VALUE,  # noqa: F401
                                       adam_loop)

DEFECTS = ("norm_keeps_scale", "scale_moves_first", "streak_kept")

State = namedtuple("State", "scale streak backoffs growths")

# ---- the schedule case: twelve steps, growth every 3 applied steps, overflows planted in steps 4, 8 and 9
#   s: 1 1 1 | 2 2 | 1 1 1 | 2 | 1 | .5 .5   (grows after steps 2 and 7, backs off after 4, 8 and 9; the overflow of step 4 interrupts a streak of one)
# The true gradients are grad_clip_reference's (same shapes, same seed) at magnitudes 1, 3 and 0.1: norms of about 51, 146, 4.96, 147, 49.8
# and 5.0 under MAX_NORM = 20, so four of six steps clip and two do not, as there.  That file's 30 is not used: its tests compare parameters
# only, these compare both moments against float64 under the same ABSOLUTE tolerance, which was derived for values of the parameters' size
# (|p| < 5).  Unclipped gradients of up to 135 put |m| at 14 and |v| at 18, where one fp32 rounding is 1e-6 and torch's own fp32 CPU loop
# ends 1.3e-6 (m) and 3.4e-6 (v) from its float64 loop - beyond ATOL = 1.84e-6 by the number format alone.  At 3, |m| <= 1.3 and |v| <= 0.2:
# torch's fp32 loop ends 5.7e-7 (p), 1.7e-7 (m) and 5.6e-8 (v) away, so ATOL is more than three times what fp32 itself costs for all
# three (tests/test_loss_scale_cpu.py::test_fp32_loop_distance_of_the_schedule_case re-measures it in every clipping mode).
SCALES = (1.0, 3.0, 0.1, 3.0, 1.0, 0.1)
# The betas are Adam's defaults AS THE KERNELS RECEIVE THEM: the C ABI takes float, and fp32(0.999) = 0.99900001287 makes 1 - beta2
# 1.29e-5 (relative) smaller than 0.001.  p hardly notices (m / sqrt(v) and the bias correction move together; grad_clip_reference's
# tests compare p alone), v does: at |v| = 0.18 that is 2.3e-6, above ATOL before the kernel has rounded anything.  A float64 loop at the
# nominal betas would measure that quantisation, not the arithmetic under test, so the optimizer under test and the float64 loop are both
# given the fp32 values (tests/test_loss_scale_cpu.py::test_beta_quantisation_alone_exceeds_the_tolerance_in_v shows the 2.3e-6 on the host).
BETAS = (float(np.float32(0.9)), float(np.float32(0.999)))
GROWTH_INTERVAL = 3
INIT_SCALE, MIN_SCALE, MAX_SCALE = 1.0, 0.125, 4.0
N_STEPS = 12
BAD_STEPS = (4, 8, 9)
BAD_AT = (2, 11)                                                     # (parameter, flat element) that carries the inf
CLIPS = {"none": {}, "norm": dict(max_norm=MAX_NORM), "value": dict(clip_value=CLIP_VALUE)}
EXACT_K = (-6, 0, 10)                                                # the fixed scales 2^k of the exactness case
HUGE_INTERVAL = 10 ** 9


def scale_step(state, skipped, growth_interval, min_scale, max_scale, defect=None):
    """The state machine of one optimizer step."""
    s, streak, backoffs, growths = state
    if skipped:
        if defect != "streak_kept":
            streak = 0
        if s > min_scale:
            s, backoffs = max(s / 2, min_scale), backoffs + 1
    else:
        streak += 1
        if streak >= growth_interval:
            streak = 0
            if s < max_scale:
                s, growths = min(2 * s, max_scale), growths + 1
    return State(s, streak, backoffs, growths)


def schedule(skipped, init_scale=INIT_SCALE, growth_interval=GROWTH_INTERVAL, min_scale=MIN_SCALE, max_scale=MAX_SCALE, defect=None):
    """[State before step 0, State after step 0, ...] for the given skipped / applied sequence."""
    states = [State(float(init_scale), 0, 0, 0)]
    for sk in skipped:
        states.append(scale_step(states[-1], bool(sk), growth_interval, min_scale, max_scale, defect))
    return states


def true_steps(n=N_STEPS):
    """(initial parameters, the TRUE gradients of n steps): grad_clip_reference's case at the six magnitudes of SCALES, repeated."""
    return R.case_tensors(scales=(SCALES * ((n + len(SCALES) - 1) // len(SCALES)))[:n])


def fed_steps(steps, scales, bad=()):
    """What the optimizer is fed: g * s_t in fp32 (exact: s_t is a power of two), an inf planted at BAD_AT in the steps of `bad`."""
    out = []
    for t, (grads, s) in enumerate(zip(steps, scales)):
        gs = [g * float(s) for g in grads]
        if t in bad:
            gs[BAD_AT[0]].view(-1)[BAD_AT[1]] = float("inf")
        out.append(gs)
    return out


def schedule_case(bad=BAD_STEPS, n=N_STEPS, **kw):
    """(init, true gradients, fed gradients, states) of the schedule case: the fed gradients carry the scales of the CORRECT schedule."""
    init, steps = true_steps(n)
    states = schedule([t in bad for t in range(n)], **kw)
    return init, steps, fed_steps(steps, [st.scale for st in states[:-1]], bad), states


def rec_fp32(sumsq, scale, gscale=1.0, max_norm=math.inf, nblk=1):
    """What tri_loss_scale_step leaves in rec for a sum of squares of the FED gradient: (fp32(total), fp32(c) * fp32(1 / s))."""
    total = abs(float(gscale)) * (1.0 / scale) * math.sqrt(sumsq) if math.isfinite(sumsq) else sumsq
    c = np.float32(R.coefficient(total, max_norm)) if nblk else np.float32(1.0)
    with np.errstate(over="ignore"):
        return np.float32(total), c * np.float32(1.0 / scale)


def scaled_loop(init, fed, init_scale=INIT_SCALE, growth_interval=GROWTH_INTERVAL, min_scale=MIN_SCALE, max_scale=MAX_SCALE, lr=LR, wd=WD,
                max_norm=None, clip_value=None, gscale=1.0, defect=None, betas=BETAS):
    """The loop FusedAdam(loss_scale="dynamic") runs over the FED gradients, in float64.  Returns adam_loop's dict (p, m, v, applied) plus
    states (schedule()'s list), norms (the TRUE norm of every step, inf / NaN for a skipped one) and clipped.
    defect "norm_keeps_scale": the coefficient is formed from the norm of the fed gradient, the unscale left out;
    defect "scale_moves_first": the scale is moved before the coefficient and the multiplier are formed, so both use the NEXT scale;
    defect "streak_kept": a skipped step does not reset the streak."""
    state = State(float(init_scale), 0, 0, 0)
    states, norms, seen, clipped = [state], [], [], 0
    for grads in fed:
        fed_norm = R.total_norm(grads, gscale)
        skipped = not math.isfinite(fed_norm)
        after = scale_step(state, skipped, growth_interval, min_scale, max_scale, defect)
        s = after.scale if defect == "scale_moves_first" else state.scale
        total = fed_norm / s
        norms.append(total)
        coef = 1.0
        if max_norm is not None:
            coef = R.coefficient(fed_norm if defect == "norm_keeps_scale" else total, max_norm)
        clipped += coef < 1.0
        seen.append([g.detach().double() * (coef / s) for g in grads])            # an inf stays an inf: adam_loop skips that step
        state = after
        states.append(state)
    out = adam_loop(init, seen, lr=lr, wd=wd, betas=betas, clip_value=clip_value, gscale=gscale)
    out.update(states=states, norms=norms, clipped=int(clipped))
    return out
