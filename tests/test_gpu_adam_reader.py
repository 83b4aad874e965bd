"""GPU: the optimizer kernels read a gradient in two ways - flat (scalar head up to a 16-byte boundary, float4 body, scalar tail) and
through a (pointer, start) segment table - and the guard, the sum of squares and the update each sit on both (csrc/adam.hip).  These
tests pin what the readers share: the four update entry points agree bit for bit on the same values, the table's limits (one segment,
1024 segments, NULL pointers, the argument errors) and the flat split's limits (head only, head and tail around an empty body).

Gradients are integer-valued (tests/grad_clip_reference.py): their sum of squares is exact in double in any order, so every norm is
compared with ==, and the update comparisons are between kernels on the same inputs, so they are byte comparisons too."""
import math

import numpy as np
import pytest
import torch

from tests import grad_clip_reference as R
from tests.guard_bands import same_bytes

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tricolo_amd import ops
    from tests.test_gpu_grad_clip import assert_rec_equal, finalize, flat_rec

DEV = "cuda"
GSCALE = 0.5


def hp(wd):
    return (R.LR, 0.9, 0.999, 1e-8, wd)                              # lr, b1, b2, eps, wd


def seg_table(g, sizes, null=()):
    """Device (pointers, starts) of the segments `sizes` laid end to end in the device gradient g; the segments in `null` get a NULL pointer."""
    starts = [0]
    for n in sizes[:-1]:
        starts.append(starts[-1] + n)
    assert g.data_ptr() % 16 == 0 and all(s_ % 4 == 0 for s_ in sizes)
    ptrs = [0 if i in null else g.data_ptr() + 4 * s_ for i, s_ in enumerate(starts)]
    return torch.tensor(ptrs, dtype=torch.int64, device=DEV), torch.tensor(starts, dtype=torch.int64, device=DEV)


def state(n, seed):
    """(p, m, v) on the host: moments that are not zero, so that an element a kernel must leave alone has bytes to keep."""
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.1, torch.rand(n, generator=gen)


def run_steps(update, pmv, grads):
    """tick + update(p, g, m, v, step) for every device gradient; returns (p, m, v, step) on the device, synchronised."""
    p, m, v = (t.to(DEV) for t in pmv)
    step = torch.zeros(4, dtype=torch.int32, device=DEV)
    for g in grads:
        ops.adam_tick(step)
        update(p, g, m, v, step)
    torch.cuda.synchronize()
    return p, m, v, step


def flat_update(wd, gscale=GSCALE, **clip):
    if not clip:
        return lambda p, g, m, v, step: ops.adam_step(p, g, m, v, step, *hp(wd), gscale)
    return lambda p, g, m, v, step: ops.adam_step_clipped(p, g, m, v, step, *hp(wd), gscale, **clip)


def seg_update(wd, sizes, null=(), gscale=GSCALE, **clip):
    def update(p, g, m, v, step):
        ptrs, starts = seg_table(g, sizes, null)
        if not clip:
            ops.adam_step_segments(p, ptrs, starts, m, v, step, *hp(wd), gscale)
        else:
            ops.adam_step_segments_clipped(p, ptrs, starts, m, v, step, *hp(wd), gscale, **clip)
    return update


def assert_same_run(a, b, what):
    for name, x, y in zip(("p", "m", "v", "step"), a, b):
        assert same_bytes(x, y), f"{what}: {name} differs"


# ================================================================================================ 1. the update paths agree
@pytest.mark.parametrize("wd", [0.0, R.WD_VALUE])
@pytest.mark.parametrize("mode", ["plain", "clamp", "coef"])
def test_update_paths_agree_bit_for_bit(mode, wd):
    """Three steps over R.SEG_SIZES, every segment present, through adam_step, adam_step_segments and the two *_clipped forms: the same
    bytes in p, m, v and the step record.  Element 5 is NaN in every step: every form refuses it, leaves its p, m, v alone and counts it.

    plain: the clipped forms run with no coefficient and no clamp.  clamp: the clipped forms with clip_value = 0.5.  coef: the clipped
    forms with a device coefficient of 0.25f - and, 0.5f * 0.25f being exact, the unclipped forms at gscale 0.125 are the same arithmetic.

    Within one reader every pair agrees.  ACROSS the readers the pairs agree with the clamp, and without weight decay; with wd != 0 and no
    clamp the compiler contracts g * gmul + wd * p as fma(wd, p, g * gmul) in the flat kernel and as fma(gmul, g, wd * p) in the segmented
    one (csrc/adam.hip), one rounding against two, and a few elements differ in the last bit - measured before the kernels were
    touched.  Those pairs are not compared; the wd = 0 cases pin everything else of the two bodies against each other."""
    n = sum(R.SEG_SIZES)
    pmv = state(n, 21)
    grads = [R.integer_gradient(n, 30 + s_) for s_ in range(3)]
    for g in grads:
        g[5] = float("nan")
    grads = [g.to(DEV) for g in grads]
    if mode == "plain":
        clip = dict(coef_dev=None, clip_value=math.inf)
        flat = [flat_update(wd), flat_update(wd, **clip)]
        seg = [seg_update(wd, R.SEG_SIZES), seg_update(wd, R.SEG_SIZES, **clip)]
    elif mode == "clamp":
        flat = [flat_update(wd, clip_value=R.CLIP_VALUE)]
        seg = [seg_update(wd, R.SEG_SIZES, clip_value=R.CLIP_VALUE)]
    else:
        coef = torch.tensor([0.25], device=DEV)
        flat = [flat_update(wd, coef_dev=coef), flat_update(wd, gscale=GSCALE * 0.25)]
        seg = [seg_update(wd, R.SEG_SIZES, coef_dev=coef), seg_update(wd, R.SEG_SIZES, gscale=GSCALE * 0.25)]
    flat = [run_steps(u, pmv, grads) for u in flat]
    seg = [run_steps(u, pmv, grads) for u in seg]
    for runs, reader in ((flat, "flat"), (seg, "segments")):
        assert runs[0][3].tolist() == [3, 3, 0, 0]
        for name, x, x0 in zip("pmv", runs[0], pmv):
            assert same_bytes(x[5:6], x0[5:6].to(DEV)), f"{reader}: {name} of the refused element changed"
        for other in runs[1:]:
            assert_same_run(other, runs[0], f"{reader}, {mode}: clipped against unclipped entry point")
    if wd == 0.0 or mode == "clamp":
        assert_same_run(seg[0], flat[0], f"{mode}: segments against flat")
    if mode != "plain":                                              # the clamp / the coefficient did act
        assert not same_bytes(flat[0][0], run_steps(flat_update(wd), pmv, grads)[0])


# ================================================================================================ 2. table edges
@pytest.mark.parametrize("nseg, size", [(1, 1028), (1024, 4)])
def test_table_edges(nseg, size):
    """One segment (two workgroups of float4s) and the limit of 1024 segments of one float4 each, every third pointer NULL: sum of
    squares, update and guard over the table against the flat calls on the elements that are present.  The update runs without weight
    decay: with it the two kernels differ in the last bit of a few elements (test_update_paths_agree_bit_for_bit)."""
    sizes, n = (size,) * nseg, nseg * size
    null = {i for i in range(nseg) if i % 3 == 2}
    keep = torch.tensor([i not in null for i in range(nseg)]).repeat_interleave(size)
    assert nseg == 1 or 0 < len(null) < nseg and nseg - 1 not in null
    g = R.integer_gradient(n, nseg)
    gd = g.to(DEV)
    ptrs, starts = seg_table(gd, sizes, null)
    # the sum of squares: exact, and the flat call's record
    nblk = ops.grad_norm_blocks(n)
    partial = torch.full((nblk,), float("nan"), dtype=torch.float64, device=DEV)
    assert ops.grad_sumsq_segments(ptrs, starts, n, partial) == nblk
    rec, _ = finalize(partial, nblk)
    assert_rec_equal(rec, R.total_norm([g[keep]]), math.inf)
    assert float(partial.sum().item()) == float((g[keep].double() ** 2).sum())
    assert np.array_equal(rec, flat_rec(g[keep].to(DEV))[0])
    # the update: the flat kernel's bytes where a gradient is present, nothing written under a NULL pointer
    pmv = state(n, 22)
    got = run_steps(seg_update(0.0, sizes, null), pmv, [gd])
    flat = run_steps(flat_update(0.0), [t[keep] for t in pmv], [g[keep].to(DEV)])
    kd = keep.to(DEV)
    for name, x, y, x0 in zip("pmv", got, flat, pmv):
        assert same_bytes(x[kd], y), f"{name}: present segments differ from the flat update"
        assert same_bytes(x[~kd], x0[~keep].to(DEV)), f"{name}: written under a NULL segment"
    assert got[3].tolist() == flat[3].tolist() == [1, 0, 0, 0]
    # the guard sees the last element of the last present segment, and flags nothing in a finite gradient
    for last, flagged in ((float("inf"), 1), (7.0, 0)):
        gd[n - 1] = last
        step = torch.zeros(4, dtype=torch.int32, device=DEV)
        ops.adam_guard_segments(ptrs, starts, n, step)
        assert step.tolist() == [0, 0, flagged, 0]


def test_segment_entry_points_refuse_a_bad_table():
    """More than 1024 segments, or a size that is no multiple of 4: an argument error whose message starts with the entry point's name."""
    buf = torch.zeros(1025, dtype=torch.int64, device=DEV)
    f = torch.zeros(8, device=DEV)
    step = torch.zeros(4, dtype=torch.int32, device=DEV)
    partial = torch.zeros(8, dtype=torch.float64, device=DEV)
    for tab, n in ((buf, 4100), (buf[:1], 6)):
        calls = {
            "tri_adam_guard_segments": lambda: ops.adam_guard_segments(tab, tab, n, step),
            "tri_adam_step_segments": lambda: ops.adam_step_segments(f[:n], tab, tab, f, f, step, *hp(0.0)),
            "tri_grad_sumsq_segments": lambda: ops.grad_sumsq_segments(tab, tab, n, partial),
            "tri_adam_step_segments_clipped": lambda: ops.adam_step_segments_clipped(f[:n], tab, tab, f, f, step, *hp(0.0), clip_value=R.CLIP_VALUE),
        }
        for name, call in calls.items():
            with pytest.raises(RuntimeError, match=rf"\(code -1\): {name}: "):
                call()
    torch.cuda.synchronize()
    assert step.tolist() == [0, 0, 0, 0] and not bool(f.any())


# ================================================================================================ 3. flat reader edges
def misaligned(g):
    """g on the device in a view that starts 4 bytes past a 16-byte boundary: the scalar head is 3 elements long."""
    buf = torch.zeros(g.numel() + 1, device=DEV)
    view = buf[1:]
    view.copy_(g)
    assert g.numel() == 0 or view.data_ptr() % 16 == 4
    return view


@pytest.mark.parametrize("n", [0, 1, 3, 5, 1031])
def test_flat_reader_edges(n):
    """Head only (n <= 3), head and tail around an empty body (n = 5), and a head in front of 257 float4s, the second workgroup's
    among them (n = 1031): the sum of squares is exact, the guard finds a non-finite value at index 0, at n - 1 and in the body, and
    flags nothing otherwise."""
    g = R.integer_gradient(n, 50 + n)
    gd = misaligned(g)
    rec, cnt, partial = flat_rec(gd)
    assert_rec_equal(rec, R.total_norm([g]), math.inf)
    assert cnt == 0 and float(partial.sum().item()) == float((g.double() ** 2).sum())
    spots = {0, n - 1} | ({3 + 4 * 130, 3 + 4 * 256 + 2} if n == 1031 else set())
    for spot in [None] + sorted(s_ for s_ in spots if 0 <= s_ < n):
        step = torch.zeros(4, dtype=torch.int32, device=DEV)
        if spot is not None:
            bad = g.clone()
            bad[spot] = float("nan") if spot % 2 else float("inf")
            gd = misaligned(bad)
        ops.adam_guard(gd, step)
        assert step.tolist() == [0, 0, int(spot is not None), 0], spot
