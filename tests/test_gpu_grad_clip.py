"""GPU: gradient clipping decided on the device - the sum-of-squares / finalize kernels against float64 (tests/grad_clip_reference.py),
every update path of FusedAdam against the float64 clipped Adam loop, the measure-only mode bit for bit against an optimizer without
clipping, the overflow guard's precedence, the guard bands of the new entry points, and train.fit's trainer.gradient_clip_val wiring.

Tolerances (grad_clip_reference.py): parameters ATOL = 4 x 4.6e-7, the distance of torch's fp32 CPU loop from its float64 loop on the same
inputs; norms of random gradients relative 2^-22; norms and coefficients of integer-valued gradients EXACTLY, because their double sum
is exact in any order."""
import math

import numpy as np
import pytest
import torch

from tests import grad_clip_reference as R
from tests.guard_bands import recording, same_bytes

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tricolo_amd import ops

DEV = "cuda"
PATHS = ["segments", "flat", "per_param", "graph"]
NEW_ENTRY_POINTS = {"tri_grad_norm_blocks", "tri_grad_sumsq", "tri_grad_sumsq_segments", "tri_grad_clip_coef", "tri_adam_step_clipped",
                    "tri_adam_step_segments_clipped"}


# ================================================================================================ kernels
def offset_view(g):
    """g on the device, starting one float past a 16-byte boundary (scalar head and tail) when its size is not a multiple of 4."""
    if g.numel() % 4 == 0:
        return g.to(DEV)
    buf = torch.empty(g.numel() + 1, device=DEV)
    view = buf[1:]
    view.copy_(g)
    assert view.data_ptr() % 16 == 4
    return view


def finalize(partial, nblk, gscale=1.0, max_norm=math.inf, count0=0):
    rec = torch.full((2,), float("nan"), device=DEV)
    cnt = torch.full((1,), count0, dtype=torch.int32, device=DEV)
    ops.grad_clip_coef(partial, nblk, gscale, max_norm, rec, cnt)
    return rec.cpu().numpy(), int(cnt.item())


def flat_rec(g, **kw):
    nblk = ops.grad_norm_blocks(g.numel())
    partial = torch.full((nblk,), float("nan"), dtype=torch.float64, device=DEV)
    assert ops.grad_sumsq(g, partial) == nblk
    return finalize(partial, nblk, **kw) + (partial,)


def run_segments(segs, sizes, **kw):
    """segs: host tensors, or None for a NULL pointer; sizes: the size of every segment, the absent ones included."""
    dev = [None if s_ is None else s_.to(DEV) for s_ in segs]
    starts = [0]
    for n in sizes[:-1]:
        starts.append(starts[-1] + n)
    ptrs = torch.tensor([0 if d is None else d.data_ptr() for d in dev], dtype=torch.int64, device=DEV)
    st = torch.tensor(starts, dtype=torch.int64, device=DEV)
    total = sum(sizes)
    nblk = ops.grad_norm_blocks(total)
    partial = torch.full((nblk,), float("nan"), dtype=torch.float64, device=DEV)
    assert ops.grad_sumsq_segments(ptrs, st, total, partial) == nblk
    torch.cuda.synchronize()
    return finalize(partial, nblk, **kw) + (partial,)


def assert_rec_equal(rec, total, max_norm):
    want = np.array(R.rec_fp32(total, max_norm), dtype=np.float32)
    assert np.array_equal(rec, want, equal_nan=True), (rec.tolist(), want.tolist())


@pytest.mark.parametrize("n", R.FLAT_SIZES)
def test_flat_sum_of_integer_gradients_is_exact(n):
    """n = 0, one float4, two workgroups, a misaligned odd size (head and tail), and one full grid of 4096 x 256 float4 plus 1028."""
    g = R.integer_gradient(n, n)
    gd = offset_view(g)
    total = R.total_norm([g])
    assert ops.grad_norm_blocks(n) == min(4096, (n // 4 + 1 + 255) // 256)
    rec, cnt, partial = flat_rec(gd, max_norm=R.MAX_NORM, count0=3)
    assert_rec_equal(rec, total, R.MAX_NORM)
    assert cnt == (4 if total > R.MAX_NORM else 3)
    assert float(partial.sum().item()) == float((g.double() ** 2).sum())         # integers below 2^53: exact in any order
    rec, cnt, again = flat_rec(gd)                                   # measure only; and the same partials bit for bit
    assert_rec_equal(rec, total, math.inf)
    assert cnt == 0 and same_bytes(partial, again)


def test_segment_sum_skips_the_null_segment_and_equals_the_flat_call():
    segs = [R.integer_gradient(n, 100 + n) for n in R.SEG_SIZES]
    present = [segs[0], None, segs[2], segs[3]]
    total = R.total_norm(present)
    rec, cnt, _ = run_segments(present, R.SEG_SIZES, max_norm=R.MAX_NORM)
    assert_rec_equal(rec, total, R.MAX_NORM)
    assert cnt == 1
    flat, _, _ = flat_rec(torch.cat([s_ for s_ in present if s_ is not None]).to(DEV), max_norm=R.MAX_NORM)
    assert np.array_equal(rec, flat)
    everything, _, _ = run_segments(segs, R.SEG_SIZES, max_norm=R.MAX_NORM)      # all four present: the flat call on all four
    assert_rec_equal(everything, R.total_norm(segs), R.MAX_NORM)
    assert everything[0] != rec[0]


@pytest.mark.parametrize("n", [R.FLAT_SIZES[3], R.FLAT_SIZES[4]])
def test_sum_of_random_gradients(n):
    g = torch.randn(n, generator=torch.Generator().manual_seed(n)) * 3.0
    gd = offset_view(g)
    total = R.total_norm([g])
    rec, _, partial = flat_rec(gd, max_norm=R.MAX_NORM)
    print(f"n = {n}: rec[0] = {rec[0]!r}, float64 {total!r}, relative {abs(float(rec[0]) - total) / total:.3e}")
    assert abs(float(rec[0]) - total) <= R.NORM_RTOL * total
    assert abs(float(rec[1]) - R.coefficient(total, R.MAX_NORM)) <= R.NORM_RTOL * R.coefficient(total, R.MAX_NORM)
    _, _, again = flat_rec(gd, max_norm=R.MAX_NORM)
    assert same_bytes(partial, again)                                # no atomics, no ticket: two runs give the same bits
    if n % 4:                                                         # the segment form over the same values (sizes multiples of 4)
        m = n - n % 4
        sizes = (1024, 4, m - 1028)
        parts = list(torch.split(g[:m], sizes))
        seg, _, _ = run_segments(parts, sizes, max_norm=R.MAX_NORM)
        tot = R.total_norm(parts)
        assert abs(float(seg[0]) - tot) <= R.NORM_RTOL * tot


COEF_CASES = {
    # name: (gradient maker, gscale, max_norm)
    "below": (lambda g: g, 1.0, 1e6),
    "above": (lambda g: g, 1.0, 20.0),
    "measure_only": (lambda g: g, 1.0, math.inf),
    "all_zero": (lambda g: torch.zeros_like(g), 1.0, 20.0),
    "half_scale": (lambda g: g, 0.5, 20.0),
    "negative_scale": (lambda g: g, -0.5, 20.0),
    "one_inf": (lambda g: g.index_fill(0, torch.tensor([517]), float("inf")), 1.0, 20.0),
    "one_nan": (lambda g: g.index_fill(0, torch.tensor([1027]), float("nan")), 1.0, 20.0),
}


@pytest.mark.parametrize("name", list(COEF_CASES))
def test_coefficient_cases(name):
    make, gscale, max_norm = COEF_CASES[name]
    g = make(R.integer_gradient(1028, 1028))
    total = R.total_norm([g], gscale)
    rec, cnt, _ = flat_rec(g.to(DEV), gscale=gscale, max_norm=max_norm, count0=7)
    assert_rec_equal(rec, total, max_norm)
    clips = name in ("above", "half_scale", "negative_scale")
    assert (rec[1] < 1) == clips and cnt == 7 + clips
    if not clips:
        assert rec[1] == np.float32(1.0)                             # exactly 1.0f: the update then takes the unclipped step's bits
    if name == "one_inf":
        assert np.isposinf(rec[0])
    if name == "one_nan":
        assert np.isnan(rec[0])


def test_finalize_over_no_partials():
    rec, cnt = finalize(torch.zeros(1, dtype=torch.float64, device=DEV), 0, max_norm=R.MAX_NORM)
    assert rec.tolist() == [0.0, 1.0] and cnt == 0


# ================================================================================================ FusedAdam
def drive(path, init, steps, after=None, **opt_kw):
    """FusedAdam over `steps` on one of its update paths, shaped like test_adam_guard_skips_the_whole_step_on_a_non_finite_gradient
    (tests/test_gpu_ops.py).  The graph path warms up with one step on zero gradients, captures ONE step and replays it for every
    gradient.  after(i, opt, w) runs after step i (synchronised).  Returns (opt, w, the steps a reference has to take)."""
    from tricolo_amd.optim import FusedAdam
    w = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
    opt = FusedAdam(w, lr=opt_kw.pop("lr", R.LR), weight_decay=opt_kw.pop("weight_decay", R.WD), flatten=path != "per_param", **opt_kw)
    opt.prepare()
    kw = dict(reduce_fn=(lambda flat: None)) if path == "flat" else {}
    gbuf = [torch.zeros(t.shape, device=DEV) for t in init]
    for p, g_ in zip(w, gbuf):
        p.grad = g_
    graph, taken = None, list(steps)
    if path == "graph":
        opt.step()                                                   # warm-up on zero gradients (the reference takes it too)
        taken = [[torch.zeros(t.shape) for t in init]] + taken
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            opt.step()
    for i, grads in enumerate(steps):
        for b_, g_ in zip(gbuf, grads):
            b_.copy_(g_)
        if graph is not None:
            graph.replay()
        else:
            opt.step(**kw)
        torch.cuda.synchronize()
        if after is not None:
            after(i, opt, w)
    return opt, w, taken


def assert_close(w, ref_p, what=""):
    d = R.max_distance([p.detach().cpu() for p in w], ref_p)
    print(f"{what}: max |p - float64| = {d:.3e} (tolerance {R.ATOL:.3e})")
    assert d <= R.ATOL, f"{what}: {d:.3e} > {R.ATOL:.3e}"


@pytest.fixture(scope="module")
def case():
    return R.case_tensors()


@pytest.mark.parametrize("path", PATHS)
def test_every_update_path_clips_by_global_norm(path, case):
    """Six steps whose norms are about 51, 1463, 4.96, 1469, 49.8 and 5.01 under max_grad_norm = 20: four clip, two do not - on the graph
    path the SAME captured step clips one replay and leaves the next alone."""
    init, steps = case
    seen = []

    def after(i, opt, w):
        seen.append((opt.grad_norm(), opt.clipped_steps()))

    opt, w, taken = drive(path, init, steps, after, max_grad_norm=R.MAX_NORM)
    ref = R.adam_loop(init, taken, max_norm=R.MAX_NORM)
    assert ref["clipped"] == 4
    norms = ref["norms"][-len(steps):]
    for (got, count), want, so_far in zip(seen, norms, np.cumsum([n > R.MAX_NORM for n in norms])):
        assert abs(got - want) <= R.NORM_RTOL * want and count == so_far, (seen, norms)
    assert opt.clipped_steps() == 4 and opt.skipped_steps() == 0 and opt.nonfinite_skipped() == 0
    assert_close(w, ref["p"], path)
    assert int(opt.state_dict()["state"][0]["step"]) == len(taken)
    assert set(opt.state_dict()["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    # the test can tell: the unclipped loop ends far away
    free = R.adam_loop(init, taken)
    assert R.max_distance(free["p"], ref["p"]) > 1000 * R.ATOL


@pytest.mark.parametrize("path", PATHS)
def test_measure_only_keeps_the_bits_of_an_optimizer_without_clipping(path, case):
    init, steps = case
    norms = []
    opt, w, taken = drive(path, init, steps, lambda i, o, w_: norms.append(o.grad_norm()), max_grad_norm=math.inf)
    twin, wt, _ = drive(path, init, steps)
    for p, q in zip(w, wt):
        assert same_bytes(p.detach(), q.detach())
        assert same_bytes(opt.state[p]["exp_avg"], twin.state[q]["exp_avg"]) and same_bytes(opt.state[p]["exp_avg_sq"], twin.state[q]["exp_avg_sq"])
    want = R.adam_loop(init, taken)["norms"][-len(steps):]
    assert all(abs(a - b) <= R.NORM_RTOL * b for a, b in zip(norms, want)), (norms, want)
    assert opt.clipped_steps() == 0 and twin.grad_norm() is None and twin.clipped_steps() == 0


@pytest.mark.parametrize("path", PATHS)
def test_value_algorithm(path, case):
    """clip_grad_value = 0.5: the clamp comes BEFORE the weight decay (torch: clip_grad_value_, then Adam adds wd * p) - with the decay of
    0.1 this case uses, the other order ends 2e-2 away (tests/test_grad_clip_cpu.py)."""
    init, steps = case
    opt, w, taken = drive(path, init, steps, clip_grad_value=R.CLIP_VALUE, weight_decay=R.WD_VALUE)
    ref = R.adam_loop(init, taken, wd=R.WD_VALUE, clip_value=R.CLIP_VALUE)
    assert_close(w, ref["p"], path)
    assert opt.grad_norm() is None and opt.clipped_steps() == 0
    assert R.max_distance(R.adam_loop(init, taken, wd=R.WD_VALUE)["p"], ref["p"]) > 1000 * R.ATOL


@pytest.mark.parametrize("path", PATHS)
def test_a_step_the_guard_skips_stays_skipped_and_is_not_counted_as_clipped(path, case):
    init, steps = case
    steps = [[g.clone() for g in gs] for gs in steps]
    steps[1][2].view(-1)[11] = float("inf")                          # a step that would have clipped (norm 1463)
    state = {}

    def after(i, opt, w):
        snap = [p.detach().clone() for p in w] + [opt.state[p][k].clone() for p in w for k in ("exp_avg", "exp_avg_sq")]
        if i == 1:
            assert all(torch.equal(a, b) for a, b in zip(snap, state["snap"]))
            assert opt.skipped_steps() == 1 and opt.clipped_steps() == state["clipped"] and math.isinf(opt.grad_norm())
        state["snap"], state["clipped"] = snap, opt.clipped_steps()

    opt, w, taken = drive(path, init, steps, after, max_grad_norm=R.MAX_NORM)
    ref = R.adam_loop(init, taken, max_norm=R.MAX_NORM)
    assert ref["clipped"] == 3 and ref["applied"] == len(taken) - 1
    assert opt.skipped_steps() == 1 and opt.clipped_steps() == 3 and opt.nonfinite_skipped() == 0
    assert_close(w, ref["p"], path)


def test_set_gradient_clip_inside_a_capture_needs_the_buffers(case):
    from tricolo_amd.optim import FusedAdam
    init, _ = case
    w = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
    for p in w:
        p.grad = torch.zeros_like(p)
    opt = FusedAdam(w, lr=R.LR)
    opt.prepare()
    opt.step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    raised = False
    with torch.cuda.graph(graph):
        try:
            opt.set_gradient_clip(R.MAX_NORM)
        except RuntimeError as e:
            raised = "capture" in str(e)
        opt.step()
    assert raised and opt._clip is None
    opt.set_gradient_clip(R.MAX_NORM)                                # eager: allocates
    graph2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph2):
        opt.set_gradient_clip(5.0)                                   # buffers exist: allowed
        opt.step()
    graph2.replay()
    torch.cuda.synchronize()
    assert opt.grad_norm() == 0.0


@pytest.mark.parametrize("path", PATHS)
def test_default_step_launches_none_of_the_new_entry_points(path, case):
    init, steps = case
    with recording() as rec:
        drive(path, init, steps[:2])
    assert rec.calls and not NEW_ENTRY_POINTS & set(rec.calls), sorted(NEW_ENTRY_POINTS & set(rec.calls))
    with recording() as rec:                                         # (and the switch does switch)
        drive(path, init, steps[:2], max_grad_norm=R.MAX_NORM)
    assert {"tri_grad_clip_coef", "tri_grad_norm_blocks"} <= set(rec.calls)
    order = [c for c in rec.calls if c.startswith(("tri_adam", "tri_grad")) and c != "tri_grad_norm_blocks"]
    last = order[-order[::-1].index("tri_adam_tick") - 1:]           # the last step: tick, sums, finalize, update(s)
    assert last[0] == "tri_adam_tick" and last[1].startswith("tri_grad_sumsq") and "tri_grad_clip_coef" in last
    assert all(c.endswith("_clipped") for c in last[last.index("tri_grad_clip_coef") + 1:]) and last[-1].endswith("_clipped")


# ================================================================================================ guard bands
def test_new_entry_points_stay_inside_their_operands():
    """Every operand, the exact-size partial buffer, rec and clipped between poisoned margins (tests/guard_bands.py), under 0xFF and 0x00
    bands: same bits both times, no band touched, results as the reference has them."""
    from tests.test_gpu_guard_bands import twice
    n = R.FLAT_SIZES[3]
    gflat = R.integer_gradient(n, n)
    segs = [R.integer_gradient(s_, 100 + s_) for s_ in R.SEG_SIZES]
    starts = [0, 4, 264, 1288]
    ns = sum(R.SEG_SIZES)
    gen = torch.Generator().manual_seed(5)
    p0, ps0 = torch.randn(n, generator=gen), torch.randn(ns, generator=gen)
    hp = (R.LR, 0.9, 0.999, 1e-8, R.WD_VALUE)

    def body(g):
        out = {}
        buf = g.put(torch.cat([torch.zeros(1), gflat]))
        view = buf[1:]
        assert view.data_ptr() % 16 == 4
        nblk = ops.grad_norm_blocks(n)
        partial = g.put(torch.zeros(nblk, dtype=torch.float64))
        rec, cnt = g.put(torch.zeros(2)), g.put(torch.zeros(1, dtype=torch.int32))
        ops.grad_sumsq(view, partial)
        ops.grad_clip_coef(partial, nblk, 1.0, R.MAX_NORM, rec, cnt)
        out.update(partial=partial, rec=rec, cnt=cnt)
        for tag, kw in (("norm", dict(coef_dev=rec[1:])), ("value", dict(clip_value=R.CLIP_VALUE))):
            pd, m, v = g.put(p0), g.put(torch.zeros(n)), g.put(torch.zeros(n))
            step = g.put(torch.zeros(4, dtype=torch.int32))
            ops.adam_tick(step)
            ops.adam_step_clipped(pd, g.put(gflat), m, v, step, *hp, **kw)
            out.update({f"p_{tag}": pd, f"m_{tag}": m, f"v_{tag}": v, f"step_{tag}": step})
        dev = [g.put(segs[0]), None, g.put(segs[2]), g.put(segs[3])]
        ptrs = g.put(torch.tensor([0 if d is None else d.data_ptr() for d in dev], dtype=torch.int64))
        st = g.put(torch.tensor(starts, dtype=torch.int64))
        nblk_s = ops.grad_norm_blocks(ns)
        partial_s = g.put(torch.zeros(nblk_s, dtype=torch.float64))
        rec_s, cnt_s = g.put(torch.zeros(2)), g.put(torch.zeros(1, dtype=torch.int32))
        ops.grad_sumsq_segments(ptrs, st, ns, partial_s)
        ops.grad_clip_coef(partial_s, nblk_s, 1.0, R.MAX_NORM, rec_s, cnt_s)
        out.update(partial_s=partial_s, rec_s=rec_s, cnt_s=cnt_s)
        for tag, kw in (("norm", dict(coef_dev=rec_s[1:])), ("value", dict(clip_value=R.CLIP_VALUE))):
            ps, ms, vs = g.put(ps0), g.put(torch.zeros(ns)), g.put(torch.zeros(ns))
            step = g.put(torch.zeros(4, dtype=torch.int32))
            ops.adam_tick(step)
            ops.adam_step_segments_clipped(ps, ptrs, st, ms, vs, step, *hp, **kw)
            out.update({f"ps_{tag}": ps, f"ms_{tag}": ms, f"step_s_{tag}": step})
        assert NEW_ENTRY_POINTS <= set(g.lib.calls)
        return out

    got = twice(body)
    assert_rec_equal(got["rec"].numpy(), R.total_norm([gflat]), R.MAX_NORM)
    present = [segs[0], None, segs[2], segs[3]]
    assert_rec_equal(got["rec_s"].numpy(), R.total_norm(present), R.MAX_NORM)
    assert got["cnt"].item() == 1 and got["cnt_s"].item() == 1
    # one step from zero moments: |p| < 4, so the fp32 result is within half an ulp (1.2e-7) of the float64 one plus the update's own rounding
    # (lr * 1e-6 = 1e-8) - torch's fp32 CPU step sits 1.1e-7 away; 2e-7 as tests/test_gpu_guard_bands.py::test_adam_kernels allows at this size
    assert float(p0.abs().max()) < 4 and float(ps0.abs().max()) < 4
    for tag, kw in (("norm", dict(max_norm=R.MAX_NORM)), ("value", dict(clip_value=R.CLIP_VALUE))):
        ref = R.adam_loop([p0], [[gflat]], lr=R.LR, wd=R.WD_VALUE, **kw)
        assert float((got[f"p_{tag}"].double() - ref["p"][0]).abs().max()) <= 2e-7
        assert got[f"step_{tag}"].tolist() == [1, 0, 0, 0]
        parts = list(torch.split(ps0, R.SEG_SIZES))
        ref = R.adam_loop(parts, [present], lr=R.LR, wd=R.WD_VALUE, **kw)
        assert float((got[f"ps_{tag}"].double() - torch.cat(ref["p"])).abs().max()) <= 2e-7
        assert torch.equal(got[f"ps_{tag}"][4:264], ps0[4:264]) and not bool(got[f"ms_{tag}"][4:264].any())      # the NULL segment: untouched
        assert got[f"step_s_{tag}"].tolist() == [1, 0, 0, 0]


# ================================================================================================ train.fit
class OneLinear(torch.nn.Module):
    """A module with the hooks fit() drives: one linear layer, a squared-output loss."""

    def __init__(self, make_opt):
        super().__init__()
        torch.manual_seed(3)
        self.lin = torch.nn.Linear(16, 8)
        self.make_opt = make_opt

    def training_step(self, batch, step):
        return self.lin(batch).pow(2).mean()

    def configure_optimizers(self):
        return self.make_opt(self.parameters())


def fit_batches(epoch):
    gen = torch.Generator().manual_seed(40 + epoch)
    return [(torch.randn(32, 16, generator=gen) * s).to(DEV) for s in (1.0, 50.0, 0.02, 50.0, 1.0)]


@pytest.mark.parametrize("which", ["fused", "torch"])
@pytest.mark.parametrize("algorithm", ["norm", "value"])
def test_fit_reads_the_trainer_keys(which, algorithm):
    """+trainer.gradient_clip_val (and gradient_clip_algorithm) reach FusedAdam through set_gradient_clip and any other optimizer through
    torch.nn.utils between backward() and step(); the history carries grad_norm and clipped_steps with the norm algorithm only."""
    from tricolo_amd import config as tcfg
    from tricolo_amd.optim import FusedAdam
    from tricolo_amd.train import fit
    clip = 0.5 if algorithm == "norm" else 0.01
    lr = 1e-2
    make = (lambda ps: FusedAdam(ps, lr=lr)) if which == "fused" else (lambda ps: torch.optim.Adam(ps, lr=lr))
    cfg = tcfg.compose(overrides=[f"+trainer.gradient_clip_val={clip}", f"+trainer.gradient_clip_algorithm={algorithm}", "trainer.max_epochs=2"])
    assert tcfg.compose().trainer.get("gradient_clip_val") is None               # not a default: it arrives as an override
    net = OneLinear(make)
    out = fit(net, cfg, fit_batches, device=DEV, log=lambda *_: None)
    # the manual loop
    twin = OneLinear(make).to(DEV)
    opt = twin.configure_optimizers()
    if which == "fused":
        opt.set_gradient_clip(clip, algorithm)
    norms, clipped, hist = [], 0, []
    for epoch in range(2):
        for batch in fit_batches(epoch):
            opt.zero_grad(set_to_none=True)
            twin.training_step(batch, 0).backward()
            total = R.total_norm([p.grad.cpu() for p in twin.parameters()])
            clipped += R.coefficient(total, clip) < 1.0
            if which == "torch":
                (torch.nn.utils.clip_grad_norm_ if algorithm == "norm" else torch.nn.utils.clip_grad_value_)(list(twin.parameters()), clip)
            opt.step()
        hist.append((total, int(clipped)))
    torch.cuda.synchronize()
    for p, q in zip(net.parameters(), twin.parameters()):
        assert torch.equal(p.detach(), q.detach())
    if algorithm == "norm":
        assert 0 < hist[-1][1] < 10                                  # the case clips some steps and leaves others alone
    # FusedAdam's norm is the kernel's (NORM_RTOL); the other is torch's own fp32 norm of 136 elements
    rtol = R.NORM_RTOL if which == "fused" else 1e-5
    assert len(out["history"]) == 2
    for rec, (total, count) in zip(out["history"], hist):
        if algorithm == "norm":
            assert abs(rec["grad_norm"] - total) <= rtol * total and rec["clipped_steps"] == count, (rec, total, count)
        else:
            assert "grad_norm" not in rec and "clipped_steps" not in rec
    # and it mattered: an unclipped twin ends elsewhere
    free = OneLinear(make).to(DEV)
    fopt = free.configure_optimizers()
    for epoch in range(2):
        for batch in fit_batches(epoch):
            fopt.zero_grad(set_to_none=True)
            free.training_step(batch, 0).backward()
            fopt.step()
    assert not torch.equal(free.lin.weight.detach(), net.lin.weight.detach())
