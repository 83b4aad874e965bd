"""GPU: dynamic loss scaling decided on the device (FusedAdam(loss_scale="dynamic"), tri_loss_scale_step) against
tests/loss_scale_reference.py: the schedule and the float64 loop on every update path with each clipping rule, bit identity with an
optimizer without the option at fixed scales, the floor and the ceiling, the kernel alone and between guard bands, a captured step that
backs off and recovers while it replays, the checkpoint round trip, train.fit on the real towers in f16 and the data-parallel paths.

Tolerances (grad_clip_reference.py, unchanged): parameters and moments ATOL = 4 x 4.6e-7, norms relative 2^-22; schedules, counters and
everything at a fixed power-of-two scale EXACTLY - every factor is a power of two and nothing leaves the normal range.  The optimizer and
the float64 loop are both given Adam's default betas as fp32 numbers (loss_scale_reference.BETAS says why: with 0.999 in the float64 loop
the quantisation of beta2 at the C ABI alone puts v 2.284e-6 away, measured, on every update path without clipping)."""
import math

import numpy as np
import pytest
import torch

from tests import grad_clip_reference as R
from tests import loss_scale_reference as L
from tests.guard_bands import recording, same_bytes

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tricolo_amd import ops

DEV = "cuda"
PATHS = ["segments", "flat", "per_param"]                            # the three update paths of test_gpu_grad_clip.py's PATHS
SCHEDULE = dict(loss_scale="dynamic", loss_scale_init=L.INIT_SCALE, loss_scale_growth_interval=L.GROWTH_INTERVAL,
                loss_scale_min=L.MIN_SCALE, loss_scale_max=L.MAX_SCALE)
CLIP_KW = {"none": {}, "norm": dict(max_grad_norm=R.MAX_NORM), "value": dict(clip_grad_value=R.CLIP_VALUE)}


def make_opt(path, init, **kw):
    from tricolo_amd.optim import FusedAdam
    w = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
    # (betas: Adam's defaults as the kernels receive them, fp32 numbers - the float64 loop is given the same; loss_scale_reference.BETAS)
    opt = FusedAdam(w, lr=kw.pop("lr", R.LR), betas=L.BETAS, weight_decay=kw.pop("weight_decay", R.WD), flatten=path != "per_param", **kw)
    opt.prepare()
    return opt, w


def drive(path, init, fed, after=None, **kw):
    """FusedAdam over the fed gradients on one update path (test_gpu_grad_clip.py's drive, eager)."""
    opt, w = make_opt(path, init, **kw)
    step_kw = dict(reduce_fn=(lambda flat: None)) if path == "flat" else {}
    gbuf = [torch.zeros(t.shape, device=DEV) for t in init]
    for p, g in zip(w, gbuf):
        p.grad = g
    for i, grads in enumerate(fed):
        for b, g in zip(gbuf, grads):
            b.copy_(g)
        opt.step(**step_kw)
        if after is not None:
            torch.cuda.synchronize()
            after(i, opt, w)
    torch.cuda.synchronize()
    return opt, w


def scale_state(opt):
    streak, backoffs, growths = opt._ls_cnt.tolist()
    return L.State(opt.loss_scale(), streak, backoffs, growths)


def moments(opt, w, key):
    return [opt.state[p][key].detach().cpu() for p in w]


@pytest.fixture(scope="module")
def case():
    return L.schedule_case()


@pytest.fixture(scope="module")
def references(case):
    """The float64 loops of the schedule case, one per clipping rule: computed once, shared, never written to."""
    init, _, fed, _ = case
    return {clip: L.scaled_loop(init, fed, wd=R.WD_VALUE if clip == "value" else R.WD, **L.CLIPS[clip]) for clip in L.CLIPS}


# ================================================================================================ schedule
@pytest.mark.parametrize("clip", list(CLIP_KW))
@pytest.mark.parametrize("path", PATHS)
def test_schedule_follows_the_reference_on_every_update_path(path, clip, case, references):
    """Twelve steps fed g_true * s_t, overflows planted in steps 4, 8 and 9, growth every three applied steps: after EVERY step the scale,
    the streak, both counters and the applied / skipped counts equal the reference's; p, m, v end within ATOL of the float64 loop."""
    init, steps, fed, states = case
    ref = references[clip]
    assert ref["states"] == states
    seen = []

    def after(i, opt, w):
        seen.append((scale_state(opt), int(opt._step_dev[0].item()), opt.skipped_steps(), opt.grad_norm()))

    opt, w = drive(path, init, fed, after, weight_decay=R.WD_VALUE if clip == "value" else R.WD, **SCHEDULE, **CLIP_KW[clip])
    skipped = np.cumsum([t in L.BAD_STEPS for t in range(L.N_STEPS)])
    for t, (state, applied, skips, norm) in enumerate(seen):
        assert state == states[t + 1], (t, state, states[t + 1])
        assert (applied, skips) == (t + 1 - skipped[t], skipped[t]), (t, applied, skips)
        if clip == "norm":                                           # the TRUE norm: the scale is divided out
            want = ref["norms"][t]
            assert (math.isinf(norm) and math.isinf(want)) if t in L.BAD_STEPS else abs(norm - want) <= R.NORM_RTOL * want, (t, norm, want)
        else:
            assert norm is None
    assert (opt.loss_scale(), opt.scale_backoffs(), opt.scale_growths()) == (0.5, 3, 2) and opt.nonfinite_skipped() == 0
    assert opt.clipped_steps() == ref["clipped"]
    for name, got, want in (("p", [p.detach().cpu() for p in w], ref["p"]), ("m", moments(opt, w, "exp_avg"), ref["m"]),
                            ("v", moments(opt, w, "exp_avg_sq"), ref["v"])):
        d = R.max_distance(got, want)
        print(f"{path} / {clip}: max |{name} - float64| = {d:.3e} (tolerance {R.ATOL:.3e})")
        assert d <= R.ATOL, f"{path} / {clip} {name}: {d:.3e} > {R.ATOL:.3e}"


# ================================================================================================ exactness
@pytest.mark.parametrize("clip", list(CLIP_KW))
@pytest.mark.parametrize("path", PATHS)
def test_a_fixed_power_of_two_scale_keeps_the_bits_of_an_optimizer_without_the_option(path, clip, case):
    """Scale 2^k, gradients pre-multiplied by 2^k: p, m, v (and the norm record) equal, bit for bit, an optimizer without the option fed the
    plain gradients.  Derived, not measured: the sums of squares scale by 2^2k exactly, so total and c are the same doubles; rec[1] =
    c * 2^-k and g * 2^k * (c * 2^-k) round where g * c rounds."""
    init, steps, _, _ = case
    steps = steps[:6]
    wd = R.WD_VALUE if clip == "value" else R.WD
    twin, wt = drive(path, init, steps, weight_decay=wd, **CLIP_KW[clip])
    for k in L.EXACT_K:
        s = 2.0 ** k
        fed = [[g * s for g in gs] for gs in steps]
        opt, w = drive(path, init, fed, weight_decay=wd, loss_scale="dynamic", loss_scale_init=s, loss_scale_growth_interval=L.HUGE_INTERVAL,
                       loss_scale_min=2.0 ** min(L.EXACT_K), loss_scale_max=2.0 ** max(L.EXACT_K), **CLIP_KW[clip])
        assert scale_state(opt) == L.State(s, 6, 0, 0)
        for p, q in zip(w, wt):
            assert same_bytes(p.detach(), q.detach()), (k, "p")
            assert same_bytes(opt.state[p]["exp_avg"], twin.state[q]["exp_avg"]), (k, "m")
            assert same_bytes(opt.state[p]["exp_avg_sq"], twin.state[q]["exp_avg_sq"]), (k, "v")
        if clip == "norm":
            assert same_bytes(opt._clip_rec[:1], twin._clip_rec[:1]) and opt.clipped_steps() == twin.clipped_steps() == 4
            assert float(opt._clip_rec[1].item()) == float(twin._clip_rec[1].item()) / s


# ================================================================================================ option off
@pytest.mark.parametrize("path", PATHS)
def test_without_the_option_the_new_entry_point_is_never_launched(path, case):
    init, steps, _, _ = case
    for kw in CLIP_KW.values():
        with recording() as rec:
            opt, _ = drive(path, init, steps[:2], **kw)
        assert rec.calls and "tri_loss_scale_step" not in rec.calls
        assert opt.backward_seed() is ops.one(opt._params[0].device) and opt.loss_scale() is None and "loss_scale" not in opt.state_dict()
    for clip, kw in CLIP_KW.items():                                 # (and the switch does switch: it stands where the finalize stood)
        with recording() as rec:
            drive(path, init, steps[:2], loss_scale="dynamic", **kw)
        order = [c for c in rec.calls if c.startswith(("tri_adam", "tri_grad", "tri_loss")) and c != "tri_grad_norm_blocks"]
        last = order[-order[::-1].index("tri_adam_tick") - 1:]       # the last step: tick, (sums,) scale step, update(s)
        assert "tri_grad_clip_coef" not in rec.calls and last.count("tri_loss_scale_step") == 1
        i = last.index("tri_loss_scale_step")
        assert all(c.startswith("tri_grad_sumsq") for c in last[1:i]) and (i > 1) == (clip == "norm")
        assert len(last) > i + 1 and all(c.endswith("_clipped") for c in last[i + 1:])


# ================================================================================================ floor and ceiling
@pytest.mark.parametrize("path", PATHS)
def test_floor_and_ceiling(path, case):
    init, steps, _, _ = case
    kw = dict(loss_scale="dynamic", loss_scale_growth_interval=2, loss_scale_min=0.25, loss_scale_max=0.5)
    # at the floor an overflowed step is still skipped; the scale and the back-off count stay
    fed = L.fed_steps(steps[:3], [0.25] * 3, bad=(1,))
    snaps = []

    def after(i, opt, w):
        snaps.append(([p.detach().clone() for p in w], scale_state(opt), opt.skipped_steps()))

    drive(path, init, fed, after, loss_scale_init=0.25, **kw)
    assert [s[1] for s in snaps] == [L.State(0.25, 1, 0, 0), L.State(0.25, 0, 0, 0), L.State(0.25, 1, 0, 0)]
    assert [s[2] for s in snaps] == [0, 1, 1]
    assert all(torch.equal(a, b) for a, b in zip(snaps[0][0], snaps[1][0])) and not torch.equal(snaps[1][0][0], snaps[2][0][0])
    # at the ceiling the streak wraps without growth
    snaps.clear()
    drive(path, init, L.fed_steps(steps[:3], [0.5] * 3), after, loss_scale_init=0.5, **kw)
    assert [s[1] for s in snaps] == [L.State(0.5, 1, 0, 0), L.State(0.5, 0, 0, 0), L.State(0.5, 1, 0, 0)]
    # (and one below the ceiling it grows to it and no further)
    snaps.clear()
    drive(path, init, L.fed_steps(steps[:4], [0.25, 0.25, 0.5, 0.5]), after, loss_scale_init=0.25, **kw)
    assert [s[1] for s in snaps][1::2] == [L.State(0.5, 0, 0, 1), L.State(0.5, 0, 0, 1)]


# ================================================================================================ the kernel alone
def scale_step_alone(partial, nblk, scale, skipped, put=lambda t: t.to(DEV), gscale=1.0, max_norm=R.MAX_NORM, cnt0=(1, 5, 7), count0=3):
    state = put(torch.tensor([scale, 1.0 / scale]))
    cnt = put(torch.tensor(cnt0, dtype=torch.int32))
    # after the tick: applied 4 + skipped 1 = attempt 5, flagged by the guard or not (its last flag was attempt 3)
    step = put(torch.tensor([4, 0, 5 if skipped else 3, 1], dtype=torch.int32))
    rec = put(torch.full((2,), float("nan")))
    clipped = put(torch.tensor([count0], dtype=torch.int32))
    ops.loss_scale_step(state, cnt, step, partial, nblk, gscale, max_norm, 2, 0.125, 8.0, rec, clipped)
    return dict(state=state, cnt=cnt, step=step, rec=rec, clipped=clipped)


@pytest.mark.parametrize("n", [None, 4, R.FLAT_SIZES[-1]])
def test_kernel_alone(n):
    """nblk = 0, 1 and 4096 (the block count of FLAT_SIZES' largest entry), integer gradients (their double sums are exact in any order):
    rec equals the reference, and at s = 1 tri_grad_clip_coef's record bit for bit."""
    if n is None:
        nblk, partial, sumsq = 0, None, 0.0
    else:
        g = R.integer_gradient(n, n)
        nblk = ops.grad_norm_blocks(n)
        assert nblk == (1 if n == 4 else 4096)
        partial = torch.full((nblk,), float("nan"), dtype=torch.float64, device=DEV)
        ops.grad_sumsq(g.to(DEV), partial)
        sumsq = float((g.double() ** 2).sum())
    for scale in (1.0, 0.125, 8.0):
        for skipped in (False, True):
            out = {k: v.cpu() for k, v in scale_step_alone(partial, nblk, scale, skipped).items()}
            # (the partials hold the sum of squares of what was fed: the same integers stand for g * s here)
            want = L.rec_fp32(sumsq, scale, max_norm=R.MAX_NORM, nblk=nblk)
            assert np.array_equal(out["rec"].numpy(), np.array(want, dtype=np.float32)), (scale, out["rec"].tolist(), want)
            c = float(want[1]) * scale
            assert out["clipped"].item() == 3 + (c < 1.0)
            after = L.scale_step(L.State(scale, 1, 5, 7), skipped, 2, 0.125, 8.0)
            assert out["state"].tolist() == [after.scale, 1.0 / after.scale] and out["cnt"].tolist() == list(after[1:])
            assert out["step"].tolist() == [4, 0, 5 if skipped else 3, 1]
    rec = torch.full((2,), float("nan"), device=DEV)
    cnt = torch.tensor([3], dtype=torch.int32, device=DEV)
    ops.grad_clip_coef(partial if nblk else torch.zeros(1, dtype=torch.float64, device=DEV), nblk, 1.0, R.MAX_NORM, rec, cnt)
    mine = scale_step_alone(partial, nblk, 1.0, False)
    assert same_bytes(mine["rec"], rec) and mine["clipped"].item() == cnt.item()


def test_the_entry_point_stays_inside_its_operands():
    """state, cnt, step, the exact-size partial buffer, rec and clipped between poisoned margins (tests/guard_bands.py), under 0xFF and 0x00
    bands: no band touched, the same bits both times, step unchanged, results as the reference has them."""
    from tests.test_gpu_guard_bands import twice
    n = R.FLAT_SIZES[3]
    g_host = R.integer_gradient(n, n)
    nblk = ops.grad_norm_blocks(n)

    def body(g):
        partial = g.put(torch.zeros(nblk, dtype=torch.float64))
        ops.grad_sumsq(g.put(g_host), partial)
        out = {f"{k}_clip": v for k, v in scale_step_alone(partial, nblk, 0.25, True, put=g.put).items()}
        out.update({f"{k}_none": v for k, v in scale_step_alone(None, 0, 0.25, False, put=g.put, max_norm=math.inf).items()})
        assert "tri_loss_scale_step" in g.lib.calls
        return out

    got = twice(body)
    want = L.rec_fp32(float((g_host.double() ** 2).sum()), 0.25, max_norm=R.MAX_NORM)
    assert np.array_equal(got["rec_clip"].numpy(), np.array(want, dtype=np.float32))
    assert got["state_clip"].tolist() == [0.125, 8.0] and got["cnt_clip"].tolist() == [0, 6, 7] and got["clipped_clip"].item() == 4
    assert got["rec_none"].tolist() == [0.0, 4.0] and got["state_none"].tolist() == [0.5, 2.0] and got["cnt_none"].tolist() == [0, 5, 8]
    assert got["clipped_none"].item() == 3 and got["step_clip"].tolist() == [4, 0, 5, 1] and got["step_none"].tolist() == [4, 0, 3, 1]


# ================================================================================================ captured step
@pytest.mark.parametrize("path", ["packed", "segments"])
def test_a_captured_step_backs_off_and_recovers_while_it_replays(path):
    """zero_grad, the backward of a tiny linear loss seeded with backward_seed(), and step() in ONE captured graph.  An inf in the static
    input before replays 3, 6 and 7 makes those steps overflow: the scale follows the reference, and the gradient of the replay after a
    back-off is half as large, bit for bit.
    "packed": the packed-gradient update path - everything is issued on the capture stream, no side stream, so the graph is a single chain
    BY CONSTRUCTION (nothing here inspects the captured graph's nodes; torch offers no count of its branches).
    "segments": the path train.fit and bench.py capture - the gradient-pointer table's copy is issued on a side stream that forks at
    zero_grad() and joins ahead of the guard, so this graph has one parallel branch; the scale step sits on the main chain after the join."""
    from tricolo_amd.optim import FusedAdam
    torch.manual_seed(11)
    lin = torch.nn.Linear(16, 8).to(DEV)
    x = torch.randn(4, 16, device=DEV)
    clean = x.clone()
    opt = FusedAdam(lin.parameters(), lr=1e-3, loss_scale="dynamic", loss_scale_init=1.0, loss_scale_growth_interval=3, loss_scale_min=0.125,
                    loss_scale_max=4.0)
    opt.prepare()
    seed = opt.backward_seed()
    assert seed.dim() == 0 and seed.data_ptr() == opt._ls_state.data_ptr()

    def one_step():
        opt.zero_grad(set_to_none=True)
        lin(x).sum().backward(gradient=opt.backward_seed())
        opt.step(**(dict(reduce_fn=lambda flat: None) if path == "packed" else {}))

    one_step()                                                       # eager warm-up: step 0 of the schedule
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        one_step()
    bad = (3, 6, 7)
    n = 10
    # [after the warm-up, after replay 0, ...]: replay t is seeded with states[t].scale - 1 1 2 2 | 1 1 1 | .5 | .25 .25
    states = L.schedule([False] + [t in bad for t in range(n)], 1.0, 3, 0.125, 4.0)[1:]
    assert [st.scale for st in states[:n]] == [1, 1, 2, 2, 1, 1, 1, 0.5, 0.25, 0.25]
    grads = []
    for t in range(n):
        x.copy_(clean)
        if t in bad:
            x[1, 3] = float("inf")
        graph.replay()
        torch.cuda.synchronize()
        assert scale_state(opt) == states[t + 1], (t, scale_state(opt), states[t + 1])
        grads.append(lin.weight.grad.detach().clone())
        if t not in bad:                                             # the same kernels on the same input: the seed's power of two, exactly
            assert same_bytes(grads[t], grads[0] * states[t].scale), t
    # d sum(x W^T + b) / d W[j] = the seed times the column sums of x (the kernel may add the four rows in another order)
    assert torch.allclose(grads[0][0], clean.sum(0), rtol=1e-5, atol=1e-6) and bool(grads[0].abs().sum() > 0)
    # replay 2 ran at scale 2, replay 3 overflowed at it, replay 4 runs at 1: half as large, bit for bit
    assert same_bytes(grads[4], 0.5 * grads[2]) and not bool(torch.isfinite(grads[3]).all())
    assert opt.skipped_steps() == 3 and opt.scale_backoffs() == 3 and int(opt._step_dev[0].item()) == n + 1 - 3
    assert all(bool(torch.isfinite(p).all()) for p in lin.parameters())


def test_first_use_inside_a_capture_raises():
    from tricolo_amd.optim import FusedAdam
    w = [torch.nn.Parameter(torch.zeros(8, device=DEV))]
    w[0].grad = torch.zeros(8, device=DEV)
    opt = FusedAdam(w, loss_scale="dynamic")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    raised = False
    with torch.cuda.graph(graph):
        try:
            opt.backward_seed()                                      # neither prepare() nor an eager backward_seed() came first
        except RuntimeError as e:
            raised = "capture" in str(e)
        w[0].grad.zero_()
    assert raised and opt._ls_state is None
    assert opt.backward_seed().item() == 1.0                         # eager: allocates


# ================================================================================================ checkpoint
def test_state_dict_round_trip(case):
    init, _, fed, states = case
    opt, w = drive("segments", init, fed[:6], **SCHEDULE)
    sd = opt.state_dict()
    assert sd["loss_scale"] == dict(zip(("scale", "streak", "backoffs", "growths"), states[6])) and states[6] == L.State(1.0, 1, 1, 1)
    fresh, w2 = make_opt("segments", init, **SCHEDULE)
    fresh.load_state_dict(sd)
    assert scale_state(fresh) == states[6] and float(fresh._ls_state[1].item()) == 1.0 / states[6].scale
    # ... and, given the parameters too, goes on as the first one does
    with torch.no_grad():
        for a, b in zip(w2, w):
            a.copy_(b)
    for o, ws in ((opt, w), (fresh, w2)):
        for p, g in zip(ws, fed[6]):
            p.grad = g.to(DEV)
        o.step()
    assert scale_state(opt) == scale_state(fresh) == states[7]
    assert all(same_bytes(a.detach(), b.detach()) for a, b in zip(w, w2))
    # torch.optim.Adam loads the same dict (it ignores the extra top-level key)
    adam = torch.optim.Adam([torch.nn.Parameter(t.clone().to(DEV)) for t in init], lr=R.LR)
    adam.load_state_dict(sd)
    first = adam.state[adam.param_groups[0]["params"][0]]
    assert int(first["step"]) == 5 and torch.equal(first["exp_avg"], sd["state"][0]["exp_avg"])
    # a dict without the key keeps the constructor's values
    plain_sd = {k: v for k, v in sd.items() if k != "loss_scale"}
    other, _ = make_opt("segments", init, **dict(SCHEDULE, loss_scale_init=2.0))
    other.load_state_dict(plain_sd)
    assert scale_state(other) == L.State(2.0, 0, 0, 0)
    # a dict from a run with a wider range and a longer interval is brought inside this optimizer's: the kernel assumes min <= s <= max
    for scale, want in ((64.0, L.MAX_SCALE), (2.0 ** -10, L.MIN_SCALE)):
        other.load_state_dict(dict(plain_sd, loss_scale={"scale": scale, "streak": 1500, "backoffs": 4, "growths": 9}))
        assert scale_state(other) == L.State(want, L.GROWTH_INTERVAL - 1, 4, 9) and float(other._ls_state[1].item()) == 1.0 / want
    with pytest.raises(ValueError, match="power of two"):
        other.load_state_dict(dict(plain_sd, loss_scale={"scale": 3.0, "streak": 0, "backoffs": 0, "growths": 0}))


# ================================================================================================ end to end, f16, real towers
def tower_fit(overrides, steps_per_epoch=20, epochs=2):
    from oracle.recipe import fill_module
    from tricolo_amd import config as tcfg
    from tricolo_amd.data import synthetic as syn
    from tricolo_amd.model.tricolo_net import TriCoLoNet
    from tricolo_amd.train import fit
    cfg = tcfg.compose(overrides=["model.text_encoder=BiGRUEncoder", "model.image_encoder=null", "model.voxel_encoder=SparseCNNEncoder",
                                  "data=synthetic", "data.voxel_size=32", "experiment_name=test", f"trainer.max_epochs={epochs}"] + overrides)
    net = TriCoLoNet(cfg)
    fill_module(net)
    made, configure = [], net.configure_optimizers
    net.configure_optimizers = lambda: made.append(configure()) or made[-1]      # keep the optimizer fit() makes: its device counters are read below
    batches = [syn.batch_to_device(syn.make_batch(4, voxel_size=32, num_views=None, seed=syn.BASE_SEED + 700 + i), DEV) for i in range(4)]
    lines = []
    out = fit(net, cfg, lambda epoch: [batches[(epoch + i) % 4] for i in range(steps_per_epoch)], device=DEV, log=lines.append)
    net.opt = made[-1]
    return net, out, lines


@pytest.fixture()
def f16():
    before = ops.default_precision()
    ops.set_default_precision("f16")
    yield
    ops.set_default_precision(before)


def test_fit_in_f16_backs_off_from_a_scale_that_overflows(f16):
    """Text + voxel at 32^3, batch 4, 40 steps from a scale of 2^20 on top of the static 2^12: structural assertions only."""
    net, out, lines = tower_fit(["+optimizer.loss_scale=dynamic", "+optimizer.loss_scale_init=1048576", "+optimizer.loss_scale_max=1048576",
                                 f"+optimizer.loss_scale_growth_interval={L.HUGE_INTERVAL}"])
    last = out["history"][-1]
    print(out["history"])
    applied = int(net.opt._step_dev[0].item())                       # the device's own count of applied steps (the t of the bias corrections)
    assert int(net.opt.state_dict()["state"][0]["step"]) == applied
    assert out["global_step"] == 40 and applied + last["skipped_steps"] == 40 and net.opt.skipped_steps() == last["skipped_steps"]
    assert last["skipped_steps"] == last["scale_backoffs"] == round(math.log2(1048576 / last["loss_scale"]))
    assert applied >= 1 and last["scale_growths"] == 0
    assert all(bool(torch.isfinite(p).all()) for p in net.parameters()) and math.isfinite(last["train_loss"])


def test_fit_in_f16_at_scale_one_keeps_the_bits_of_a_run_without_the_option(f16):
    """init = 1, the default ceiling of 1, no overflow: the seed is 1.0f and rec[1] = 1.0f, so every epoch loss equals, bit for bit, the run
    without the option."""
    _, on, _ = tower_fit(["+optimizer.loss_scale=dynamic", "+optimizer.loss_scale_init=1"])
    _, off, _ = tower_fit([])
    assert [r["train_loss"] for r in on["history"]] == [r["train_loss"] for r in off["history"]]
    assert on["history"][-1]["skipped_steps"] == 0 and on["history"][-1]["loss_scale"] == 1.0
    assert (on["history"][-1]["scale_backoffs"], on["history"][-1]["scale_growths"]) == (0, 0)
    assert not {"loss_scale", "scale_backoffs", "scale_growths"} & set(off["history"][-1])


# ================================================================================================ data-parallel paths
def test_data_parallel_paths(monkeypatch):
    """dp_training_step in a world of one (TRICOLO_FORCE_DIST=1) seeds its backward with the optimizer's scale; the two-stage backward and
    GraphedDPStep refuse the option by name."""
    import torch.distributed as dist
    from tests.test_gpu_modules import _build_net
    from tricolo_amd import parallel
    from tricolo_amd.data import synthetic as syn
    monkeypatch.setenv("TRICOLO_FORCE_DIST", "1")
    for k, v in dict(MASTER_ADDR="127.0.0.1", MASTER_PORT="29547", RANK="0", WORLD_SIZE="1").items():
        monkeypatch.setenv(k, v)
    dist.init_process_group("nccl", device_id=torch.device("cuda", 0))
    try:
        assert parallel.is_dist()
        batch = syn.batch_to_device(syn.make_batch(4, voxel_size=32, num_views=2, image_size=64, seed=syn.BASE_SEED + 31), DEV)
        nets = [_build_net("BiGRUEncoder", "MVCNNEncoder", "SparseCNNEncoder", 32, 2, 64)[0] for _ in range(2)]      # same recipe weights
        from tricolo_amd.optim import FusedAdam
        on = FusedAdam(nets[0].parameters(), lr=1e-4, loss_scale="dynamic", loss_scale_init=0.5, loss_scale_growth_interval=L.HUGE_INTERVAL)
        off = FusedAdam(nets[1].parameters(), lr=1e-4)
        handed = []
        seed_of = on.backward_seed
        monkeypatch.setattr(on, "backward_seed", lambda: handed.append(seed_of()) or handed[-1])
        loss_on = parallel.dp_training_step(nets[0], batch, on)["train_loss/total_loss"]
        loss_off = parallel.dp_training_step(nets[1], batch, off)["train_loss/total_loss"]
        torch.cuda.synchronize()
        assert len(handed) == 1 and handed[0].data_ptr() == on._ls_state.data_ptr()
        # the gradients carry the scale.  The backward is linear in the seed and a factor of 0.5 commutes with every rounding, so the two
        # runs differ only where two launches of the same kernel may add in another order: fp32 sums of a few thousand terms, 2^-24 each
        # - 1e-5 of the largest gradient covers that with room, and a seed of 1 (twice as large everywhere) is five orders beyond it
        g_on, g_off = on.flat_grad(), off.flat_grad()
        top = float(g_off.abs().max())
        d = float((g_on - 0.5 * g_off).abs().max())
        print(f"loss {loss_on.item()!r} / {loss_off.item()!r}; max |g_on - g_off / 2| = {d:.3e}, max |g_off| = {top:.3e}")
        assert abs(loss_on.item() - loss_off.item()) <= 1e-5 * abs(loss_off.item())
        assert top > 0 and d <= 1e-5 * top
        assert scale_state(on) == L.State(0.5, 1, 0, 0) and on.skipped_steps() == 0
        split = parallel.BackwardSplit.for_net(nets[0])
        with pytest.raises(RuntimeError, match="loss_scale='dynamic'"):
            parallel.dp_training_step(nets[0], batch, on, split=split)
        with pytest.raises(RuntimeError, match="loss_scale='dynamic'"):
            parallel.GraphedDPStep(nets[0], on, batch)
    finally:
        dist.destroy_process_group()
