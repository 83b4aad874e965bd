"""GPU: NT-Xent with a learnable temperature - the four tri_ntxent_*_ls_* entry points against the float64 restatement
(tests/ntxent_temperature_reference.py), the clamp, reproducibility, the untouched fixed path, HIP-graph replay that follows the
parameter, the module inside a FusedAdam step with its checkpoint round trip, rejections, guard bands and a two-rank run.

Tolerances.  Loss and dz: hr.NTX_LOSS_TOL / hr.NTX_GRAD_ATOL at logit_scale = ln(10) (T = 0.1), per pair and at upstream 1 as everywhere
else; the gradient is linear in the upstreams, so with per-pair upstreams u_q a modality's bound is NTX_GRAD_ATOL * max(1, max |u_q| over
its pairs).  d loss / d logit_scale: DLS_BOUND, relative to the gradient's mass sum_q |u_q| sum_ij |G_ij S_ij| (the size of the terms that
are summed; the sum itself cancels to a fraction of it) - four times the largest error of a plain fp32 torch-autograd evaluation on the CPU
over these same cases, measured in profiles/r26/NOTES_learnable_temperature.md (`python -m tests.ntxent_temperature_reference` prints
the table)."""
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import grad_clip_reference as R
from tests import head_reference as hr
from tests import ntxent_temperature_reference as tr

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tricolo_amd import _C, ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
ALPHA, MAXLS, LS10 = hr.ALPHA, tr.MAX_LOGIT_SCALE, tr.LS_T01
# profiles/r26/NOTES_learnable_temperature.md: the largest fp32 CPU error is 5.956e-7 of the mass ((16, 2048) at ln 10); 4 x that
DLS_BOUND = 2.38e-6
_REF = {}


def scalar(v):
    return torch.tensor(float(v), dtype=torch.float32, device=DEV)


def inputs(B, D, M=2, norm=True):
    zs = hr.ntx_inputs(B, D, M=M)
    return zs if norm else [hr.normalise_rows_f64_to_f32(z) for z in zs]


def reference(B, D, M, ls, norm=True, dpairs=None):
    """float64 (losses, total, dzs, dlogit_scale, mass), computed once per case and left unchanged."""
    key = (B, D, M, float(ls), norm, None if dpairs is None else tuple(dpairs))
    if key not in _REF:
        zs = inputs(B, D, M, norm)
        out = tr.nt_xent_ls_all_pairs_f64(zs, ls, norm=norm, dpairs=dpairs)
        _REF[key] = out + (tr.dls_mass(zs, ls, norm=norm, dpairs=dpairs),)
    return _REF[key]


def check_dls(case, got, ref, mass):
    err = abs(float(got) - ref)
    print(f"{case}: dlogit_scale {float(got):+.7e} float64 {ref:+.7e} |err| {err:.3e} = {err / mass if mass else 0.0:.3e} of the mass {mass:.4e} "
          f"(bound {DLS_BOUND:.2e})")
    assert err <= DLS_BOUND * mass, (case, err, mass)


def run_pair(B, D, ls, norm=True):
    za, zb = (z.to(DEV) for z in inputs(B, D, 2, norm))
    return ops.ntxent_fwd_bwd(za, zb, None, ALPHA, norm, logit_scale=scalar(ls), max_logit_scale=MAXLS)


def check_pair(case, out, ref):
    loss, dza, dzb, dls = out
    (l64,), _, (da, db), d64, mass = ref
    le = abs(float(loss) - l64)
    ge = max(float(np.abs(dza.cpu().numpy() - da).max()), float(np.abs(dzb.cpu().numpy() - db).max()))
    print(f"{case}: loss err {le:.3e} grad err {ge:.3e}")
    assert le < hr.NTX_LOSS_TOL and ge <= hr.NTX_GRAD_ATOL, (case, le, ge)
    check_dls(case, dls, d64, mass)


# ================================================================================================ against float64
@pytest.mark.parametrize("B,D", tr.ROW_CASES)
def test_single_pair_row_kernel(B, D):
    """ntxm_sim_rows_kernel: B not a multiple of 4 or 16, D past one 256-lane pass, B past one 256-thread pass of the lse and coefficient loops;
    the split call (forward, then the gradient half with an upstream of 1) gives the same bits as the fused one."""
    out = run_pair(B, D, LS10)
    check_pair(f"pair_rows_{B}x{D}", out, reference(B, D, 2, LS10))
    za, zb = (z.to(DEV) for z in inputs(B, D))
    ls = scalar(LS10)
    loss, ws = ops.ntxent_fwd(za, zb, None, ALPHA, logit_scale=ls)
    dza, dzb, dls = ops.ntxent_bwd(za, zb, ws, None, ALPHA, dloss=scalar(1.0), logit_scale=ls)
    for a, b in zip(out, (loss, dza, dzb, dls)):
        assert torch.equal(a, b)
    if B == 1:
        assert float(out[3]) == 0.0 and float(out[0]) == 0.0


@pytest.mark.parametrize("B,D,norm", [(70, 18, True), (513, 8, True), (70, 18, False)])
def test_single_pair_tiled_similarity_kernel(B, D, norm):
    """ntx_sim_kernel (B > 512 or D % 4 != 0), which took 1 / T as a kernel argument."""
    check_pair(f"pair_tiled_{B}x{D}_norm{int(norm)}", run_pair(B, D, LS10, norm), reference(B, D, 2, LS10, norm))


def run_multi(B, D, M, ls, dpairs=None):
    zd = [z.to(DEV) for z in inputs(B, D, M)]
    lsd = scalar(ls)
    losses, ws = ops.ntxent_multi_fwd(zd, None, ALPHA, logit_scale=lsd, max_logit_scale=MAXLS)
    dp = None if dpairs is None else [scalar(v) for v in dpairs]
    out = ops.ntxent_multi_bwd(zd, ws, None, ALPHA, dpairs=dp, dtotal=scalar(1.0), logit_scale=lsd, max_logit_scale=MAXLS)
    return losses, out[:-1], out[-1]


@pytest.mark.parametrize("with_pairs", [False, True], ids=["dtotal", "dtotal_dpairs"])
@pytest.mark.parametrize("B,D", tr.MULTI_CASES)
@pytest.mark.parametrize("M", [2, 3])
def test_all_pairs(M, B, D, with_pairs):
    P = M * (M - 1) // 2
    dpairs = list(tr.PAIR_UPSTREAMS[:P]) if with_pairs else None
    losses, dzs, dls = run_multi(B, D, M, LS10, dpairs)
    l64, t64, dz64, d64, mass = reference(B, D, M, LS10, dpairs=dpairs)
    losses = losses.cpu().numpy().astype(np.float64)
    case = f"multi_M{M}_{B}x{D}_{'pairs' if with_pairs else 'total'}"
    print(f"{case}: loss err {np.abs(losses[:P] - l64).max():.3e} total err {abs(losses[P] - t64):.3e}")
    assert np.abs(losses[:P] - l64).max() < hr.NTX_LOSS_TOL and abs(losses[P] - t64) < P * hr.NTX_LOSS_TOL
    from itertools import combinations
    for m in range(M):
        ups = [1.0 + (dpairs[q] if dpairs else 0.0) for q, pr in enumerate(combinations(range(M), 2)) if m in pr]
        atol = hr.NTX_GRAD_ATOL * max(1.0, max(abs(u) for u in ups))
        ge = float(np.abs(dzs[m].cpu().numpy() - dz64[m]).max())
        print(f"{case}: dz[{m}] err {ge:.3e} (atol {atol:.1e})")
        assert ge <= atol
    check_dls(case, dls, d64, mass)


# ================================================================================================ clamp
@pytest.mark.parametrize("outside,edge", [(MAXLS + 1.0, MAXLS), (-0.5, 0.0)], ids=["above", "below"])
def test_clamp_stops_the_gradient_outside_and_passes_it_at_the_boundaries(outside, edge):
    B, D = 37, 260
    out_o, out_e = run_pair(B, D, outside), run_pair(B, D, edge)
    assert float(out_o[3]) == 0.0 and out_o[3].cpu().view(torch.int32).item() == 0          # +0.0f exactly
    for a, b in zip(out_o[:3], out_e[:3]):                       # loss, dza, dzb: the run AT the boundary, bit for bit
        assert torch.equal(a, b)
    (l64,), _, (da, db), d64, mass = reference(B, D, 2, edge)
    assert float(out_e[3]) != 0.0 and d64 != 0.0
    check_dls(f"pair_edge_{edge:.3f}", out_e[3], d64, mass)
    # the all-pairs form gates the same way
    _, dzs_o, dls_o = run_multi(B, D, 3, outside)
    _, dzs_e, dls_e = run_multi(B, D, 3, edge)
    assert float(dls_o) == 0.0 and float(dls_e) != 0.0 and all(torch.equal(a, b) for a, b in zip(dzs_o, dzs_e))
    _, _, _, d64m, massm = reference(B, D, 3, edge)
    check_dls(f"multi_edge_{edge:.3f}", dls_e, d64m, massm)


def test_batch_of_one_gives_exactly_zero():
    for ls in (LS10, 0.0, MAXLS):
        loss, dza, dzb, dls = run_pair(1, 4, ls)
        assert float(dls) == 0.0 and float(loss) == 0.0 and not dza.any() and not dzb.any()
    _, _, dls = run_multi(1, 4, 3, LS10, list(tr.PAIR_UPSTREAMS))
    assert float(dls) == 0.0


def test_backward_is_bit_reproducible():
    a, b = run_multi(300, 64, 3, LS10, list(tr.PAIR_UPSTREAMS)), run_multi(300, 64, 3, LS10, list(tr.PAIR_UPSTREAMS))
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))


# ================================================================================================ fixed path
def test_fixed_temperature_path_keeps_its_bits(golden):
    """ops.ntxent_multi_fwd / _bwd WITHOUT logit_scale at (37, 260), M = 3: the bits recorded from the commit before the kernels learnt to
    read the scale from the device (tests/golden/ntxent_fixed_37x260_m3.npz; upstream 1 on the total, then also 0.5 / -1.25 / 2 per pair)."""
    g = golden("ntxent_fixed_37x260_m3")
    zd = [z.to(DEV) for z in hr.ntx_inputs(37, 260, M=3)]
    losses, ws = ops.ntxent_multi_fwd(zd, hr.T, ALPHA)
    one = scalar(1.0)
    dz_total = ops.ntxent_multi_bwd(zd, ws, hr.T, ALPHA, dtotal=one)
    dz_pairs = ops.ntxent_multi_bwd(zd, ws, hr.T, ALPHA, dpairs=[scalar(v) for v in tr.PAIR_UPSTREAMS], dtotal=one)
    assert len(dz_total) == 3 and len(dz_pairs) == 3              # no trailing dlogit_scale
    assert np.array_equal(losses.cpu().numpy().view(np.int32), g["losses"].view(np.int32))
    for m in range(3):
        assert np.array_equal(dz_total[m].cpu().numpy().view(np.int32), g[f"dz_total_{m}"].view(np.int32)), m
        assert np.array_equal(dz_pairs[m].cpu().numpy().view(np.int32), g[f"dz_pairs_{m}"].view(np.int32)), m
    assert ws.numel() == ops.lib().tri_ntxent_multi_workspace(3, 37, 260)


# ================================================================================================ replay
def test_captured_step_follows_the_parameter():
    """Forward and backward of the M = 3 all-pairs loss captured ONCE; logit_scale changed in place; replayed: the outputs are those of an
    eager call at the new value, bit for bit, and differ from the first replay.  (A scale passed by value would freeze in the graph.)"""
    zd = [z.to(DEV) for z in hr.ntx_inputs(37, 260, M=3)]
    ls, one = scalar(LS10), scalar(1.0)
    dp = [scalar(v) for v in tr.PAIR_UPSTREAMS]

    def call():
        losses, ws = ops.ntxent_multi_fwd(zd, None, ALPHA, logit_scale=ls)
        return [losses] + ops.ntxent_multi_bwd(zd, ws, None, ALPHA, dpairs=dp, dtotal=one, logit_scale=ls)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = call()
    graph.replay()
    torch.cuda.synchronize()
    first = [t.clone() for t in static]
    for a, b in zip(first, call()):
        assert torch.equal(a, b)
    ls.fill_(3.25)
    graph.replay()
    torch.cuda.synchronize()
    second = [t.clone() for t in static]
    eager = call()
    for a, b in zip(second, eager):
        assert torch.equal(a, b)
    assert all(not torch.equal(a, b) for a, b in zip(first, second))


# ================================================================================================ module and step
BASE = ["data=synthetic", "model.text_encoder=BiGRUEncoder", "model.image_encoder=MVCNNEncoder", "model.voxel_encoder=SparseCNNEncoder",
        "data.voxel_size=32", "data.num_views=2", "data.image_size=64", "experiment_name=learnable_temperature"]
OVERRIDE = ["+loss.NTXentLoss.learnable_temperature=true"]


def build_net(overrides):
    from oracle.recipe import fill_module
    from tricolo_amd import config as tcfg
    from tricolo_amd.model.tricolo_net import TriCoLoNet
    cfg = tcfg.compose(overrides=BASE + overrides)
    net = TriCoLoNet(cfg)
    for tower in ("text_encoder", "image_encoder", "voxel_encoder"):           # the recipe's values under the net's own keys; logit_scale keeps
        fill_module(getattr(net, tower), prefix=tower + ".")                   # its initial ln(1 / temperature) (the recipe has no 0-d rule)
    return net.to(DEV), cfg


def make_batch(B, seed_off=11):
    from tricolo_amd.data import synthetic as syn
    return syn.make_batch(B, voxel_size=32, num_views=2, image_size=64, seed=syn.BASE_SEED + seed_off)


def test_module_trains_the_temperature_with_fused_adam_and_round_trips(tmp_path):
    """Three FusedAdam steps of TriCoLoNet at batch 8 with the override: logit_scale moves; its p, m, v follow a float64 Adam loop driven by the
    restated gradient of each step's own embeddings (tolerance of tests/test_gpu_grad_clip.py for that comparison, R.ATOL); the state dict has
    `loss_fn.logit_scale`, last; a checkpoint round trip restores the parameter and its optimizer state bit for bit."""
    from tricolo_amd.checkpoint import extract_state_dict, save_reference_checkpoint
    from tricolo_amd.data import synthetic as syn
    from tricolo_amd.optim import FusedAdam
    before = ops.default_precision()
    ops.set_default_precision("bf16x3")
    try:
        fixed_keys = list(build_net([])[0].state_dict())
        net, cfg = build_net(OVERRIDE)
        assert list(net.state_dict()) == fixed_keys + ["loss_fn.logit_scale"]
        assert [n for n, _ in net.named_parameters()][-1] == "loss_fn.logit_scale"
        opt = net.configure_optimizers()
        assert isinstance(opt, FusedAdam)
        batch = syn.batch_to_device(make_batch(8), DEV)
        p = net.loss_fn.logit_scale
        p0 = float(p.detach())
        assert p0 == float(np.float32(math.log(10.0)))
        p64, grads = p0, []
        for step in range(3):
            opt.zero_grad(set_to_none=True)
            out = net(batch)
            losses = net._calculate_losses(out, "train_loss")
            torch.cuda.synchronize()
            zs = [v.detach().cpu() for v in out.values()]
            ls_now = float(p.detach())
            _, t64, _, d64 = tr.nt_xent_ls_all_pairs_f64(zs, ls_now)
            assert abs(float(losses["train_loss/total_loss"].detach()) - t64) < 3 * hr.NTX_LOSS_TOL
            losses["train_loss/total_loss"].backward()
            check_dls(f"step{step}", p.grad, d64, tr.dls_mass(zs, ls_now))
            grads.append(d64)
            opt.step()
        torch.cuda.synchronize()
        assert float(p.detach()) != p0
        rp, rm, rv = tr.adam_f64(p0, grads, float(cfg.optimizer.lr), weight_decay=float(cfg.optimizer.weight_decay))
        st = opt.state[p]
        got = (float(p.detach()), float(st["exp_avg"]), float(st["exp_avg_sq"]))
        print(f"logit_scale {p0:.7f} -> {got[0]:.7f}; |p - f64| {abs(got[0] - rp):.3e} |m - f64| {abs(got[1] - rm):.3e} |v - f64| {abs(got[2] - rv):.3e} "
              f"(tolerance {R.ATOL:.3e})")
        assert abs(got[0] - rp) <= R.ATOL and abs(got[1] - rm) <= R.ATOL and abs(got[2] - rv) <= R.ATOL
        assert abs(net.loss_fn.current_temperature() - math.exp(-got[0])) < 1e-7
        # checkpoint round trip: parameter and optimizer state, bit for bit, into a fresh learnable net + optimizer
        path = str(tmp_path / "lt.ckpt")
        save_reference_checkpoint(net, path, epoch=0, global_step=3, optimizer=opt)
        doc = torch.load(path, map_location="cpu", weights_only=False)
        assert "loss_fn.logit_scale" in doc["state_dict"] and doc["state_dict"]["loss_fn.logit_scale"].dim() == 0
        net2, _ = build_net(OVERRIDE)
        net2.load_state_dict(extract_state_dict(doc), strict=True)
        opt2 = net2.configure_optimizers()
        opt2.load_state_dict(doc["optimizer_states"][0])
        p2 = net2.loss_fn.logit_scale
        assert torch.equal(p2.detach(), p.detach())
        st2 = opt2.state[p2]
        assert torch.equal(st2["exp_avg"], st["exp_avg"]) and torch.equal(st2["exp_avg_sq"], st["exp_avg_sq"])
        assert int(opt2._step_dev[0].item()) == 3
    finally:
        ops.set_default_precision(before)


def test_fit_logs_the_temperature_once_per_epoch_and_resumes_a_fixed_checkpoint(tmp_path, capsys):
    """train.fit: `train_loss/temperature` in every epoch record of a learnable run and in none of a fixed one; a fixed-temperature
    checkpoint resumes into a learnable run from ln(1 / temperature) with one line saying so, the other parameters' optimizer state kept."""
    from tricolo_amd import config as tcfg, train
    from tricolo_amd.data import synthetic as syn
    before = ops.default_precision()
    ops.set_default_precision("bf16x3")
    try:
        batch = syn.batch_to_device(make_batch(8), DEV)
        batches = lambda epoch: [batch, batch]                  # noqa: E731
        net_f, _ = build_net([])
        cfg_f = tcfg.compose(overrides=BASE + ["trainer.max_epochs=1"])
        res_f = train.fit(net_f, cfg_f, batches, out_dir=str(tmp_path / "fixed"), log=lambda r: None)
        assert all("train_loss/temperature" not in r for r in res_f["history"])
        net_l, _ = build_net(OVERRIDE)
        cfg_l = tcfg.compose(overrides=BASE + OVERRIDE + ["trainer.max_epochs=2"])
        capsys.readouterr()
        res_l = train.fit(net_l, cfg_l, batches, ckpt_path=str(tmp_path / "fixed" / "last.ckpt"), log=lambda r: None)
        said = [l for l in capsys.readouterr().out.splitlines() if "loss_fn.logit_scale" in l]
        assert len(said) == 1 and "fixed temperature" in said[0]
        temps = [r["train_loss/temperature"] for r in res_l["history"]]
        assert len(temps) == 1 and res_l["history"][0]["epoch"] == 1 and res_l["history"][0]["global_step"] == 4
        assert temps[0] == net_l.loss_fn.current_temperature() and temps[0] != 0.1 and abs(temps[0] - 0.1) < 1e-3
    finally:
        ops.set_default_precision(before)


# ================================================================================================ rejections
def test_rejections():
    lib = ops.lib()
    B, D = 5, 8
    za, zb = (torch.randn(B, D, device=DEV) for _ in range(2))
    ls, loss, dls, one = scalar(LS10), scalar(0.0), scalar(0.0), scalar(1.0)
    dza, dzb = torch.empty_like(za), torch.empty_like(zb)
    n2 = lib.tri_ntxent_ls_workspace(2, B, D)
    ws = torch.empty(n2, dtype=torch.uint8, device=DEV)
    P_, st = _C.ptr, ops.stream()

    def pair(ls_=ls, dls_=dls, nbytes=n2, maxls=MAXLS):
        return lib.tri_ntxent_ls_fwd_bwd(P_(za), P_(zb), B, D, P_(ls_), maxls, ALPHA, 1, P_(loss), P_(dza), P_(dzb), P_(dls_), P_(ws), nbytes, st)

    def pair_bwd(ls_=ls, dls_=dls, nbytes=n2):
        return lib.tri_ntxent_ls_bwd(P_(za), P_(zb), B, D, P_(ls_), MAXLS, ALPHA, 1, None, P_(dza), P_(dzb), P_(dls_), P_(ws), nbytes, st)

    assert pair() == 0 and pair_bwd() == 0
    small = lib.tri_ntxent_workspace(B, D)                      # the fixed workspace is too small for the learnable calls
    assert small < n2
    for call, kw, what in ((pair, dict(ls_=None), "logit_scale is NULL"), (pair, dict(dls_=None), "dlogit_scale is NULL"),
                           (pair, dict(nbytes=small), "workspace too small"), (pair, dict(nbytes=n2 - 1), "workspace too small"),
                           (pair, dict(maxls=-1.0), "max_logit_scale"), (pair, dict(maxls=math.inf), "max_logit_scale"),
                           (pair, dict(maxls=math.nan), "max_logit_scale"), (pair_bwd, dict(ls_=None), "logit_scale is NULL"),
                           (pair_bwd, dict(dls_=None), "dlogit_scale is NULL"), (pair_bwd, dict(nbytes=small), "workspace too small")):
        rc = call(**kw)
        assert rc == _C.TRI_ERR_ARG, (kw, rc)
        with pytest.raises(RuntimeError, match=f"tri_ntxent.*{what}"):
            ops.check(rc, "tri_ntxent_ls")
    # a forward-only call needs no dlogit_scale
    assert lib.tri_ntxent_ls_fwd_bwd(P_(za), P_(zb), B, D, P_(ls), MAXLS, ALPHA, 1, P_(loss), None, None, None, P_(ws), n2, st) == 0
    # all pairs
    zs = [torch.randn(B, D, device=DEV) for _ in range(3)]
    arr = lambda ts: (_C.C.c_void_p * len(ts))(*[P_(t) for t in ts])             # noqa: E731
    n3 = lib.tri_ntxent_ls_workspace(3, B, D)
    ws3 = torch.empty(n3, dtype=torch.uint8, device=DEV)
    losses = torch.empty(4, device=DEV)
    dzs = [torch.empty_like(z) for z in zs]

    def mfwd(ls_=ls, nbytes=n3):
        return lib.tri_ntxent_multi_ls_fwd(arr(zs), 3, B, D, P_(ls_), MAXLS, ALPHA, 1, P_(losses), P_(ws3), nbytes, st)

    def mbwd(ls_=ls, dls_=dls, nbytes=n3):
        return lib.tri_ntxent_multi_ls_bwd(arr(zs), 3, B, D, P_(ls_), MAXLS, ALPHA, 1, None, P_(one), arr(dzs), P_(dls_), P_(ws3), nbytes, st)

    assert mfwd() == 0 and mbwd() == 0
    for call, kw in ((mfwd, dict(ls_=None)), (mfwd, dict(nbytes=lib.tri_ntxent_multi_workspace(3, B, D))), (mbwd, dict(ls_=None)),
                     (mbwd, dict(dls_=None)), (mbwd, dict(nbytes=n3 - 1))):
        rc = call(**kw)
        assert rc == _C.TRI_ERR_ARG, (kw, rc)
        with pytest.raises(RuntimeError, match="tri_ntxent"):
            ops.check(rc, "tri_ntxent_multi_ls")
    torch.cuda.synchronize()
    # the multi range limits, through ops: B <= 512, 4 <= D <= 2048, D % 4 == 0
    for Bm, Dm in ((513, 8), (8, 2052), (8, 6), (8, 2)):
        with pytest.raises(RuntimeError, match="tri_ntxent"):
            ops.ntxent_multi_fwd([torch.zeros(Bm, Dm, device=DEV) for _ in range(2)], None, ALPHA, logit_scale=ls)
    with pytest.raises(RuntimeError, match="tri_ntxent"):      # single pair: D <= 2048
        ops.ntxent_fwd(torch.zeros(4, 2049, device=DEV), torch.zeros(4, 2049, device=DEV), None, ALPHA, logit_scale=ls)
    with pytest.raises(RuntimeError, match="logit_scale"):     # a host scalar is refused before any launch
        ops.ntxent_fwd(za, zb, None, ALPHA, logit_scale=torch.tensor(1.0))


# ================================================================================================ guard bands
@pytest.mark.parametrize("B,D,M", [(37, 260, 3), (70, 18, 2)])
def test_new_calls_under_guard_bands(B, D, M):
    """The four new calls between poisoned and zeroed margins (tests/guard_bands.py), their workspace of EXACTLY tri_ntxent_ls_workspace
    bytes banded too: nothing outside the operands is read into a result or written."""
    from tests.guard_bands import recording  # noqa: F401  (the harness this relies on)
    from tests.test_gpu_guard_bands import twice
    zs = inputs(B, D, M)
    launched = set()

    def body(g):
        zd = [g.put(z) for z in zs]
        ls = g.put(torch.tensor(LS10, dtype=torch.float32))
        out = {}
        loss, dza, dzb, dls = ops.ntxent_fwd_bwd(zd[0], zd[1], None, ALPHA, logit_scale=ls)
        out.update(loss=loss, dza=dza, dzb=dzb, dls=dls)
        l2, ws = ops.ntxent_fwd(zd[0], zd[1], None, ALPHA, logit_scale=ls)
        assert ws.numel() == ops.lib().tri_ntxent_ls_workspace(2, B, D)
        dza2, dzb2, dls2 = ops.ntxent_bwd(zd[0], zd[1], ws, None, ALPHA, dloss=g.put(torch.ones(())), logit_scale=ls)
        out.update(l2=l2, dza2=dza2, dzb2=dzb2, dls2=dls2)
        if ops.ntxent_multi_supported(B, D, M):
            losses, wsm = ops.ntxent_multi_fwd(zd, None, ALPHA, logit_scale=ls)
            assert wsm.numel() == ops.lib().tri_ntxent_ls_workspace(M, B, D)
            res = ops.ntxent_multi_bwd(zd, wsm, None, ALPHA, dtotal=g.put(torch.ones(())), logit_scale=ls)
            out.update(losses=losses, mdls=res[-1], **{f"mdz{i}": d for i, d in enumerate(res[:-1])})
        launched.update(g.launched)
        return out

    got = twice(body)
    want = {"tri_ntxent_ls_fwd_bwd", "tri_ntxent_ls_bwd"} | ({"tri_ntxent_multi_ls_fwd", "tri_ntxent_multi_ls_bwd"} if M == 3 else set())
    assert want <= launched
    (l64,), _, (da, db), d64, mass = reference(B, D, 2, LS10)
    for k in ("", "2"):
        assert abs(float(got["loss" if not k else "l2"]) - l64) < hr.NTX_LOSS_TOL
        np.testing.assert_allclose(got[f"dza{k}"].numpy(), da, rtol=0, atol=hr.NTX_GRAD_ATOL)
        np.testing.assert_allclose(got[f"dzb{k}"].numpy(), db, rtol=0, atol=hr.NTX_GRAD_ATOL)
        check_dls(f"guarded_pair{k}_{B}x{D}", got[f"dls{k}"], d64, mass)
    if M == 3:
        l64m, t64, dz64, d64m, massm = reference(B, D, 3, LS10)
        assert abs(float(got["losses"][3]) - t64) < 3 * hr.NTX_LOSS_TOL
        for m in range(3):
            np.testing.assert_allclose(got[f"mdz{m}"].numpy(), dz64[m], rtol=0, atol=hr.NTX_GRAD_ATOL)
        check_dls(f"guarded_multi_{B}x{D}", got["mdls"], d64m, massm)


# ================================================================================================ data-parallel
DP_STEPS = 2


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _shard(full, rank, per):
    sl = slice(per * rank, per * rank + per)
    keep = (full["voxels"]["locs"][:, 0] >= per * rank) & (full["voxels"]["locs"][:, 0] < per * rank + per)
    locs = full["voxels"]["locs"][keep].clone()
    locs[:, 0] -= per * rank
    return {"model_id": full["model_id"][sl], "category": full["category"][sl], "tokens": full["tokens"][sl],
            "images": full["images"][sl], "voxels": {"locs": locs, "feats": full["voxels"]["feats"][keep]}}


def _dp_worker(rank, world, port, out_dir):
    """One rank of the two-rank run (tests/test_gpu_dp.py's manner: both ranks share cuda:0 and exchange through gloo; BatchNorm uses the
    global batch's statistics, so the two ranks together are the single-process run over the concatenated batch)."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from tricolo_amd import ops, parallel
    from tricolo_amd.data import synthetic as syn
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ops.set_default_precision("bf16x3")
    ops.set_sync_bn(True)
    net, _ = build_net(OVERRIDE)
    opt = net.configure_optimizers()
    opt.prepare()
    shard = syn.batch_to_device(_shard(make_batch(8), rank, 4), DEV)
    for _ in range(DP_STEPS):
        parallel.dp_training_step(net, shard, opt)
    torch.cuda.synchronize()
    p = net.loss_fn.logit_scale
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), p=p.detach().cpu().numpy(), m=opt.state[p]["exp_avg"].cpu().numpy(),
             v=opt.state[p]["exp_avg_sq"].cpu().numpy())
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_keep_one_temperature(tmp_path):
    """Two steps on two ranks (4 samples each): both hold the same logit_scale bits, and the value is the single-process run's over the
    8 samples within the bound tests/test_gpu_dp.py puts on parameters (5e-3).  Every rank differentiates the SAME global loss, so the
    ranks' gradients must not simply add up (parallel.replicated): Adam's sign-like first steps would hide a doubled gradient in p, its
    first moment would not - it is held to 2e-2, that file's bound on a gradient norm."""
    port = _free_port()
    code = "import sys; from tests.test_gpu_ntxent_temperature import _dp_worker; _dp_worker(int(sys.argv[1]), 2, int(sys.argv[2]), sys.argv[3])"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    procs = [subprocess.Popen([sys.executable, "-c", code, str(r), str(port), str(tmp_path)], cwd=REPO, env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = []
    try:
        for pr in procs:                                        # each rank under its own time limit
            outs.append(pr.communicate(timeout=240)[0])
    finally:
        for pr in procs:
            if pr.poll() is None:
                pr.kill()
                pr.communicate()
    for r, (pr, out) in enumerate(zip(procs, outs)):
        assert pr.returncode == 0, f"rank {r} exited with {pr.returncode}:\n{out[-3000:]}"
    r0, r1 = (dict(np.load(tmp_path / f"rank{r}.npz")) for r in range(2))
    for k in ("p", "m", "v"):
        assert np.array_equal(r0[k].view(np.int32), r1[k].view(np.int32)), k
    # the single-process run over the concatenated batch
    from tricolo_amd.data import synthetic as syn
    before = ops.default_precision()
    ops.set_default_precision("bf16x3")
    try:
        net, _ = build_net(OVERRIDE)
        opt = net.configure_optimizers()
        batch = syn.batch_to_device(make_batch(8), DEV)
        for _ in range(DP_STEPS):
            opt.zero_grad(set_to_none=True)
            net.training_step(batch, 0).backward()
            opt.step()
        torch.cuda.synchronize()
        p = net.loss_fn.logit_scale
        sp, sm = float(p.detach()), float(opt.state[p]["exp_avg"])
    finally:
        ops.set_default_precision(before)
    print(f"logit_scale two ranks {float(r0['p']):.7f} single {sp:.7f}; exp_avg two ranks {float(r0['m']):+.6e} single {sm:+.6e}")
    assert float(r0["p"]) != float(np.float32(math.log(10.0)))
    assert abs(float(r0["p"]) - sp) < 5e-3
    assert abs(float(r0["m"]) - sm) <= 2e-2 * abs(sm)
