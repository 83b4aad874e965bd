"""CPU: the float64 restatement of NT-Xent with a learnable temperature (tests/ntxent_temperature_reference.py) against torch autograd
on the reference's formula with temperature = exp(-clamp(logit_scale)); the new C-ABI symbols; the module without the switch."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import head_reference as hr
from tests import ntxent_temperature_reference as tr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXLS = tr.MAX_LOGIT_SCALE
# inside, both inclusive boundaries, and both sides outside the clamp
SCALES = [tr.LS_T01, 0.0, MAXLS, MAXLS + 1.0, -0.5]


@pytest.mark.parametrize("ls", SCALES)
@pytest.mark.parametrize("B,D,norm", [(5, 4, True), (37, 260, True), (70, 18, False)])
def test_pair_restatement_matches_float64_autograd(B, D, norm, ls):
    za, zb = hr.ntx_inputs(B, D)
    if not norm:
        za, zb = hr.normalise_rows_f64_to_f32(za), hr.normalise_rows_f64_to_f32(zb)
    loss, da, db, dls = tr.nt_xent_ls_f64(za, zb, ls, norm=norm)
    tl, (ta, tb), tdls = tr.nt_xent_ls_torch([za, zb], ls, norm=norm)
    assert abs(loss - tl[0]) <= 1e-12 * max(1.0, abs(tl[0]))
    np.testing.assert_allclose(da, ta, rtol=0, atol=1e-12)
    np.testing.assert_allclose(db, tb, rtol=0, atol=1e-12)
    inside = 0.0 <= np.float32(ls) <= np.float32(MAXLS)
    if inside:
        assert dls != 0.0 and abs(dls - tdls) <= 1e-11 * max(1.0, abs(tdls))
    else:
        assert dls == 0.0 and tdls == 0.0
        # the clamped run IS the run at the boundary
        edge = MAXLS if ls > MAXLS else 0.0
        le, dae, dbe, _ = tr.nt_xent_ls_f64(za, zb, edge, norm=norm)
        assert le == loss and np.array_equal(dae, da) and np.array_equal(dbe, db)


@pytest.mark.parametrize("M", [2, 3])
@pytest.mark.parametrize("ls", [tr.LS_T01, MAXLS, -0.5])
def test_all_pairs_restatement_matches_float64_autograd(M, ls):
    zs = hr.ntx_inputs(37, 260, M=M)
    P = M * (M - 1) // 2
    for dpairs, dtotal in ((None, 1.0), (list(tr.PAIR_UPSTREAMS[:P]), 1.0), (list(tr.PAIR_UPSTREAMS[:P]), 0.75)):
        losses, total, dzs, dls = tr.nt_xent_ls_all_pairs_f64(zs, ls, dpairs=dpairs, dtotal=dtotal)
        tl, tdz, tdls = tr.nt_xent_ls_torch(zs, ls, dpairs=dpairs, dtotal=dtotal)
        np.testing.assert_allclose(losses, tl, rtol=1e-12)
        assert abs(total - sum(tl)) <= 1e-12 * abs(total)
        for a, b in zip(dzs, tdz):
            np.testing.assert_allclose(a, b, rtol=0, atol=1e-11)
        assert abs(dls - tdls) <= 1e-11 * max(1.0, abs(tdls))
        assert (dls == 0.0) == (ls < 0)


def test_dlogit_scale_is_sum_G_times_S_and_matches_a_difference_quotient():
    za, zb = hr.ntx_inputs(37, 260)
    inv_T = tr.inv_temperature(tr.LS_T01)
    loss, _, _, gs, G, S = tr._pair_terms(za, zb, inv_T, hr.ALPHA, True)
    _, _, _, dls = tr.nt_xent_ls_f64(za, zb, tr.LS_T01)
    assert abs(dls - float((G * S).sum())) <= 1e-14 * abs(dls) and dls == gs
    # G is d loss / d S: rows of softmax - I sum to zero on either side
    assert abs(G.sum()) < 1e-14
    h = 1e-6
    s = float(np.float32(tr.LS_T01))
    lp = tr._pair_terms(za, zb, math.exp(s + h), hr.ALPHA, True)[0]
    lm = tr._pair_terms(za, zb, math.exp(s - h), hr.ALPHA, True)[0]
    assert abs((lp - lm) / (2 * h) - dls) <= 1e-8 * max(1.0, abs(dls))


def test_batch_of_one_has_no_temperature_gradient():
    za, zb = hr.ntx_inputs(1, 4)
    loss, _, _, dls = tr.nt_xent_ls_f64(za, zb, tr.LS_T01)
    assert dls == 0.0 and loss == 0.0


def test_adam_restatement_matches_torch_adam():
    grads = [0.3, -0.2, 0.05]
    p = torch.nn.Parameter(torch.tensor(2.0, dtype=torch.float64))
    opt = torch.optim.Adam([p], lr=1e-2, weight_decay=1e-3)
    for g in grads:
        p.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
    pp, m, v = tr.adam_f64(2.0, grads, 1e-2, weight_decay=1e-3)
    st = opt.state[p]
    assert abs(pp - float(p.detach())) < 1e-14 and abs(m - float(st["exp_avg"])) < 1e-16 and abs(v - float(st["exp_avg_sq"])) < 1e-16


# ------------------------------------------------------------------------------------------------ C ABI
NEW_SYMBOLS = {"tri_ntxent_ls_workspace": 3, "tri_ntxent_ls_fwd_bwd": 15, "tri_ntxent_ls_bwd": 15, "tri_ntxent_multi_ls_fwd": 12,
               "tri_ntxent_multi_ls_bwd": 15}


def _header_prototypes():
    text = open(os.path.join(REPO, "include", "tricolo_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(tri_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}


def test_new_symbols_are_declared_exported_and_bound():
    from tricolo_amd import _C
    if not os.path.exists(_C.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib, protos = _C.lib(), _header_prototypes()
    for name, nargs in NEW_SYMBOLS.items():
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in protos, f"{name} is not declared in tricolo_hip.h"
        assert len(protos[name].split(",")) == nargs, (name, protos[name])
        assert len(_C.SIGNATURES[name][1]) == nargs
    # the fixed twins keep their signatures; a learnable call swaps one float for (pointer, float) and the backward forms add one pointer
    for fixed, ls, extra in (("tri_ntxent_fwd_bwd", "tri_ntxent_ls_fwd_bwd", 2), ("tri_ntxent_bwd", "tri_ntxent_ls_bwd", 2),
                             ("tri_ntxent_multi_fwd", "tri_ntxent_multi_ls_fwd", 1), ("tri_ntxent_multi_bwd", "tri_ntxent_multi_ls_bwd", 2)):
        assert len(_C.SIGNATURES[ls][1]) == len(_C.SIGNATURES[fixed][1]) + extra
        assert "float temperature" in protos[fixed] and "const float* logit_scale, float max_logit_scale" in protos[ls]
    assert len(_C.SIGNATURES["tri_ntxent_fwd_bwd"][1]) == 13 and len(_C.SIGNATURES["tri_ntxent_multi_bwd"][1]) == 13
    # host-only: the learnable workspace is the fixed one plus [P][B] row partials (256-byte aligned), for M = 2 and 3
    for M, B, D in ((2, 37, 260), (3, 37, 260), (2, 8192, 4), (3, 512, 2048), (2, 1, 4)):
        P = M * (M - 1) // 2
        assert lib.tri_ntxent_ls_workspace(M, B, D) == lib.tri_ntxent_multi_workspace(M, B, D) + P * ((4 * B + 255) // 256 * 256)
    assert lib.tri_ntxent_workspace(37, 260) == lib.tri_ntxent_multi_workspace(2, 37, 260)


# ------------------------------------------------------------------------------------------------ module
def test_module_without_the_switch_is_unchanged():
    from tricolo_amd.loss.nt_xent import NTXentLoss
    for loss in (NTXentLoss(0.1, 0.25), NTXentLoss(0.1, 0.25, learnable_temperature=False)):
        assert list(loss.parameters()) == [] and list(loss.state_dict()) == [] and list(loss.buffers()) == []
        assert loss.temperature == 0.1 and loss.current_temperature() == 0.1


def test_learnable_module_owns_a_zero_d_fp32_parameter():
    from tricolo_amd.loss.nt_xent import NTXentLoss
    loss = NTXentLoss(0.1, 0.25, learnable_temperature=True)
    assert list(loss.state_dict()) == ["logit_scale"]
    p = loss.logit_scale
    assert isinstance(p, torch.nn.Parameter) and p.dim() == 0 and p.dtype == torch.float32 and p.requires_grad
    assert float(p.detach()) == float(np.float32(math.log(1 / 0.1))) and loss.temperature == 0.1
    assert abs(loss.current_temperature() - 0.1) < 1e-7
    assert loss.max_logit_scale == math.log(100.0)
    with torch.no_grad():
        p.fill_(9.0)
    assert abs(loss.current_temperature() - 0.01) < 1e-9                        # clamped at ln(100)
    with torch.no_grad():
        p.fill_(-3.0)
    assert loss.current_temperature() == 1.0
    assert NTXentLoss(0.1, 0.25, True, max_logit_scale=3.0).max_logit_scale == 3.0
    with pytest.raises(ValueError, match="max_logit_scale"):
        NTXentLoss(0.1, 0.25, True, max_logit_scale=-1.0)


def test_fixed_checkpoint_loads_into_a_learnable_module_and_says_so(capsys):
    from tricolo_amd.loss.nt_xent import NTXentLoss
    holder = torch.nn.Module()
    holder.loss_fn = NTXentLoss(0.07, 0.25, learnable_temperature=True)
    holder.load_state_dict({}, strict=True)
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "loss_fn.logit_scale" in out and "0.07" in out
    assert float(holder.loss_fn.logit_scale) == float(np.float32(math.log(1 / 0.07)))
    holder.load_state_dict({"loss_fn.logit_scale": torch.tensor(1.5)}, strict=True)
    assert float(holder.loss_fn.logit_scale) == 1.5 and capsys.readouterr().out == ""


BASE = ["data=synthetic", "model.text_encoder=BiGRUEncoder", "model.voxel_encoder=SparseCNNEncoder", "model.image_encoder=MVCNNEncoder",
        "data.voxel_size=32", "data.num_views=2", "data.image_size=64", "experiment_name=lt"]
OVERRIDE = ["+loss.NTXentLoss.learnable_temperature=true"]


def test_net_parameter_order_config_override_and_test_time_keys():
    from tricolo_amd import config as tcfg
    from tricolo_amd.model.tricolo_net import TriCoLoNet
    from tricolo_amd.parallel import BackwardSplit
    from tricolo_amd.test import select_checkpoint_keys
    fixed, learn = TriCoLoNet(tcfg.compose(overrides=BASE)), TriCoLoNet(tcfg.compose(overrides=BASE + OVERRIDE))
    names_f, names_l = [n for n, _ in fixed.named_parameters()], [n for n, _ in learn.named_parameters()]
    # the new parameter is LAST: the optimizer-state indices of existing checkpoints do not move
    assert names_l == names_f + ["loss_fn.logit_scale"]
    assert list(learn.state_dict()) [-1] == "loss_fn.logit_scale" and sorted(set(learn.state_dict()) - set(fixed.state_dict())) == ["loss_fn.logit_scale"]
    assert not any(k.startswith("loss_fn.") for k in fixed.state_dict())
    cfg3 = tcfg.compose(overrides=BASE + OVERRIDE + ["+loss.NTXentLoss.max_logit_scale=3.0"])
    assert TriCoLoNet(cfg3).loss_fn.max_logit_scale == 3.0
    # its gradient is written at the very start of the backward: it belongs to the bucket that is reduced after stage 1
    split = BackwardSplit.for_net(learn)
    assert any(p is learn.loss_fn.logit_scale for p in split.early_params)
    assert not any(p is learn.loss_fn.logit_scale for p in split.late_params)
    # tricolo_amd.test: the key loads into a learnable config and is dropped for a fixed one (strict loading either way)
    sd = learn.state_dict()
    assert "loss_fn.logit_scale" in select_checkpoint_keys(sd, tcfg.compose(overrides=BASE + OVERRIDE))
    fixed.load_state_dict(select_checkpoint_keys(sd, tcfg.compose(overrides=BASE)), strict=True)
    learn.load_state_dict(select_checkpoint_keys(sd, tcfg.compose(overrides=BASE + OVERRIDE)), strict=True)
