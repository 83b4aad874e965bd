"""CPU: tests/golden/triplet.npz (written by tools/make_triplet_golden.py from the REAL tricolo.loss.triplet.TripletLoss) against the
float64 numpy restatement tests/triplet_reference.py, and the config / checkpoint surface of loss.name=TripletLoss."""
import hashlib
import os

import numpy as np
import pytest

from tests import triplet_reference as tr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "triplet.npz")
CASES = [str(t) for t in np.load(GOLDEN, allow_pickle=False)["cases"]]
RESTATEMENT_TOL = 1e-12


def case_inputs(g, tag):
    """The case's fp32 inputs from its recipe, checked against the recorded SHA-256."""
    a, b = tr.make_inputs(str(g[f"{tag}/kind"]), int(g[f"{tag}/B"]), int(g[f"{tag}/D"]), int(g[f"{tag}/r"]), float(g[f"{tag}/s"]),
                          int(g[f"{tag}/seed"]), bool(g[f"{tag}/normalise"]))
    assert hashlib.sha256(a.numpy().tobytes() + b.numpy().tobytes()).hexdigest() == str(g[f"{tag}/sha256"]), \
        f"{tag}: the recipe no longer yields the arrays the fixture was computed from"
    return a, b


def check_against_fixture(g, tag, loss, dzis, dzls, tol_loss, tol_grad, scale=1.0, report=None):
    """loss / gradients (gradients taken with upstream factor `scale`) against the fixture's float64 reference values: relative on
    the loss, relative L2 on each gradient - on the whole array where the fixture holds it, else on the sampled rows, on the
    vector of row norms and on the total norm."""
    ref = float(g[f"{tag}/loss64"])
    figures = {"loss": abs(float(loss) - ref) / abs(ref)}
    for name, got in (("dzis", dzis), ("dzls", dzls)):
        got = np.asarray(got, dtype=np.float64) / scale
        if f"{tag}/{name}64" in g:
            figures[name] = tr.rel_l2(got, g[f"{tag}/{name}64"])
        else:
            rows = g[f"{tag}/{name}_rows"]
            figures[name + " rows"] = tr.rel_l2(got[rows], g[f"{tag}/{name}64_rows"])
            figures[name + " rownorms"] = tr.rel_l2(np.linalg.norm(got, axis=1), g[f"{tag}/{name}64_rownorms"])
            figures[name + " norm"] = abs(np.linalg.norm(got) - float(g[f"{tag}/{name}64_norm"])) / float(g[f"{tag}/{name}64_norm"])
    if report is not None:
        print(f"{report} {tag}: " + "  ".join(f"{k} {v:.3e}" for k, v in figures.items()) + f"   (bounds: loss {tol_loss:.3e}, gradient {tol_grad:.3e})")
    for k, v in figures.items():
        assert v <= (tol_loss if k == "loss" else tol_grad), (tag, k, v)


@pytest.mark.parametrize("tag", CASES)
def test_restatement_reproduces_the_reference(golden, tag):
    g = golden("triplet")
    a, b = case_inputs(g, tag)
    margin = float(g[f"{tag}/margin"])
    m = tr.triplet(a.numpy(), b.numpy(), margin)
    assert (m.n_semi, m.n_hard) == (int(g[f"{tag}/n_semi"]), int(g[f"{tag}/n_hard"]))
    assert m.gap == pytest.approx(float(g[f"{tag}/gap"]), rel=1e-6)
    if np.isnan(float(g[f"{tag}/loss64"])):                # the reference raised ZeroDivisionError
        assert m.n_semi == 0 and m.n_hard == 0 and np.isnan(m.loss) and np.isnan(m.dzis).all() and np.isnan(m.dzls).all()
        return
    check_against_fixture(g, tag, m.loss, m.dzis, m.dzls, RESTATEMENT_TOL, RESTATEMENT_TOL, report="restatement")
    # the upstream factor is linear
    m3 = tr.triplet(a.numpy(), b.numpy(), margin, upstream=0.75)
    assert tr.rel_l2(m3.dzis, 0.75 * m.dzis) < 1e-14 and tr.rel_l2(m3.dzls, 0.75 * m.dzls) < 1e-14


def test_restatement_gradient_is_the_derivative_of_its_loss():
    """Central differences on the restatement itself (float64), swapped-norm formula and non-unit rows included."""
    a, b = tr.make_inputs("clustered", 6, 8, 2, 0.6, 5, normalise=False)
    a, b = a.double().numpy(), b.double().numpy()
    m = tr.triplet(a, b, 0.3)
    assert m.n_semi > 0 and m.gap > 1e-3
    h = 1e-6
    for arr, grad in ((a, m.dzis), (b, m.dzls)):
        num = np.zeros_like(arr)
        for idx in np.ndindex(arr.shape):
            old = arr[idx]
            arr[idx] = old + h
            up = tr.triplet(a, b, 0.3).loss
            arr[idx] = old - h
            dn = tr.triplet(a, b, 0.3).loss
            arr[idx] = old
            num[idx] = (up - dn) / (2 * h)
        assert tr.rel_l2(grad, num) < 1e-7


def test_fixture_meets_its_conditions(golden):
    g = golden("triplet")
    semi = [t for t in CASES if int(g[f"{t}/n_semi"]) > 0]
    hard = [t for t in CASES if int(g[f"{t}/n_semi"]) == 0 and int(g[f"{t}/n_hard"]) > 0]
    empty = [t for t in CASES if int(g[f"{t}/n_semi"]) == 0 and int(g[f"{t}/n_hard"]) == 0]
    assert semi and hard and empty                                           # every branch
    assert any(not bool(g[f"{t}/normalise"]) and str(g[f"{t}/kind"]) == "clustered" for t in CASES)      # the swapped norms show
    assert all(float(g[f"{t}/gap"]) >= 1e-5 for t in CASES)                  # no candidate on a threshold
    assert {int(g[f"{t}/B"]) for t in CASES} >= {2, 5, 32, 48, 64, 200, 512}
    assert os.path.getsize(GOLDEN) < 1 << 20
    errs_l = [float(g[f"{t}/err_loss32"]) for t in CASES if f"{t}/err_loss32" in g]
    errs_g = [float(g[f"{t}/err_{n}32"]) for t in CASES for n in ("dzis", "dzls") if f"{t}/err_{n}32" in g]
    assert float(g["max_err_loss32"]) == max(errs_l) and float(g["max_err_grad32"]) == max(errs_g)
    assert 1e-7 < max(errs_l) < 1e-3 and 1e-7 < max(errs_g) < 1e-4           # fp32 noise of the reference, neither zero nor broken


def test_config_selects_triplet_loss():
    from tricolo_amd import config as tcfg
    from tricolo_amd.checkpoint import reference_targets
    cfg = tcfg.compose(overrides=["data=synthetic", "model.text_encoder=BiGRUEncoder", "loss.name=TripletLoss"])
    assert cfg.loss.name == "TripletLoss"
    loss_fn = tcfg.instantiate(getattr(cfg.loss, cfg.loss.name))
    from tricolo_amd.loss.triplet import TripletLoss
    assert type(loss_fn) is TripletLoss and loss_fn.margin == 0.025 and loss_fn.last_counts is None
    assert callable(loss_fn.all_pairs)
    default = tcfg.compose(overrides=["data=synthetic", "model.text_encoder=BiGRUEncoder"])
    assert default.loss.name == "NTXentLoss"                                 # the default loss is unchanged
    plain = cfg.to_dict()
    mapped = reference_targets(plain)
    assert mapped["loss"]["TripletLoss"] == {"_target_": "tricolo.loss.triplet.TripletLoss", "margin": 0.025}
    assert reference_targets(mapped, back=True)["loss"]["TripletLoss"]["_target_"] == "tricolo_amd.loss.triplet.TripletLoss"


def test_triplet_needs_a_gpu_and_knows_its_fused_range():
    import torch
    from tricolo_amd import ops
    from tricolo_amd.loss.triplet import TripletLoss
    with pytest.raises(RuntimeError, match="MI355X"):
        TripletLoss(0.025)(torch.zeros(4, 8), torch.zeros(4, 8))
    assert TripletLoss(0.025).all_pairs([torch.zeros(4, 8), torch.zeros(4, 8)]) is None          # host tensors: not the fused path
    assert ops.triplet_multi_supported(64, 512, 3) and ops.triplet_multi_supported(2, 4, 2) and ops.triplet_multi_supported(512, 2048, 3)
    assert not any(ops.triplet_multi_supported(*a) for a in ((1, 512, 3), (600, 512, 3), (64, 6, 3), (64, 2052, 2), (64, 512, 4)))
