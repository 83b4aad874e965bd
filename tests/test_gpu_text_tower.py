"""The text tower's backward pinned to float64 in every precision mode (tests/gru_reference.py is the reference).

Tower replay: BiGRUEncoder forward + NT-Xent + backward against the float64 explicit-equation tower with its hand-written backward, on a
batch with a ragged last chunk, a row without pads and a row of pads only, with the gradient scale of a training step.  Every one of the
eleven parameter gradients is compared as a whole tensor, relative L2 <= min(REPLAY_BOUND[mode], 4 E[mode][tensor] + 2e-5), where E is the
error the mode's MFMA operand rounding accounts for in the float64 emulation (tests/test_gru_reference_cpu.py asserts 4 E + 2e-5 <=
REPLAY_BOUND for every tensor).  The 4 x covers fp32 accumulation and the 1-ulp exp / rcp gates, which the emulation leaves out; 2e-5 is the
project's fp32-grade kernel tolerance.

Kernel level (ops.gru_fwd / ops.gru_bwd on random gate pre-activations): exact power-of-two scaling of the bf16 / bf16x3 backward, the f16
backward over the scale of its upstream (upper edge of f16's range down to 2^-20), bit-exact independence of batch rows from their chunk and
slot, and the edge shapes in relative terms.  Measured figures go into the parity report of
tests/test_gpu_modules.py under "text_tower/..." (copied to profiles/r17/text_tower_report.json)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tricolo_amd import ops
    from tricolo_amd.model.module.text_encoder.bigru import BiGRUEncoder

from oracle.recipe import fill_module
from tests import gru_reference as gr
from tests.test_gpu_modules import EMB_TOL, LOSS_TOL, REPLAY_BOUND, _report as _parity_report
from tricolo_amd.data import synthetic as syn

DEV = "cuda"
MODES = list(gr.MODES)


def _report(key, value):
    _parity_report("text_tower/" + key, value)


@pytest.fixture(autouse=True)
def _precision():
    ops.set_default_precision("bf16x3")
    yield
    ops.set_default_precision("bf16x3")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


# ------------------------------------------------------------------------------------------------------------------ the tower replay
TOWER_PARAMS = [(prec, B, L) for (B, L) in gr.TOWER_CASES[:2] for prec in MODES] + [("bf16x3",) + gr.TOWER_CASES[2]]


@pytest.mark.parametrize("prec,B,L", TOWER_PARAMS)
def test_text_tower_backward_replay(prec, B, L):
    """B = 19: one full chunk of 16 rows + a ragged chunk of 3, L = 96; (33, 13): three chunks, the last with one row; (65, 5): fc and its
    backward leave linear_small for the generic dense path.  Row 0 has no pad, row 1 nothing but pads; the other rows end in 32 to 90 pads, so
    the forward direction's weight_ih gradient comes only from steps behind them.  The upstream is NT-Xent's own gradient (T = 0.1,
    alpha = 0.25, a fixed unit-norm partner): dh of the recurrence has rms ~1e-2, not randn's 1."""
    tok, partner, ref, E = gr.tower_case(B, L)
    m = BiGRUEncoder(syn.DEFAULT_VOCAB, gr.OUT_DIM, precision=prec)
    fill_module(m, prefix="text_encoder.")
    m = m.to(DEV)
    z = m(tok.to(DEV), {})
    loss, dz, _ = ops.ntxent_fwd_bwd(z.detach(), partner.float().to(DEV), gr.TEMPERATURE, gr.ALPHA)
    z.backward(dz)
    zdiff = float((z.detach().double().cpu() - ref["z"]).abs().max())
    ldiff = abs(loss.item() - ref["loss"])
    table, bounds = {}, {}
    for name, p in m.named_parameters():
        table[name] = gr.rel_l2(p.grad, ref["grads"][name])
        bounds[name] = min(REPLAY_BOUND[prec], 4 * E[prec][name] + 2e-5)
    assert set(table) == set(gr.PARAM_NAMES)
    pad_row = float(m.embedding_layer.weight.grad[0].abs().max())
    worst = max(table, key=lambda n: table[n] / bounds[n])
    _report(f"tower_replay/{prec}/B{B}_L{L}", {"embedding_max_abs_diff": zdiff, "loss_abs_diff": ldiff, "rel_l2": table, "bound": bounds,
                                               "emulated_rel_l2": {n: E[prec][n] for n in gr.PARAM_NAMES},
                                               "worst_ratio_to_bound": table[worst] / bounds[worst], "worst_tensor": worst, "pad_row_max_abs": pad_row})
    print(f"\ntower_replay {prec} B={B} L={L}: z {zdiff:.2e} loss {ldiff:.2e} " + " ".join(f"{n}={table[n]:.2e}/{bounds[n]:.2e}" for n in table))
    assert zdiff <= (EMB_TOL if prec == "bf16x3" else 5e-3)
    assert ldiff <= LOSS_TOL
    assert pad_row == 0.0
    bad = [(n, table[n], bounds[n]) for n in table if not table[n] <= bounds[n]]
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------ kernel level
def _gpu_fwd(inp, prec):
    xproj, w_hh, b_hh, _ = inp
    L, B, _ = xproj.shape
    return ops.gru_fwd(xproj.to(DEV), w_hh.to(DEV), b_hh.to(DEV), B, L, prec)


def _gpu_bwd(inp, fwd, up, prec):
    """-> dict of GPU tensors in the reference's shapes: dgi [L,B,768], dgh [2,L,B,384], hprev [2,L,B,128], dbias [chunks,2,4,128]."""
    xproj, w_hh, _, _ = inp
    L, B, _ = xproj.shape
    _, hs, gates = fwd
    dgi, dgh, hprev, dbias = ops.gru_bwd(up.to(DEV), w_hh.to(DEV), hs, gates, B, L, prec)
    return dict(dgi=dgi.view(L, B, 768), dgh=dgh.view(2, L, B, 384), hprev=hprev.view(2, L, B, 128), dbias=dbias)


def _dw_hh(r):
    """dW_hh = dgh^T hprev per direction, contracted in float64 from the GPU's stored tensors."""
    dgh, hprev = r["dgh"].double().cpu(), r["hprev"].double().cpu()
    return torch.stack([dgh[d].reshape(-1, 384).t() @ hprev[d].reshape(-1, 128) for d in range(2)])


@pytest.mark.parametrize("prec", ["bf16x3", "bf16"])
@pytest.mark.parametrize("B,L", [(19, 7), (33, 13)])
def test_gru_backward_scales_exactly_by_powers_of_two(prec, B, L):
    """The bf16 / bf16x3 backward is linear in dhfinal and made of fp32 and bf16 operations only, all of which commute with a power of
    two: gru_bwd(2^k up) == 2^k gru_bwd(up) bit for bit.  A value that crossed LDS or a register at another scale than it was stored
    (gru.hip's round-6 hazard) breaks this in one element."""
    inp = gr.kernel_inputs(B, L)
    fwd = _gpu_fwd(inp, prec)
    base = _gpu_bwd(inp, fwd, inp[3], prec)
    assert float(base["dgi"].abs().max()) > 0
    for k in (-10, 3):
        s = 2.0 ** k
        r = _gpu_bwd(inp, fwd, inp[3] * s, prec)
        for name in ("dgi", "dgh", "dbias"):
            assert _same_bits(r[name], base[name] * s), (k, name, int((_bits(r[name]) != _bits(base[name] * s)).sum()))
        assert _same_bits(r["hprev"], base["hprev"]), k


SWEEP_SCALES = ("upper", 0, -10, -20)


@pytest.mark.parametrize("scale", SWEEP_SCALES, ids=[str(s) for s in SWEEP_SCALES])
@pytest.mark.parametrize("B,L", gr.SWEEP_CASES)
def test_gru_f16_backward_over_the_scale_of_its_upstream(B, L, scale):
    """The f16 mode sends the gate gradients through LDS as f16(4096 dgate).  Upstream 2^k * randn, k = the upper edge (the largest k with
    max |dgate| 2^k 4096 < 65504 in the float64 reference; nothing above it is fed), 0, -10 and -20: dgi, dgh and dW_hh = dgh^T hprev per
    direction, relative L2 over the whole tensor <= 4 max(E_ieee, E_ftz) + 2e-5, E from the float64 emulation with f16 subnormals kept /
    flushed.  From the sweep table's lower end (gr.SWEEP_ASSERTED_LOW) to the upper edge that bound is within REPLAY_BOUND["f16"] (asserted on the CPU).
    Reported: relative L2 per 16-step bucket and the distance to either emulation - the measurement of what the hardware does with f16
    subnormals on this path."""
    sw = gr.f16_sweep(B, L)
    k = sw["upper"] if scale == "upper" else scale
    assert k <= sw["upper"]
    s = 2.0 ** k
    inp = sw["inputs"]
    r = _gpu_bwd(inp, _gpu_fwd(inp, "f16"), inp[3] * s, "f16")
    assert bool(torch.isfinite(r["dgi"]).all()) and bool(torch.isfinite(r["dgh"]).all())
    got = {n: t.double().cpu() / s for n, t in gr.sweep_tensors(dict(dgi=r["dgi"], dgh=r["dgh"], dw_hh=_dw_hh(r))).items()}
    ref, bound, row = sw["tensors"], gr.sweep_bound(B, L, k), gr.sweep_row(B, L, k)
    table = {n: gr.rel_l2(got[n], ref[n]) for n in ref}
    emu = {v: gr.sweep_emulation(B, L, k, v) for v in ("ieee", "ftz")}
    dist = {v: {n: gr.rel_l2(got[n], emu[v][n]) for n in ref} for v in emu}
    buckets = {}
    for n in ref:
        if n.startswith("dw_hh"):
            continue
        buckets[n] = {v: [gr.rel_l2(t[n][j:j + 16], ref[n][j:j + 16]) for j in range(0, L, 16)] for v, t in (("gpu", got), ("ieee", emu["ieee"]), ("ftz", emu["ftz"]))}
    di, df = sum(dist["ieee"].values()), sum(dist["ftz"].values())
    nearer = "ieee" if di < 0.5 * df else "ftz" if df < 0.5 * di else "neither (the two emulations coincide at this scale)"
    _report(f"f16_sweep/B{B}_L{L}/2^{k}", {"rel_l2": table, "bound": bound, "emulated": row, "distance_to_emulation": dist, "nearer_to": nearer,
                                           "rel_l2_per_16_steps": buckets, "upper_edge_exp": sw["upper"]})
    print(f"\nf16 sweep B={B} 2^{k}: nearer {nearer} " + " ".join(f"{n}={table[n]:.2e}/{bound[n]:.2e}" for n in table))
    if k >= gr.SWEEP_ASSERTED_LOW:
        assert max(bound.values()) <= REPLAY_BOUND["f16"]
    bad = [(n, table[n], bound[n]) for n in table if not table[n] <= bound[n]]
    assert not bad, bad


@pytest.mark.parametrize("prec", MODES)
def test_gru_rows_do_not_depend_on_their_chunk_or_slot(prec):
    """A permutation of the 19 batch rows permutes every per-row output bit for bit (rows move between the full and the ragged chunk and
    between MFMA rows), and the first 16 rows of the B = 19 run equal a B = 16 run of those rows."""
    B, L = 19, 14
    xproj, w_hh, b_hh, up = gr.kernel_inputs(B, L)
    perm = torch.from_numpy(np.random.default_rng(5).permutation(B))
    assert int((perm[:16] >= 16).sum()) > 0 and int((perm != torch.arange(B)).sum()) >= 16

    def run(x, u):
        inp = (x.contiguous(), w_hh, b_hh, u.contiguous())
        fwd = _gpu_fwd(inp, prec)
        out = _gpu_bwd(inp, fwd, inp[3], prec)
        b = x.shape[1]
        out.update(hfinal=fwd[0], hs=fwd[1].view(2, L, b, 128), gates=fwd[2].view(2, L, b, 128, 4))
        return out

    a, p, head = run(xproj, up), run(xproj[:, perm], up[perm]), run(xproj[:, :16], up[:16])
    pd = perm.to(DEV)
    for name, dim in (("hfinal", 0), ("hs", 2), ("gates", 2), ("dgi", 1), ("dgh", 2), ("hprev", 2)):
        assert float(a[name].abs().max()) > 0
        assert _same_bits(p[name], a[name].index_select(dim, pd)), (name, "permutation")
        assert _same_bits(head[name], a[name].narrow(dim, 0, 16)), (name, "B = 16 run")


@pytest.mark.parametrize("prec", MODES)
@pytest.mark.parametrize("B,L", gr.EDGE_CASES)
def test_gru_edge_shapes_in_relative_terms(prec, B, L):
    """L = 1 (hprev = 0: dW_hh must be exactly zero), L below both prefetch depths, multiples of the six-step unroll, exact and ragged
    chunks: hfinal, dgi, the four bias gradients through ops.gru_bias_grads and dW_hh per direction against float64, relative L2 per tensor
    <= min(REPLAY_BOUND[mode], 4 E + 2e-5)."""
    inp, ref, E = gr.edge_case(B, L)
    fwd = _gpu_fwd(inp, prec)
    r = _gpu_bwd(inp, fwd, inp[3], prec)
    dw = _dw_hh(r)
    got = {"hfinal": fwd[0], "dgi": r["dgi"], "dw_hh/fwd": dw[0], "dw_hh/rev": dw[1]}
    got.update(zip(("db_ih/fwd", "db_hh/fwd", "db_ih/rev", "db_hh/rev"), ops.gru_bias_grads(r["dbias"])))
    table = {n: gr.rel_l2(got[n], ref[n]) for n in ref}
    bound = {n: min(REPLAY_BOUND[prec], 4 * E[prec][n] + 2e-5) for n in ref}
    _report(f"edges/{prec}/B{B}_L{L}", {"rel_l2": table, "bound": bound})
    print(f"\nedges {prec} B={B} L={L}: " + " ".join(f"{n}={table[n]:.2e}/{bound[n]:.2e}" for n in table))
    if L == 1:
        assert float(r["hprev"].abs().max()) == 0.0 and float(dw.abs().max()) == 0.0
    bad = [(n, table[n], bound[n]) for n in table if not table[n] <= bound[n]]
    assert not bad, bad
