"""The float64 text-tower reference of tests/gru_reference.py checked against autograd and nn.GRU, and the reference-only conditions the
GPU bounds of tests/test_gpu_text_tower.py rest on (tables: profiles/r17/NOTES_text_tower.md).  No GPU."""
import numpy as np
import pytest
import torch

from oracle.modules import BiGRURef, gru_explicit, nt_xent_ref
from oracle.recipe import fill_module
from tests import gru_reference as gr
from tests.test_gpu_modules import REPLAY_BOUND
from tricolo_amd.data import synthetic as syn


def test_hand_backward_equals_autograd_of_the_explicit_forward():
    """(a) unrounded, float64: every one of the eleven gradients within 1e-12 relative L2 of autograd through gru_explicit."""
    p = gr.recipe_params()
    for B, L in ((19, 96), (5, 3)):
        tok, partner = gr.tower_tokens(B, L), gr.tower_partner(B)
        hand = gr.tower_replay(p, tok, partner)
        z, g = gr.tower_autograd(p, tok, lambda z_: nt_xent_ref(z_, partner, gr.TEMPERATURE, gr.ALPHA))
        assert float((z - hand["z"]).abs().max()) <= 1e-14
        for name in gr.PARAM_NAMES:
            assert gr.rel_l2(hand["grads"][name], g[name]) <= 1e-12, name
        assert float(hand["grads"]["embedding_layer.weight"][0].abs().max()) == 0.0
        # what tri_gru_bwd hands back is consistent with the parameter gradients made of it
        for d, s in enumerate(("", "_reverse")):
            assert gr.rel_l2(hand["dgh"][d].sum((0, 1)), g[f"gru.bias_hh_l0{s}"]) <= 1e-12
            assert gr.rel_l2(hand["dgi"][:, :, d * 384:(d + 1) * 384].sum((0, 1)), g[f"gru.bias_ih_l0{s}"]) <= 1e-12


def test_explicit_forward_equals_nn_gru_in_float32_and_float64():
    """(b) the explicit equations against torch's own GRU: float32 within 1e-5; BiGRURef.double() runs (h0 takes the embedding's dtype) and
    agrees with the float64 tower to 1e-12."""
    ref = BiGRURef(syn.DEFAULT_VOCAB, gr.OUT_DIM)
    fill_module(ref, prefix="text_encoder.")
    tok = gr.tower_tokens(19, 96)
    with torch.no_grad():
        z32 = ref(tok.long())
        emb = ref.embedding_layer(tok.long()).transpose(0, 1)
        g = ref.gru
        hf, _ = gru_explicit(emb, g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0, g.bias_hh_l0)
        hr, _ = gru_explicit(emb, g.weight_ih_l0_reverse, g.weight_hh_l0_reverse, g.bias_ih_l0_reverse, g.bias_hh_l0_reverse, reverse=True)
        _, hidden = g(emb, torch.zeros((2, 19, 128)))
        assert hf.dtype == torch.float32
        np.testing.assert_allclose(hf.numpy(), hidden[0].numpy(), atol=1e-5)
        np.testing.assert_allclose(hr.numpy(), hidden[1].numpy(), atol=1e-5)
        z_exp = torch.nn.functional.normalize(torch.tanh(ref.fc(torch.cat((hf, hr), dim=1))), dim=1)
        np.testing.assert_allclose(z_exp.numpy(), z32.numpy(), atol=1e-5)
        assert z32.dtype == torch.float32
        p = gr.tower_params(ref)
        z64 = ref.double()(tok.long())
        assert z64.dtype == torch.float64
        np.testing.assert_allclose(z64.numpy(), gr.tower_forward(p, tok)[0].numpy(), atol=1e-12)
        np.testing.assert_allclose(z64.numpy(), z32.numpy(), atol=1e-5)


def test_rounding_emulation_is_what_it_says():
    """The operand pieces: bf16 hi + lo carries 16 significand bits; the f16 variants differ only below 2^-14, where ftz gives zero."""
    x = torch.tensor([1.0 + 2.0 ** -9, 3.0e-5, 2.0 ** -14, 2.0 ** -24, 2.0 ** -26, -5.0e-6], dtype=torch.float64)
    hi, lo = gr._operands(x, "bf16x3")
    assert float(((hi + lo - x).abs() / x.abs()).max()) <= 2.0 ** -16
    ie, fz = gr._operands(x, "f16", 1.0, "ieee")[0], gr._operands(x, "f16", 1.0, "ftz")[0]
    assert ie[1] != 0 and ie[3] == 2.0 ** -24 and ie[4] == 0 and ie[5] != 0
    assert fz.tolist()[1:] == [0.0, 2.0 ** -14, 0.0, 0.0, 0.0] and fz[0] == ie[0]
    # the 2^12 of the backward: 3e-5 crosses as 0.123 and keeps 11 bits either way
    s_ie, s_fz = gr._operands(x, "f16", 4096.0, "ieee")[0], gr._operands(x, "f16", 4096.0, "ftz")[0]
    assert s_ie[1] == s_fz[1] and abs(float(s_ie[1]) / 3.0e-5 - 1) <= 2.0 ** -11


@pytest.mark.parametrize("B,L", gr.TOWER_CASES)
def test_emulated_error_table_leaves_room_under_the_replay_bounds(B, L):
    """(c) E[mode][tensor] on the inputs of the GPU replay: 4 E + 2e-5 <= REPLAY_BOUND[mode] for every tensor, so the GPU test's bound
    min(REPLAY_BOUND, 4 E + 2e-5) is the emulated one everywhere.  Also the conditions the replay's inputs promise."""
    tok, partner, ref, E = gr.tower_case(B, L)
    assert tok.shape == (B, L) and bool((tok[0] != 0).all()) and bool((tok[1] == 0).all())
    pads = (tok[2:] == 0).sum(1)
    if L == 96:
        assert int(pads.min()) >= 32 and int(pads.max()) <= 90               # the forward direction's gradient comes from behind these
    assert float((partner.norm(dim=1) - 1).abs().max()) <= 1e-12
    for mode in gr.MODES:
        for name in gr.PARAM_NAMES:
            assert 0.0 < E[mode][name] and 4 * E[mode][name] + 2e-5 <= REPLAY_BOUND[mode], (mode, name, E[mode][name])
    # the ordering of the formats: 8, 11 and 16 significand bits
    for name in gr.PARAM_NAMES:
        assert E["bf16x3"][name] < E["f16"][name] < E["bf16"][name], name
    # the loss's own gradient scale, the one the f16 path has to carry: dh of the step is ~2^-7, not randn's 1
    p = gr.recipe_params()
    z, saved = gr.tower_forward(p, tok)
    dy = (ref["dz"] - z * (ref["dz"] * z).sum(1, keepdim=True)) / saved["nrm"]
    dh = (dy * (1 - saved["y"] ** 2)) @ p["fc.weight"]
    assert 2.0 ** -10 < float(dh.pow(2).mean().sqrt()) < 2.0 ** -4 and float(dh.abs().max()) < 1.0


def _lower_end(B, L):
    """Smallest k such that the bound 4 max(E_ieee, E_ftz) + 2e-5 stays within REPLAY_BOUND["f16"] at every scale from 2^k to the upper edge."""
    sw = gr.f16_sweep(B, L)
    k = sw["upper"]
    while k - 1 >= gr.SWEEP_LOW_EXP and max(gr.sweep_bound(B, L, k - 1).values()) <= REPLAY_BOUND["f16"]:
        k -= 1
    return k


@pytest.mark.parametrize("B,L", gr.SWEEP_CASES)
def test_f16_scale_sweep_table(B, L):
    """(d) the f16 path over the scale of the upstream.  With subnormals kept the error stays at the operand rounding down to 2^-20; with
    them flushed it doubles per halving below ~2^-12.  The range over which even the flushed reading meets REPLAY_BOUND["f16"] contains the
    scale of a real step (2^-7) with room on both sides; the GPU sweep asserts the tight bound inside it."""
    sw = gr.f16_sweep(B, L)
    upper, lower = sw["upper"], _lower_end(B, L)
    assert max(float(sw["ref"]["dgh"].abs().max()), float(sw["ref"]["dgi"].abs().max())) * 2.0 ** upper * gr.F16_GATE_SCALE < gr.F16_MAX
    assert max(float(sw["ref"]["dgh"].abs().max()), float(sw["ref"]["dgi"].abs().max())) * 2.0 ** (upper + 1) * gr.F16_GATE_SCALE >= gr.F16_MAX
    assert lower == gr.SWEEP_ASSERTED_LOW and upper >= 0 and lower <= -10 and lower <= -7 <= upper
    for k in range(lower, upper + 1):
        assert max(gr.sweep_bound(B, L, k).values()) <= REPLAY_BOUND["f16"], k
    for k in (upper, 0, -7):                                    # at these scales nothing is subnormal: the two readings coincide
        row = gr.sweep_row(B, L, k)
        for n in row["ieee"]:
            assert abs(row["ieee"][n] - row["ftz"][n]) <= 0.02 * row["ieee"][n], (k, n)
    r20 = gr.sweep_row(B, L, -20)                               # here they part by two orders: the GPU sweep can tell them apart
    for n in r20["ieee"]:
        assert r20["ieee"][n] <= 3e-4 and r20["ftz"][n] >= 1e-2, n
