"""float64 reference of the text tower (embedding, input projection, both GRU recurrences, fc + tanh, normalise) with a HAND-WRITTEN
backward, on the CPU.  TEST INFRASTRUCTURE.

The equations are those of oracle.modules.gru_explicit (torch.nn.GRU docs, gate order r, z, n); the backward is written out so that it can
hand back what tri_gru_bwd hands back (dgi, dgh, hprev, the four bias sums) next to the eleven parameter gradients, and so that the one
place where the HIP recurrence rounds - the operands of its recurrent MFMA products - can be emulated while everything else stays float64:

  mode None      nothing is rounded (the reference proper)
  mode "bf16"    h_{t-1}, dgh_t and W_hh are rounded to bf16 before each recurrent product
  mode "bf16x3"  each operand is split x = hi + lo (two bf16) and the product is hi*hi + hi*lo + lo*hi, as the kernel's three MFMAs
  mode "f16"     operands rounded to f16; in the backward dgh goes through f16 as f16(4096 * dgh) / 4096 (gru.hip: the gate gradients cross
                 LDS times 2^12), in two variants: f16_variant "ieee" keeps f16 subnormals, "ftz" zeroes every |q| < 2^-14.

The relative L2 distance of an emulated replay from the unrounded one is the error the operand format alone accounts for; the GPU bounds of
tests/test_gpu_text_tower.py are built on it (tests/test_gru_reference_cpu.py holds the tables).
"""
import functools

import numpy as np
import torch

H = 128
F16_GATE_SCALE = 4096.0
F16_MAX = 65504.0
F16_MIN_NORMAL = 2.0 ** -14
MODES = ("bf16x3", "f16", "bf16")
PARAM_NAMES = ("embedding_layer.weight", "gru.weight_ih_l0", "gru.weight_hh_l0", "gru.bias_ih_l0", "gru.bias_hh_l0",
               "gru.weight_ih_l0_reverse", "gru.weight_hh_l0_reverse", "gru.bias_ih_l0_reverse", "gru.bias_hh_l0_reverse",
               "fc.weight", "fc.bias")


def rel_l2(a, ref):
    """|a - ref| / |ref| over the whole tensor, in float64.  A reference that is exactly zero (dW_hh at L = 1) asks for an exact zero."""
    a, ref = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    n = float(ref.norm())
    d = float((a - ref).norm())
    if n == 0.0:
        return 0.0 if d == 0.0 else float("inf")
    return d / n


def _r16(x, dtype):
    return x.to(torch.float32).to(dtype).to(torch.float64)


def _f16(x, variant="ieee"):
    q = _r16(x, torch.float16)
    if variant == "ftz":
        q = torch.where(q.abs() < F16_MIN_NORMAL, torch.zeros_like(q), q)
    else:
        assert variant == "ieee", variant
    return q


def _operands(x, mode, scale=1.0, variant="ieee"):
    """The 16-bit pieces an fp32 MFMA operand is fed as: [x] unrounded, [hi] in the single-product modes, [hi, lo] in the split mode.
    scale (f16 backward only): the value crosses as f16(scale * x), the product is divided by scale afterwards."""
    if mode is None:
        return [x]
    if mode == "bf16":
        return [_r16(x, torch.bfloat16)]
    if mode == "f16":
        return [_f16(x * scale, variant) / scale]
    assert mode == "bf16x3", mode
    x32 = x.to(torch.float32).to(torch.float64)
    hi = _r16(x32, torch.bfloat16)
    return [hi, _r16(x32 - hi, torch.bfloat16)]


def _product(a_parts, b_parts):
    """a @ b from operand pieces: hi*hi (+ lo*hi + hi*lo in the split mode; lo*lo is not computed by the kernel either)."""
    out = a_parts[0] @ b_parts[0]
    if len(a_parts) == 2:
        out = out + a_parts[1] @ b_parts[0] + a_parts[0] @ b_parts[1]
    return out


def gru_fwd_ref(xproj, w_hh, b_hh, mode=None):
    """xproj [L,B,768] (x W_ih^T + b_ih, 768 = dir*384 + gate*128 + unit), w_hh [2,384,128], b_hh [2,384], float64.
    -> hfinal [B,256], hs [2,L,B,128] (h after time index t), gates [2,L,B,128,4] (r, z, n, hn + b_hn): tri_gru_fwd's outputs."""
    L, B, _ = xproj.shape
    hs = xproj.new_zeros((2, L, B, H))
    gates = xproj.new_zeros((2, L, B, H, 4))
    finals = []
    for d in range(2):
        wt = _operands(w_hh[d].t().contiguous(), mode)                    # [128, 384]
        h = xproj.new_zeros((B, H))
        for t in (range(L - 1, -1, -1) if d == 1 else range(L)):
            gi = xproj[t, :, d * 384:(d + 1) * 384]
            gh = _product(_operands(h, mode), wt) + b_hh[d]
            r = torch.sigmoid(gi[:, :H] + gh[:, :H])
            z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
            n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
            h = (1 - z) * n + z * h
            hs[d, t] = h
            gates[d, t] = torch.stack((r, z, n, gh[:, 2 * H:]), dim=-1)
        finals.append(h)
    return torch.cat(finals, dim=1), hs, gates


def gru_bwd_ref(dhfinal, w_hh, hs, gates, mode=None, f16_variant="ieee"):
    """dhfinal [B,256] -> dgi [L,B,768], dgh [2,L,B,384], hprev [2,L,B,128], dbias [2,4,128] (sums over time and rows of dr, dz, dn_input,
    dn_hidden): tri_gru_bwd's outputs, the last summed over its row chunks."""
    _, L, B, _ = hs.shape
    dgi = hs.new_zeros((L, B, 768))
    dgh = hs.new_zeros((2, L, B, 384))
    hprev = hs.new_zeros((2, L, B, H))
    dbias = hs.new_zeros((2, 4, H))
    scale = F16_GATE_SCALE if mode == "f16" else 1.0
    for d in range(2):
        w = _operands(w_hh[d], mode)                                       # [384, 128]
        dh = dhfinal[:, d * H:(d + 1) * H].clone()
        order = list(range(L - 1, -1, -1)) if d == 1 else list(range(L))   # forward-time order of this direction
        for s in range(L - 1, -1, -1):
            t = order[s]
            r, z, n, ghn = gates[d, t].unbind(-1)
            hp = hs[d, order[s - 1]] if s > 0 else torch.zeros_like(dh)
            dn = dh * (1 - z)
            dz = dh * (hp - n)
            dn_pre = dn * (1 - n * n)
            dz_pre = dz * z * (1 - z)
            dr_pre = dn_pre * ghn * r * (1 - r)
            dgn = dn_pre * r
            dgi[t, :, d * 384:(d + 1) * 384] = torch.cat((dr_pre, dz_pre, dn_pre), dim=1)
            g = torch.cat((dr_pre, dz_pre, dgn), dim=1)
            dgh[d, t] = g
            hprev[d, t] = hp
            dbias[d] += torch.stack((dr_pre.sum(0), dz_pre.sum(0), dn_pre.sum(0), dgn.sum(0)))
            dh = dh * z + _product(_operands(g, mode, scale, f16_variant), w)
    return dgi, dgh, hprev, dbias


def bias_grads(dbias):
    """dbias [2,4,128] -> (db_ih_f, db_hh_f, db_ih_r, db_hh_r), [384] each: what tri_gru_bias_grads makes of the chunk sums."""
    out = []
    for d in range(2):
        out += [dbias[d, :3].reshape(384), torch.cat((dbias[d, :2].reshape(256), dbias[d, 3]))]
    return tuple(out)


def tower_params(module):
    """The eleven parameters of a BiGRUEncoder / BiGRURef as float64 CPU tensors, by state-dict name."""
    p = {k: v.detach().double().cpu() for k, v in module.state_dict().items()}
    assert set(p) == set(PARAM_NAMES), sorted(p)
    return p


def _stacked(p):
    sfx = ("", "_reverse")
    return (torch.stack([p[f"gru.weight_ih_l0{s}"] for s in sfx]), torch.stack([p[f"gru.weight_hh_l0{s}"] for s in sfx]),
            torch.stack([p[f"gru.bias_ih_l0{s}"] for s in sfx]), torch.stack([p[f"gru.bias_hh_l0{s}"] for s in sfx]))


def tower_forward(p, tokens, mode=None):
    """tokens [B,L] int -> (z [B,out] unit rows, saved).  bigru.py:15-18 from explicit equations; pads (id 0) are stepped through."""
    tok = tokens.long()
    w_ih, w_hh, b_ih, b_hh = _stacked(p)
    x = p["embedding_layer.weight"][tok].transpose(0, 1).contiguous()                   # [L,B,256]
    xproj = torch.cat([x @ w_ih[d].t() + b_ih[d] for d in range(2)], dim=2)             # [L,B,768]
    hfinal, hs, gates = gru_fwd_ref(xproj, w_hh, b_hh, mode)
    y = torch.tanh(hfinal @ p["fc.weight"].t() + p["fc.bias"])
    nrm = y.norm(dim=1, keepdim=True).clamp_min(1e-12)
    z = y / nrm
    return z, dict(tok=tok, x=x, hfinal=hfinal, hs=hs, gates=gates, y=y, nrm=nrm, z=z)


def tower_backward(p, saved, dz, mode=None, f16_variant="ieee"):
    """dz [B,out] = d loss / d z -> dict(grads={name: gradient} for the eleven parameters, dgi, dgh, hprev, dbias, bias_grads)."""
    w_ih, w_hh, _, _ = _stacked(p)
    z, y, nrm, x, tok = saved["z"], saved["y"], saved["nrm"], saved["x"], saved["tok"]
    dy = (dz - z * (dz * z).sum(1, keepdim=True)) / nrm                                  # normalise
    dpre = dy * (1 - y * y)                                                              # tanh
    grads = {"fc.weight": dpre.t() @ saved["hfinal"], "fc.bias": dpre.sum(0)}
    dgi, dgh, hprev, dbias = gru_bwd_ref(dpre @ p["fc.weight"], w_hh, saved["hs"], saved["gates"], mode, f16_variant)
    L, B, I = x.shape
    x2d = x.reshape(L * B, I)
    db = bias_grads(dbias)
    dx = x.new_zeros((L * B, I))
    for d, s in enumerate(("", "_reverse")):
        gi = dgi[:, :, d * 384:(d + 1) * 384].reshape(L * B, 384)
        grads[f"gru.weight_ih_l0{s}"] = gi.t() @ x2d
        grads[f"gru.weight_hh_l0{s}"] = dgh[d].reshape(L * B, 384).t() @ hprev[d].reshape(L * B, H)
        grads[f"gru.bias_ih_l0{s}"], grads[f"gru.bias_hh_l0{s}"] = db[2 * d], db[2 * d + 1]
        dx += gi @ w_ih[d]
    demb = torch.zeros_like(p["embedding_layer.weight"])
    demb.index_add_(0, tok.t().reshape(-1), dx)                                           # x is time-major: row l*B + b <- tok[b, l]
    demb[0] = 0.0                                                                        # padding_idx = 0 (bigru.py:10)
    grads["embedding_layer.weight"] = demb
    assert set(grads) == set(PARAM_NAMES)
    return dict(grads=grads, dgi=dgi, dgh=dgh, hprev=hprev, dbias=dbias, bias_grads=db)


def tower_autograd(p, tokens, loss_fn):
    """The same tower through oracle.modules.gru_explicit and autograd, float64: (z, {name: gradient}).  What the hand backward is checked
    against, and a second statement of the forward."""
    from oracle.modules import gru_explicit
    q = {k: v.clone().requires_grad_() for k, v in p.items()}
    emb = q["embedding_layer.weight"][tokens.long()].transpose(0, 1)
    hf, _ = gru_explicit(emb, q["gru.weight_ih_l0"], q["gru.weight_hh_l0"], q["gru.bias_ih_l0"], q["gru.bias_hh_l0"])
    hr, _ = gru_explicit(emb, q["gru.weight_ih_l0_reverse"], q["gru.weight_hh_l0_reverse"], q["gru.bias_ih_l0_reverse"],
                         q["gru.bias_hh_l0_reverse"], reverse=True)
    z = torch.nn.functional.normalize(torch.tanh(torch.cat((hf, hr), dim=1) @ q["fc.weight"].t() + q["fc.bias"]), dim=1)
    loss_fn(z).backward()
    g = {k: v.grad for k, v in q.items()}
    g["embedding_layer.weight"][0] = 0.0                                                # nn.Embedding(padding_idx=0) keeps that row's gradient zero
    return z.detach(), g


# ---------------------------------------------------------------------------------------------------------------- the replay's inputs
TEMPERATURE, ALPHA = 0.1, 0.25
OUT_DIM = 512
TOWER_CASES = ((19, 96), (33, 13), (65, 5))           # (B, L); the last one in bf16x3 only (fc leaves linear_small at 65 rows)


def tower_tokens(B, L):
    """Tokens of the synthetic batch (seed BASE_SEED + 6) cut to L steps; row 0 is overwritten with L non-pad tokens, row 1 is all pads."""
    from tricolo_amd.data import synthetic as syn
    tok = syn.make_batch(B, voxel_size=None, num_views=None, seed=syn.BASE_SEED + 6)["tokens"][:, :L].clone()
    rng = np.random.default_rng(syn.BASE_SEED + 6)
    tok[0] = torch.from_numpy(rng.integers(1, syn.DEFAULT_VOCAB, size=L).astype(np.int32))
    tok[1] = 0
    return tok


def tower_partner(B):
    """The fixed unit-norm partner embedding [B, 512] of the NT-Xent loss."""
    v = torch.randn((B, OUT_DIM), generator=torch.Generator().manual_seed(17), dtype=torch.float64)
    return v / v.norm(dim=1, keepdim=True)


def ntxent_grad(z, partner):
    """(loss, d loss / d z) of NT-Xent(z, partner) in float64 through oracle.modules.nt_xent_ref."""
    from oracle.modules import nt_xent_ref
    zl = z.detach().double().clone().requires_grad_()
    loss = nt_xent_ref(zl, partner.double(), TEMPERATURE, ALPHA)
    loss.backward()
    return float(loss.detach()), zl.grad


def recipe_params():
    from oracle.modules import BiGRURef
    from oracle.recipe import fill_module
    from tricolo_amd.data import synthetic as syn
    ref = BiGRURef(syn.DEFAULT_VOCAB, OUT_DIM)
    fill_module(ref, prefix="text_encoder.")
    return tower_params(ref)


def tower_replay(p, tokens, partner, mode=None, f16_variant="ieee"):
    z, saved = tower_forward(p, tokens, mode)
    loss, dz = ntxent_grad(z, partner)
    out = tower_backward(p, saved, dz, mode, f16_variant)
    out.update(z=z, loss=loss, dz=dz)
    return out


@functools.lru_cache(maxsize=None)
def tower_case(B, L):
    """(tokens, partner, unrounded float64 replay, E) of one replay shape, computed once per process and shared (treat as read-only).
    E[mode][tensor]: relative L2 of the mode's emulated gradient against the unrounded one; f16: the larger of the two variants."""
    p = recipe_params()
    tok, partner = tower_tokens(B, L), tower_partner(B)
    ref = tower_replay(p, tok, partner)
    E = {}
    for mode in MODES:
        runs = [tower_replay(p, tok, partner, mode, v) for v in (("ieee", "ftz") if mode == "f16" else ("ieee",))]
        E[mode] = {n: max(rel_l2(r["grads"][n], ref["grads"][n]) for r in runs) for n in PARAM_NAMES}
        E[mode]["z_max_abs"] = max(float((r["z"] - ref["z"]).abs().max()) for r in runs)
    return tok, partner, ref, E


# ---------------------------------------------------------------------------------------------------------------- kernel-level inputs
def kernel_inputs(B, L, seed=3):
    """Random xproj, W_hh ~ 1 / sqrt(128), b_hh ~ 0.1, a unit-size upstream [B,256]: fp32 values, as the kernels receive them."""
    g = torch.Generator().manual_seed(seed + 1000 * B + L)
    xproj = torch.randn(L, B, 768, generator=g)
    w_hh = torch.randn(2, 384, 128, generator=g) / np.sqrt(128)
    b_hh = torch.randn(2, 384, generator=g) * 0.1
    up = torch.randn(B, 256, generator=g)
    return xproj, w_hh, b_hh, up


def kernel_replay(xproj, w_hh, b_hh, up, mode=None, f16_variant="ieee"):
    """float64 fwd + bwd of the recurrence alone -> dict(hfinal, hs, gates, dgi, dgh, hprev, dbias, bias_grads, dw_hh [2,384,128])."""
    xproj, w_hh, b_hh, up = (t.double() for t in (xproj, w_hh, b_hh, up))
    hfinal, hs, gates = gru_fwd_ref(xproj, w_hh, b_hh, mode)
    dgi, dgh, hprev, dbias = gru_bwd_ref(up, w_hh, hs, gates, mode, f16_variant)
    L, B, _ = xproj.shape
    dw_hh = torch.stack([dgh[d].reshape(L * B, 384).t() @ hprev[d].reshape(L * B, H) for d in range(2)])
    return dict(hfinal=hfinal, hs=hs, gates=gates, dgi=dgi, dgh=dgh, hprev=hprev, dbias=dbias, bias_grads=bias_grads(dbias), dw_hh=dw_hh)


def rescale_backward(fwd, w_hh, up, mode=None, f16_variant="ieee"):
    """The backward of kernel_replay again for another upstream, on the forward already computed (the forward does not depend on it)."""
    dgi, dgh, hprev, dbias = gru_bwd_ref(up.double(), w_hh.double(), fwd["hs"], fwd["gates"], mode, f16_variant)
    _, L, B, _ = fwd["hs"].shape
    dw_hh = torch.stack([dgh[d].reshape(L * B, 384).t() @ hprev[d].reshape(L * B, H) for d in range(2)])
    return dict(dgi=dgi, dgh=dgh, hprev=hprev, dbias=dbias, bias_grads=bias_grads(dbias), dw_hh=dw_hh)


def sweep_tensors(r):
    """The tensors the f16 sweep measures, per direction: dgi, dgh, dW_hh."""
    out = {}
    for d, s in enumerate(("fwd", "rev")):
        out[f"dgi/{s}"] = r["dgi"][:, :, d * 384:(d + 1) * 384]
        out[f"dgh/{s}"] = r["dgh"][d]
        out[f"dw_hh/{s}"] = r["dw_hh"][d]
    return out


def f16_upper_edge(ref):
    """Largest power of two s with max |dgate| * s * 4096 < 65504, dgate of the float64 reference at unit scale (the backward is linear in
    the upstream): above it f16(4096 * dgate) overflows."""
    m = max(float(ref["dgh"].abs().max()), float(ref["dgi"].abs().max()))
    k = int(np.floor(np.log2(F16_MAX / (F16_GATE_SCALE * m))))
    while m * 2.0 ** k * F16_GATE_SCALE >= F16_MAX:
        k -= 1
    return k


SWEEP_CASES = ((8, 96), (19, 96))
SWEEP_LOW_EXP = -24
SWEEP_ASSERTED_LOW = -15       # the table's lower end: from 2^-15 up even the flushed reading stays within REPLAY_BOUND["f16"] (test_gru_reference_cpu.py)


@functools.lru_cache(maxsize=None)
def f16_sweep(B, L):
    """The f16 sweep's fixed part: dict(inputs, ref (unit scale, unrounded), fwd (the f16-emulated forward), upper=k_max).  The unrounded
    backward is linear in the upstream, so the unit-scale reference serves every scale 2^k."""
    xproj, w_hh, b_hh, up = kernel_inputs(B, L)
    ref = kernel_replay(xproj, w_hh, b_hh, up)
    fwd = kernel_replay(xproj, w_hh, b_hh, up, "f16")
    return dict(inputs=(xproj, w_hh, b_hh, up), ref=ref, fwd=fwd, upper=f16_upper_edge(ref), tensors=sweep_tensors(ref))


def sweep_emulation(B, L, k, variant):
    """The tensors of sweep_tensors from the f16 emulation with the upstream 2^k * (unit randn), divided by 2^k again."""
    sw = f16_sweep(B, L)
    _, w_hh, _, up = sw["inputs"]
    s = 2.0 ** k
    return {n: t / s for n, t in sweep_tensors(rescale_backward(sw["fwd"], w_hh, up.double() * s, "f16", variant)).items()}


@functools.lru_cache(maxsize=None)
def sweep_row(B, L, k):
    """Emulated error of the f16 path at scale 2^k against the unrounded replay: {"ieee": {tensor: E}, "ftz": {tensor: E}}."""
    ref = f16_sweep(B, L)["tensors"]
    return {v: {n: rel_l2(t, ref[n]) for n, t in sweep_emulation(B, L, k, v).items()} for v in ("ieee", "ftz")}


def sweep_bound(B, L, k):
    """4 * max(E_ieee, E_ftz) + 2e-5 per tensor at scale 2^k."""
    row = sweep_row(B, L, k)
    return {n: 4 * max(row["ieee"][n], row["ftz"][n]) + 2e-5 for n in row["ieee"]}


# ---------------------------------------------------------------------------------------------------------------- edge shapes
EDGE_CASES = ((1, 1), (16, 6), (17, 12), (32, 18), (3, 2))


def edge_tensors(r):
    """What the edge test compares: hfinal, dgi, the four nn.GRU bias gradients, dW_hh per direction."""
    out = {"hfinal": r["hfinal"], "dgi": r["dgi"], "dw_hh/fwd": r["dw_hh"][0], "dw_hh/rev": r["dw_hh"][1]}
    out.update(zip(("db_ih/fwd", "db_hh/fwd", "db_ih/rev", "db_hh/rev"), r["bias_grads"]))
    return out


@functools.lru_cache(maxsize=None)
def edge_case(B, L):
    """(inputs, unrounded float64 tensors, E[mode][tensor]) of one edge shape at unit upstream scale; f16: the larger of the two variants."""
    inp = kernel_inputs(B, L)
    ref = edge_tensors(kernel_replay(*inp))
    E = {}
    for mode in MODES:
        runs = [edge_tensors(kernel_replay(*inp, mode, v)) for v in (("ieee", "ftz") if mode == "f16" else ("ieee",))]
        E[mode] = {n: max(rel_l2(r[n], ref[n]) for r in runs) for n in ref}
    return inp, ref, E
