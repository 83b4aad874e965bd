"""GPU parity of every kernel family, called through the C ABI (tricolo_amd.ops -> libtricolo_hip.so), against
plain PyTorch-CPU fp32 / float64 restatements of the same op.  Integer-valued inputs make the bf16 MFMA path exact,
so layout / fragment-mapping mistakes show up as exact mismatches, not as tolerance noise."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tricolo_amd import ops

DEV = "cuda"


def cl3(x):       # [B,C,D,H,W] -> channels-last [B,D,H,W,C]
    return x.permute(0, 2, 3, 4, 1).contiguous()


def cf3(x):       # channels-last -> [B,C,D,H,W]
    return x.permute(0, 4, 1, 2, 3).contiguous()


def ints(shape, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).to(torch.float32)


CONV_CASES = [
    # name, B, grid(D,H,W), cin, cout, kernel, stride, pad, layout
    ("vox_l0", 2, (8, 8, 8), 3, 32, (3, 3, 3), 1, (1, 1, 1), "spconv"),
    ("vox_l1", 2, (8, 8, 8), 32, 64, (3, 3, 3), 1, (1, 1, 1), "spconv"),
    ("vox_l3", 3, (4, 4, 4), 128, 256, (3, 3, 3), 1, (1, 1, 1), "spconv"),
    ("stem7x7", 3, (1, 32, 32), 3, 64, (1, 7, 7), 2, (0, 3, 3), "torch"),
    ("c3x3s1", 2, (1, 16, 16), 64, 64, (1, 3, 3), 1, (0, 1, 1), "torch"),
    ("c3x3s2", 2, (1, 16, 16), 64, 128, (1, 3, 3), 2, (0, 1, 1), "torch"),
    ("c1x1s2", 2, (1, 16, 16), 64, 128, (1, 1, 1), 2, (0, 0, 0), "torch"),
    ("odd14", 2, (1, 14, 14), 128, 256, (1, 3, 3), 2, (0, 1, 1), "torch"),
    ("linear", 8, (1, 1, 1), 512, 512, (1, 1, 1), 1, (0, 0, 0), "torch"),
    ("clip768", 5, (1, 1, 1), 768, 512, (1, 1, 1), 1, (0, 0, 0), "torch"),
]


def make_case(case, integer, seed=0):
    name, B, grid, cin, cout, k, s, p, layout = case
    ntaps = k[0] * k[1] * k[2]
    if integer:
        x = ints((B, cin, *grid), -3, 3, seed)
        w = ints((cout, cin, *k), -2, 2, seed + 1)
    else:
        g = torch.Generator().manual_seed(seed)
        x = torch.randn((B, cin, *grid), generator=g)
        w = torch.randn((cout, cin, *k), generator=g) / np.sqrt(cin * ntaps)
    cs = 4 if cin == 3 else cin
    if layout == "spconv":
        wp = w.permute(0, 2, 3, 4, 1).contiguous()                 # [Cout,kd,kh,kw,Cin]
        strides = (ntaps * cin, cin, 1)
    else:
        wp = w.contiguous()                                        # [Cout,Cin,kd,kh,kw]
        strides = (cin * ntaps, 1, ntaps)
    geom = ops.ConvGeom(B, grid, cin, cs, cout, k, s, p, strides)
    xcl = cl3(x)
    if cs != cin:
        xcl = torch.cat([xcl, torch.zeros(*xcl.shape[:-1], cs - cin)], dim=-1).contiguous()
    return x, w, wp, xcl, geom


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
def test_conv_fwd_integer_exact(case, precision):
    x, w, wp, xcl, g = make_case(case, integer=True)
    ref = cl3(F.conv3d(x, w, stride=case[6], padding=case[7]))
    packed = ops.pack_weight(wp.to(DEV), g, precision, storage=torch.float32)
    out = ops.conv_fwd(xcl.to(DEV), g, packed).cpu()
    assert out.shape == ref.shape
    assert torch.equal(out, ref), f"max abs diff {(out - ref).abs().max().item()}"


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_fwd_float_split_precision(case):
    x, w, wp, xcl, g = make_case(case, integer=False, seed=5)
    ref = cl3(F.conv3d(x.double(), w.double(), stride=case[6], padding=case[7]))
    scale = ref.abs().max().item()
    out3 = ops.conv_fwd(xcl.to(DEV), g, ops.pack_weight(wp.to(DEV), g, "bf16x3")).cpu().double()
    out1 = ops.conv_fwd(xcl.to(DEV), g, ops.pack_weight(wp.to(DEV), g, "bf16", storage=torch.float32)).cpu().double()
    assert (out3 - ref).abs().max().item() < 2e-5 * scale          # fp32-grade
    assert (out1 - ref).abs().max().item() < 3e-2 * scale          # plain bf16 operands


@pytest.mark.parametrize("precision", ["bf16", "bf16x3", "f16"])
def test_batched_weight_packing_equals_per_layer_packing(precision):
    """tri_weight_prep_multi (LDS-transposed fast paths per parameter layout) against the element-wise tri_weight_prep for
    every layer shape of the towers, forward and data-gradient operands."""
    packer = ops.WeightPacker()
    ref = {}
    for case in CONV_CASES + [("c3x3_512", 1, (1, 4, 4), 512, 512, (1, 3, 3), 1, (0, 1, 1), "torch"),
                              ("ds1x1_odd", 1, (1, 8, 8), 72, 200, (1, 1, 1), 2, (0, 0, 0), "torch"),
                              ("vox_odd", 1, (4, 4, 4), 40, 72, (3, 3, 3), 1, (1, 1, 1), "spconv")]:
        _, _, wp, _, g = make_case(case, integer=False, seed=7)
        w = wp.to(DEV)
        for tr in (False, True):
            if tr and (g.cin != g.cin_stored or g.cin % 4):
                continue
            packer.add((case[0], tr), w, g, transposed=tr)
            ref[(case[0], tr)] = ops.pack_weight(w, g, precision, transposed=tr)
    out = packer.run(precision, torch.device(DEV))
    for key, (hi, lo) in ref.items():
        assert torch.equal(out[key][0], hi), key
        if lo is not None:
            assert torch.equal(out[key][1], lo), key


def test_conv_fwd_mask_bias_act_stats():
    case = CONV_CASES[1]
    x, w, wp, xcl, g = make_case(case, integer=True, seed=3)
    B, grid = case[1], case[2]
    M = B * grid[0] * grid[1] * grid[2]
    gen = torch.Generator().manual_seed(9)
    mask = (torch.rand(M, generator=gen) < 0.3).to(torch.uint8)
    mask[:256] = 0                                                  # two fully inactive 128-row tiles
    ref = cl3(F.conv3d(x, w, padding=1)).reshape(M, -1) * mask[:, None].float()
    packed = ops.pack_weight(wp.to(DEV), g, "bf16", storage=torch.float32)
    out, stats = ops.conv_fwd(xcl.to(DEV), g, packed, row_mask=mask.to(DEV), want_stats=True)
    out = out.cpu().reshape(M, -1)
    assert torch.equal(out, ref)
    st = stats.cpu().double().sum(0)
    np.testing.assert_allclose(st[0].numpy(), ref.double().sum(0).numpy(), rtol=1e-6, atol=1e-3)
    np.testing.assert_allclose(st[1].numpy(), (ref.double() ** 2).sum(0).numpy(), rtol=1e-6, atol=1e-3)
    bias = ints((case[4],), -2, 2, 4)
    out2 = ops.conv_fwd(xcl.to(DEV), g, packed, bias=bias.to(DEV), act=1).cpu().reshape(M, -1)
    assert torch.equal(out2, F.relu(cl3(F.conv3d(x, w, padding=1)).reshape(M, -1) + bias))
    out3 = ops.conv_fwd(xcl.to(DEV), g, packed, bias=bias.to(DEV), act=2).cpu().reshape(M, -1)
    np.testing.assert_allclose(out3.numpy(), torch.tanh(cl3(F.conv3d(x, w, padding=1)).reshape(M, -1) + bias).numpy(), atol=2e-6)


@pytest.mark.parametrize("precision,mode", [("bf16", 0), ("bf16x3", 1)])
def test_conv_fwd_stats_from_the_unsplit_generic_kernel(precision, mode):
    """The BatchNorm records conv_igemm_kernel's own epilogue writes (fp32 storage, no split-K: the small layers above are split over K
    and get their records from conv_splitk_finish_kernel).  A 1x1x1 layer with two k-steps is never split (plan_generic asks for eight);
    300 rows = two full 128-row tiles and a partial one, 192 channels = three 64-wide channel tiles.  |x| <= 2, |w| <= 1 over 64 inputs:
    |out| <= 128, so a record's sum of squares is at most 128 * 128^2 = 2^21 - every fp32 sum is exact and the records must add up to the
    float64 column sums exactly."""
    M, cin, cout = 300, 64, 192
    g = ops.ConvGeom(M, (1, 1, 1), cin, cin, cout, (1, 1, 1), 1, (0, 0, 0), (cin, 1, 1))
    assert (g.kernel_family[(False, mode)] & 255) == 0 and not g.splitk(False, mode)
    x = ints((M, cin), -2, 2, 91)
    w = ints((cout, cin), -1, 1, 92)
    ref = x @ w.t()
    assert float(ref.abs().max()) <= 128
    packed = ops.pack_weight(w.view(cout, cin, 1, 1, 1).to(DEV), g, precision, storage=torch.float32)
    out, stats = ops.conv_fwd(x.view(M, 1, 1, 1, cin).to(DEV), g, packed, want_stats=True)
    assert stats.shape == (g.num_mtiles[mode], 2, cout) and g.num_mtiles[mode] == 3
    assert torch.equal(out.cpu().view(M, cout), ref)
    st = stats.cpu().double().sum(0)
    assert torch.equal(st[0], ref.double().sum(0)) and torch.equal(st[1], (ref.double() ** 2).sum(0))


DGRAD_CASES = [c for c in CONV_CASES if c[3] != 3]


@pytest.mark.parametrize("case", DGRAD_CASES, ids=[c[0] for c in DGRAD_CASES])
@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
def test_conv_dgrad_integer_exact(case, precision):
    x, w, wp, xcl, g = make_case(case, integer=True, seed=7)
    xr = x.clone().requires_grad_()
    y = F.conv3d(xr, w, stride=case[6], padding=case[7])
    dy = ints(tuple(y.shape), -2, 2, 11)
    y.backward(dy)
    ref = cl3(xr.grad)
    packed_t = ops.pack_weight(wp.to(DEV), g, precision, transposed=True, storage=torch.float32)
    dx = ops.conv_dgrad(cl3(dy).to(DEV), g, packed_t).cpu()
    assert torch.equal(dx, ref), f"max abs diff {(dx - ref).abs().max().item()}"
    base = ints(tuple(ref.shape), -5, 5, 13)
    dx2 = ops.conv_dgrad(cl3(dy).to(DEV), g, packed_t, out=base.clone().to(DEV), accumulate=True).cpu()
    assert torch.equal(dx2, ref + base)


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
def test_conv_wgrad_integer_exact(case, precision):
    x, w, wp, xcl, g = make_case(case, integer=True, seed=17)
    wr = w.clone().requires_grad_()
    y = F.conv3d(x, wr, stride=case[6], padding=case[7])
    dy = ints(tuple(y.shape), -2, 2, 19)
    y.backward(dy)
    ref = wr.grad
    if case[8] == "spconv":
        ref = ref.permute(0, 2, 3, 4, 1).contiguous()
    dw = ops.conv_wgrad(xcl.to(DEV), cl3(dy).to(DEV), g, wp.to(DEV), precision).cpu()
    assert dw.shape == ref.shape
    assert torch.equal(dw, ref), f"max abs diff {(dw - ref).abs().max().item()}"


# Real-valued data: the lo terms of the 3-product split (a_lo*b_hi + a_hi*b_lo) only matter here - integer data has lo == 0.
# Reference in float64; bound 2e-5 * scale for bf16x3 (operand error ~2^-17), 3e-2 * scale for single bf16 operands.
@pytest.mark.parametrize("case", DGRAD_CASES, ids=[c[0] for c in DGRAD_CASES])
def test_conv_dgrad_float_split_precision(case):
    x, w, wp, xcl, g = make_case(case, integer=False, seed=71)
    xr = x.double().requires_grad_()
    y = F.conv3d(xr, w.double(), stride=case[6], padding=case[7])
    dy = torch.randn(tuple(y.shape), generator=torch.Generator().manual_seed(73))
    y.backward(dy.double())
    ref = cl3(xr.grad)
    scale = ref.abs().max().item()
    dx3 = ops.conv_dgrad(cl3(dy).to(DEV), g, ops.pack_weight(wp.to(DEV), g, "bf16x3", transposed=True)).cpu().double()
    dx1 = ops.conv_dgrad(cl3(dy).to(DEV), g, ops.pack_weight(wp.to(DEV), g, "bf16", transposed=True, storage=torch.float32)).cpu().double()
    assert (dx3 - ref).abs().max().item() < 2e-5 * scale
    assert (dx1 - ref).abs().max().item() < 3e-2 * scale
    assert (dx1 - ref).abs().max().item() > 1e-4 * scale          # the single-operand path really is the coarser one


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_wgrad_float_split_precision(case):
    x, w, wp, xcl, g = make_case(case, integer=False, seed=79)
    wr = w.double().requires_grad_()
    y = F.conv3d(x.double(), wr, stride=case[6], padding=case[7])
    dy = torch.randn(tuple(y.shape), generator=torch.Generator().manual_seed(83))
    y.backward(dy.double())
    ref = wr.grad.permute(0, 2, 3, 4, 1).contiguous() if case[8] == "spconv" else wr.grad
    scale = ref.abs().max().item()
    dw3 = ops.conv_wgrad(xcl.to(DEV), cl3(dy).to(DEV), g, wp.to(DEV), "bf16x3").cpu().double()
    dw1 = ops.conv_wgrad(xcl.to(DEV), cl3(dy).to(DEV), g, wp.to(DEV), "bf16").cpu().double()
    assert (dw3 - ref).abs().max().item() < 2e-5 * scale
    assert (dw1 - ref).abs().max().item() < 3e-2 * scale
    assert (dw1 - ref).abs().max().item() > 1e-5 * scale


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_f16_storage_float_precision(case):
    """f16 mode: operands and results rounded to f16 (11 significand bits) - 8x tighter than bf16 storage; fwd / dgrad / wgrad."""
    x, w, wp, xcl, g = make_case(case, integer=False, seed=89)
    xr, wr = x.double().requires_grad_(), w.double().requires_grad_()
    y = F.conv3d(xr, wr, stride=case[6], padding=case[7])
    dy = torch.randn(tuple(y.shape), generator=torch.Generator().manual_seed(97))
    y.backward(dy.double())
    h = torch.float16
    out = ops.conv_fwd(xcl.to(DEV).to(h), g, ops.pack_weight(wp.to(DEV), g, "f16")).cpu().double()
    ref = cl3(y.detach())
    assert (out - ref).abs().max().item() < 2e-3 * ref.abs().max().item()
    refw = wr.grad.permute(0, 2, 3, 4, 1).contiguous() if case[8] == "spconv" else wr.grad
    dw = ops.conv_wgrad(xcl.to(DEV).to(h), cl3(dy).to(DEV).to(h), g, wp.to(DEV), "f16", out_scale=0.5).cpu().double()
    assert (2.0 * dw - refw).abs().max().item() < 2e-3 * refw.abs().max().item()
    if case[3] != 3:
        dx = ops.conv_dgrad(cl3(dy).to(DEV).to(h), g, ops.pack_weight(wp.to(DEV), g, "f16", transposed=True)).cpu().double()
        refx = cl3(xr.grad)
        assert (dx - refx).abs().max().item() < 2e-3 * refx.abs().max().item()


def test_conv_wgrad_masked_steps_skipped():
    case = CONV_CASES[1]
    x, w, wp, xcl, g = make_case(case, integer=True, seed=23)
    B, grid = case[1], case[2]
    M = B * grid[0] * grid[1] * grid[2]
    gen = torch.Generator().manual_seed(29)
    mask = (torch.rand(M, generator=gen) < 0.2).to(torch.uint8)
    mask[64:320] = 0
    wr = w.clone().requires_grad_()
    y = F.conv3d(x, wr, padding=1)
    dy = ints(tuple(y.shape), -2, 2, 31) * mask.view(B, 1, *grid).float()
    y.backward(dy)
    ref = wr.grad.permute(0, 2, 3, 4, 1).contiguous()
    dw = ops.conv_wgrad(xcl.to(DEV), cl3(dy).to(DEV), g, wp.to(DEV), "bf16", row_mask=mask.to(DEV)).cpu()
    assert torch.equal(dw, ref)


def test_linear_spatial_flatten_matches_channels_first():
    """mlp[0] at 64^3: Linear(4096) over the channels-FIRST flatten of [B,512,2,2,2] (sparse_cnn.py:49)."""
    from tricolo_amd.layers import linear_bwd, linear_fwd
    B, C, e = 4, 512, 2
    x = ints((B, C, e, e, e), -2, 2, 37)
    w = ints((512, C * e ** 3), -1, 1, 41)
    b = ints((512,), -3, 3, 43)
    xr, wr = x.clone().requires_grad_(), w.clone().requires_grad_()
    ref = F.relu(F.linear(xr.reshape(B, -1), wr, b))
    xcl = cl3(x).reshape(B, -1).to(DEV)
    out = linear_fwd(xcl, w.to(DEV), b.to(DEV), 1, "bf16", spatial=e ** 3)
    assert torch.equal(out.cpu(), ref.detach())
    dout = ints((B, 512), -2, 2, 47)
    ref.backward(dout)
    dx, dw, db = linear_bwd(xcl, w.to(DEV), out, dout.to(DEV), 1, "bf16", spatial=e ** 3)
    assert torch.equal(dw.cpu(), wr.grad)
    assert torch.equal(db.cpu(), (dout * (ref > 0)).sum(0))
    assert torch.equal(dx.cpu().view(B, e, e, e, C), cl3(xr.grad))


# ------------------------------------------------------------------------------------------------ BatchNorm
@pytest.mark.parametrize("M,K,N", [(32, 512, 512), (1, 128, 128), (19, 768, 512), (64, 256, 384)])
@pytest.mark.parametrize("act", [0, 1, 2])
def test_linear_small_matches_torch(M, K, N, act):
    """Dense layers with <= 64 rows (MLP heads): three dedicated launches.  Integer inputs are exact in both precision
    modes; real inputs are checked against float64 with the bf16x3 (near-fp32) and bf16 tolerances."""
    from tricolo_amd.layers import linear_bwd, linear_fwd
    assert ops.linear_small_supported(M, K, N)
    f = {0: lambda v: v, 1: torch.relu, 2: torch.tanh}[act]
    for precision in ("bf16", "bf16x3"):
        x, w, b = ints((M, K), -3, 3, 1), ints((N, K), -2, 2, 2), ints((N,), -2, 2, 3)
        if act != 2:
            out = linear_fwd(x.to(DEV), w.to(DEV), b.to(DEV), act, precision)
            assert torch.equal(out.cpu(), f(x @ w.t() + b))
        g = torch.Generator().manual_seed(5)
        x, w, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / np.sqrt(K), torch.randn(N, generator=g)
        ref = f(x.double() @ w.double().t() + b.double())
        dout = torch.randn(M, N, generator=g)
        out = linear_fwd(x.to(DEV), w.to(DEV), b.to(DEV), act, precision)
        dx, dw, db = linear_bwd(x.to(DEV), w.to(DEV), out, dout.to(DEV), act, precision)
        tol = 2e-5 if precision == "bf16x3" else 3e-2
        np.testing.assert_allclose(out.cpu().numpy(), ref.numpy(), atol=tol, rtol=tol)
        # backward reference with the activation derivative taken from the kernel's own forward output (a ReLU unit whose
        # pre-activation is within the forward tolerance of 0 may legitimately switch sides)
        o = out.cpu().double()
        dpre = dout.double() * {0: torch.ones_like(o), 1: (o > 0).double(), 2: 1 - o * o}[act]
        np.testing.assert_allclose(dx.cpu().numpy(), (dpre @ w.double()).numpy(), atol=tol, rtol=tol)
        np.testing.assert_allclose(dw.cpu().numpy(), (dpre.t() @ x.double()).numpy(), atol=tol * 20, rtol=tol)   # |dW| ~ 10
        np.testing.assert_allclose(db.cpu().numpy(), dpre.sum(0).numpy(), atol=tol * 4, rtol=tol)
        # the one-launch backward (weight + data gradient tiles) against the weight-gradient entry point alone
        _, dw1, db1 = linear_bwd(x.to(DEV), w.to(DEV), out, dout.to(DEV), act, precision, need_dx=False)
        assert torch.equal(dw1, dw) and torch.equal(db1, db)


@pytest.mark.parametrize("M,C,store", [(3072, 512, torch.float16), (12288, 256, torch.float16), (49152, 128, torch.float16), (49152, 128, torch.bfloat16),
                                       (100, 64, torch.float32)])
def test_bn_bwd_pair_is_two_single_backward_passes_bit_for_bit(M, C, store):
    """Round 6: bn2 and the shortcut's BatchNorm of a down-sampling BasicBlock receive the same gradient g = dout * (out > 0); ops.bn_bwd_pair
    runs ONE reduce / finalize / apply for both.  Every output must EQUAL what bn_bwd(y2, ..., relu_out=out, g_masked=...) followed by
    bn_bwd(yd, g_masked, ...) produce - down to the compiler's choice of folding the last FMA into the f16 conversion or not, which differs
    between the two single passes and which the pair kernel reproduces (a toolchain that changes either shows up here) - at the layer shapes
    of the bench step and a ragged one in fp32 storage; plus a float64 anchor."""
    gen = torch.Generator().manual_seed(97)
    ya, yb = torch.randn(M, C, generator=gen).to(DEV).to(store), (torch.randn(M, C, generator=gen) * 0.5 + 0.2).to(DEV).to(store)
    out = torch.relu(torch.randn(M, C, generator=gen)).to(DEV).to(store)
    dout = (torch.randn(M, C, generator=gen) * 64).to(DEV).to(store)
    ga, gb = (torch.rand(C, generator=gen) + 0.5).to(DEV), (torch.rand(C, generator=gen) + 0.5).to(DEV)
    coa, cob = ops.BNCoeffs(C, DEV), ops.BNCoeffs(C, DEV)
    for co, y in ((coa, ya), (cob, yb)):
        yf = y.float()
        co.mean.copy_(yf.mean(0))
        co.invstd.copy_(1.0 / torch.sqrt(yf.var(0, unbiased=False) + 1e-5))
    scale = 1.0 / 4096
    d1 = dout.clone()
    dya, dga, dba = ops.bn_bwd(ya, d1, coa, ga, count_host=M, inplace=False, relu_out=out, g_masked=d1, out_scale=scale)
    dyb, dgb, dbb = ops.bn_bwd(yb, d1, cob, gb, count_host=M, inplace=False, out_scale=scale)
    d2 = dout.clone()
    pa, pga, pba, pb, pgb, pbb = ops.bn_bwd_pair(ya, coa, ga, yb, cob, gb, d2, out, M, g_masked=d2, out_scale=scale)
    torch.cuda.synchronize()
    for a_, b_, name in ((pa, dya, "dya"), (pga, dga, "dgamma_a"), (pba, dba, "dbeta_a"), (pb, dyb, "dyb"), (pgb, dgb, "dgamma_b"), (pbb, dbb, "dbeta_b"),
                         (d2, d1, "g_masked")):
        if store == torch.float32:                          # (fp32 storage: no conversion to fold, but the FMA contraction of the two forms may differ by an ulp)
            np.testing.assert_allclose(a_.cpu().numpy(), b_.cpu().numpy(), rtol=1e-5, atol=1e-4, err_msg=name)
        else:
            assert torch.equal(a_, b_), (name, float((a_.float() - b_.float()).abs().max()))
    # float64 anchor for tensor b (the single form has its own torch parity test)
    g64 = (dout.double() * (out > 0)).cpu()
    xh = ((yb.double() - cob.mean.double()) * cob.invstd.double()).cpu()
    np.testing.assert_allclose(pgb.cpu().numpy(), ((g64 * xh).sum(0) * scale).numpy(), rtol=2e-3, atol=2e-3)
    np.testing.assert_allclose(pbb.cpu().numpy(), (g64.sum(0) * scale).numpy(), rtol=2e-3, atol=2e-3)


def test_embedding_kernels_match_torch():
    """Token lookup into time-major order and the deterministic dense weight gradient (duplicates, padding row)."""
    g = torch.Generator().manual_seed(23)
    B, L, V, D = 7, 96, 50, 256
    tok = torch.randint(0, V, (B, L), generator=g, dtype=torch.int32)       # small vocabulary: many duplicates and pads
    w = torch.randn(V, D, generator=g)
    w[0] = 0
    wr = w.clone().requires_grad_()
    ref = F.embedding(tok.t().contiguous().long(), wr, padding_idx=0)
    dout = ints((L, B, D), -3, 3, 29)                                       # integer gradients: any summation order is exact
    ref.backward(dout)
    out = ops.embedding_fwd(tok.to(DEV), w.to(DEV))
    assert torch.equal(out.cpu(), ref.detach())
    dw = ops.embedding_bwd(tok.to(DEV), dout.to(DEV), V)
    assert torch.equal(dw.cpu(), wr.grad)
    assert torch.count_nonzero(dw[0]) == 0


def test_bn2d_forward_backward_matches_torch():
    g = torch.Generator().manual_seed(3)
    N, H, W, C = 4, 6, 6, 64
    y = torch.randn(N, C, H, W, generator=g) * 2 + 0.5
    res = torch.randn(N, C, H, W, generator=g)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    rm, rv = torch.zeros(C), torch.ones(C)
    yr, gr, br, rr = y.clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_(), res.clone().requires_grad_()
    ref = F.relu(F.batch_norm(yr, rm.clone(), rv.clone(), gr, br, True, 0.1, 1e-5) + rr)
    dout = torch.randn(ref.shape, generator=g)
    ref.backward(dout)
    M = N * H * W
    ycl = y.permute(0, 2, 3, 1).contiguous().view(M, C)
    # statistics as the conv epilogue would deliver them: 128-row tiles of (sum, sumsq)
    nt = (M + 127) // 128
    stats = torch.zeros(nt, 2, C)
    for t in range(nt):
        blk = ycl[t * 128:(t + 1) * 128].double()
        stats[t, 0], stats[t, 1] = blk.sum(0).float(), (blk * blk).sum(0).float()
    rm_d, rv_d, nbt = rm.clone().to(DEV), rv.clone().to(DEV), torch.zeros((), dtype=torch.long, device=DEV)
    co = ops.bn_finalize(stats.to(DEV), C, gamma.to(DEV), beta.to(DEV), rm_d, rv_d, nbt, count_host=M)
    out = ops.bn_act(ycl.to(DEV), co, relu=True, res=res.permute(0, 2, 3, 1).contiguous().view(M, C).to(DEV))
    np.testing.assert_allclose(out.cpu().numpy(), ref.detach().permute(0, 2, 3, 1).reshape(M, C).numpy(), atol=2e-5)
    rm_ref, rv_ref = torch.zeros(C), torch.ones(C)
    F.batch_norm(y, rm_ref, rv_ref, gamma, beta, True, 0.1, 1e-5)
    np.testing.assert_allclose(rm_d.cpu().numpy(), rm_ref.numpy(), atol=1e-6)
    np.testing.assert_allclose(rv_d.cpu().numpy(), rv_ref.numpy(), rtol=1e-5)
    assert int(nbt.item()) == 1
    gz = ops.relu_bwd(dout.permute(0, 2, 3, 1).contiguous().view(M, C).to(DEV), out, inplace=False)
    dy, dgamma, dbeta = ops.bn_bwd(ycl.to(DEV), gz, co, gamma.to(DEV), count_host=M, inplace=False)
    np.testing.assert_allclose(dy.cpu().numpy(), yr.grad.permute(0, 2, 3, 1).reshape(M, C).numpy(), atol=3e-5)
    np.testing.assert_allclose(dgamma.cpu().numpy(), gr.grad.numpy(), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(dbeta.cpu().numpy(), br.grad.numpy(), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(gz.cpu().numpy(), rr.grad.permute(0, 2, 3, 1).reshape(M, C).numpy(), atol=1e-6)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_bn_bwd_recomputed_relu_mask(dtype):
    """relu(bn(y)) backward with the mask recomputed from y inside the BN passes == relu_bwd followed by bn_bwd."""
    g = torch.Generator().manual_seed(13)
    M, C = 700, 64
    y = (torch.randn(M, C, generator=g) * 2 + 0.3).to(dtype)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    yf = y.float()
    stats = torch.stack([yf.double().sum(0).float(), (yf.double() ** 2).sum(0).float()]).view(1, 2, C)
    co = ops.bn_finalize(stats.to(DEV), C, gamma.to(DEV), beta.to(DEV), None, None, None, count_host=M)
    out = ops.bn_act(y.to(DEV), co, relu=True)
    dout = torch.randn(M, C, generator=g).to(dtype).to(DEV)
    gz = ops.relu_bwd(dout, out, inplace=False)
    dy_a, dg_a, db_a = ops.bn_bwd(y.to(DEV), gz, co, gamma.to(DEV), count_host=M, inplace=False)
    dy_b, dg_b, db_b = ops.bn_bwd(y.to(DEV), dout, co, gamma.to(DEV), count_host=M, inplace=False, relu=True)
    assert torch.equal(dy_a, dy_b) and torch.equal(dg_a, dg_b) and torch.equal(db_a, db_b)
    yr, gr, br = yf.clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    F.relu(F.batch_norm(yr, None, None, gr, br, True, 0.1, 1e-5)).backward(dout.float().cpu())
    tol = 3e-5 if dtype == torch.float32 else 3e-2
    np.testing.assert_allclose(dy_b.float().cpu().numpy(), yr.grad.numpy(), atol=tol, rtol=tol)
    np.testing.assert_allclose(dg_b.cpu().numpy(), gr.grad.numpy(), rtol=2e-3 if dtype == torch.bfloat16 else 1e-4, atol=tol * 10)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_bn_bwd_residual_relu_mask(dtype):
    """relu(bn(y) + res) backward inside the BN passes (mask from the saved output, masked g written back in place)
    == relu_bwd followed by bn_bwd."""
    g = torch.Generator().manual_seed(17)
    M, C = 520, 128
    y = (torch.randn(M, C, generator=g) * 2 + 0.3).to(dtype)
    res = torch.randn(M, C, generator=g).to(dtype)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    yf = y.float()
    stats = torch.stack([yf.double().sum(0).float(), (yf.double() ** 2).sum(0).float()]).view(1, 2, C)
    co = ops.bn_finalize(stats.to(DEV), C, gamma.to(DEV), beta.to(DEV), None, None, None, count_host=M)
    out = ops.bn_act(y.to(DEV), co, relu=True, res=res.to(DEV))
    dout = torch.randn(M, C, generator=g).to(dtype).to(DEV)
    gz = ops.relu_bwd(dout, out, inplace=False)
    dy_a, dg_a, db_a = ops.bn_bwd(y.to(DEV), gz, co, gamma.to(DEV), count_host=M, inplace=False)
    d2 = dout.clone()
    dy_b, dg_b, db_b = ops.bn_bwd(y.to(DEV), d2, co, gamma.to(DEV), count_host=M, inplace=False, relu_out=out, g_masked=d2)
    assert torch.equal(dy_a, dy_b) and torch.equal(dg_a, dg_b) and torch.equal(db_a, db_b)
    assert torch.equal(d2, gz)                                      # the residual branch's gradient, written in place


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("M,C,mode", [(3072, 512, "plain"), (3072, 512, "relu"), (12288, 256, "relu_out"), (16384, 128, "rowmask"),
                                      (2048, 256, "rowmask_keep"), (777, 64, "relu"), (256, 512, "rowmask"), (243, 512, "rowmask_keep")])
def test_bn_bwd_small_matches_the_three_pass_form(monkeypatch, M, C, mode, dtype):
    """tri_bn_bwd_small (one workgroup per 4 / 8 channels over all positions: sums, coefficients and apply in one launch - the deepest
    voxel level in the product, every size it accepts here) against reduce + finalize + apply on the same tensors, every mask form, with a row mask and a
    device-side count, fp32 and f16 storage.  Same arithmetic, different summation order: dy to 1e-5 of its scale (one f16 ulp for f16
    storage), dgamma / dbeta to 1e-4."""
    g = torch.Generator().manual_seed(M + C)
    y = (torch.randn(M, C, generator=g) * 1.5 + 0.2).to(dtype).to(DEV)
    gin = torch.randn(M, C, generator=g).to(dtype).to(DEV)
    gamma, beta = (torch.rand(C, generator=g) + 0.5).to(DEV), (torch.randn(C, generator=g) * 0.3).to(DEV)
    mask = cnt = None
    rows = torch.ones(M, dtype=torch.bool)
    if mode.startswith("rowmask"):
        rows = torch.rand(M, generator=g) < 0.4
        mask = torch.zeros((M + 31) // 32 * 32, dtype=torch.uint8)
        mask[:M] = rows.to(torch.uint8)
        mask = mask.to(DEV)
        cnt = ops.mask_count(mask, M)
        y[~rows.to(DEV)] = float("nan")                                # rows of inactive sites are never read
        gin[~rows.to(DEV)] = float("nan")
    yf = y.float()[rows.to(DEV)].double()
    stats = torch.stack([yf.sum(0).float(), (yf ** 2).sum(0).float()]).view(1, 2, C)
    co = ops.bn_finalize(stats, C, gamma, beta, None, None, None, count_dev=cnt, count_host=0 if cnt is not None else M)
    kw = dict(count_dev=cnt, count_host=0 if cnt is not None else M, row_mask=mask, inplace=False, out_scale=0.5)
    res = {}
    real_small = ops.lib().tri_bn_bwd_small

    def bn_bwd_forced_small(y_, g_, co_, gamma_, count_dev=None, count_host=0, row_mask=None, inplace=True, relu=False, relu_out=None,
                            g_masked=None, out_scale=1.0, keep_inactive=False):
        """ops.bn_bwd's small branch for ANY M <= 16,384 (the product takes it for M <= 512 only)."""
        rs, rb = (co_.scale, co_.shift) if relu else (None, None)
        dy = g_ if inplace else torch.empty_like(g_)
        buf = torch.empty((2, C), dtype=torch.float32, device=DEV)
        ops.check(real_small(ops.ptr(y_), ops.ptr(g_), M, C, ops.ptr(count_dev), int(count_host), ops.ptr(gamma_), ops.ptr(co_.mean),
                             ops.ptr(co_.invstd), ops.ptr(rs), ops.ptr(rb), ops.ptr(relu_out), ops.ptr(g_masked), ops.ptr(row_mask),
                             1 if keep_inactive else 0, ops.ptr(dy), ops.ptr(buf[0]), ops.ptr(buf[1]), float(out_scale), ops._abf(y_), ops.stream()),
                  "tri_bn_bwd_small")
        return dy, buf[0], buf[1]
    for small in (True, False):
        monkeypatch.setattr(ops, "_BN_SMALL", False)
        bn_bwd = bn_bwd_forced_small if small else ops.bn_bwd
        g_in = gin.clone()
        if mode == "relu":
            out = bn_bwd(y, g_in, co, gamma, relu=True, **kw)
            extra = None
        elif mode == "relu_out":
            ro = (torch.randn(M, C, generator=torch.Generator().manual_seed(5)) > 0).to(dtype).to(DEV)
            out = bn_bwd(y, g_in, co, gamma, relu_out=ro, g_masked=g_in, **kw)
            extra = g_in
        else:
            out = bn_bwd(y, g_in, co, gamma, keep_inactive=mode == "rowmask_keep", **kw)
            extra = None
        res[small] = (out, extra)
    (dy_s, dg_s, db_s), ex_s = res[True]
    (dy_r, dg_r, db_r), ex_r = res[False]
    live = rows.to(DEV)
    scale = float(dy_r[live].float().abs().max())
    tol = 1e-5 * scale if dtype == torch.float32 else 2e-3 * scale
    assert float((dy_s[live].float() - dy_r[live].float()).abs().max()) <= tol
    if mode == "rowmask":
        assert bool((dy_s[~live] == 0).all())                          # inactive rows zeroed
    np.testing.assert_allclose(dg_s.cpu().numpy(), dg_r.cpu().numpy(), rtol=1e-4, atol=1e-4 * float(dg_r.abs().max()))
    np.testing.assert_allclose(db_s.cpu().numpy(), db_r.cpu().numpy(), rtol=1e-4, atol=1e-4 * float(db_r.abs().max()))
    if ex_s is not None:
        assert torch.equal(ex_s, ex_r)                                 # the masked gradient for the residual branch


def test_voxel_bn_pool_forward_backward_matches_oracle():
    from oracle import spconv_dense as sp
    g = torch.Generator().manual_seed(5)
    B, D, C = 2, 8, 32
    mask = (torch.rand(B, 1, D, D, D, generator=g) < 0.3).float()
    mask[1, :, 4:] = 0
    y = torch.randn(B, C, D, D, D, generator=g) * mask
    bn = torch.nn.BatchNorm1d(C)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(C, generator=g) * 0.3)
    yr = y.clone().requires_grad_()
    t = sp.masked_batchnorm(bn, sp.SparseConvTensor.from_dense(yr, mask))
    t = sp.SparseMaxPool3d(2, 2)(sp.SparseConvTensor.from_dense(F.relu(t.dense), t.mask))
    dp = torch.randn(t.dense.shape, generator=g)
    t.dense.backward(dp)
    # HIP path
    M = B * D ** 3
    ycl = cl3(y).to(DEV)
    m8 = torch.zeros((M + 31) // 32 * 32, dtype=torch.uint8)
    m8[:M] = mask.reshape(-1).to(torch.uint8)
    m8 = m8.to(DEV)
    cnt = ops.mask_count(m8, M)
    assert int(cnt.item()) == int(mask.sum().item())
    y2 = ycl.view(M, C).cpu()
    nt = (M + 127) // 128
    stats = torch.zeros(nt, 2, C)
    for i in range(nt):
        blk = y2[i * 128:(i + 1) * 128].double()
        stats[i, 0], stats[i, 1] = blk.sum(0).float(), (blk * blk).sum(0).float()
    bn2 = torch.nn.BatchNorm1d(C)
    bn2.load_state_dict({k: v.clone() for k, v in bn.state_dict().items()})
    with torch.no_grad():
        bn2.running_mean.zero_(); bn2.running_var.fill_(1.0)
    bn2 = bn2.to(DEV)
    co = ops.bn_finalize(stats.to(DEV), C, bn2.weight, bn2.bias, bn2.running_mean, bn2.running_var, bn2.num_batches_tracked, count_dev=cnt)
    pooled, mask_out = ops.bn_relu_pool3d_fwd(ycl, co, m8, B, D, C)
    np.testing.assert_allclose(cf3(pooled.cpu()).numpy(), t.dense.detach().numpy(), atol=2e-5)
    Mo = B * (D // 2) ** 3
    assert torch.equal(mask_out[:Mo].cpu().float().view(B, 1, D // 2, D // 2, D // 2), t.mask)
    np.testing.assert_allclose(bn2.running_mean.cpu().numpy(), bn.running_mean.numpy(), atol=1e-6)
    np.testing.assert_allclose(bn2.running_var.cpu().numpy(), bn.running_var.numpy(), rtol=1e-5)
    gz = ops.pool3d_bwd_route(ycl, co, m8, pooled, cl3(dp).to(DEV), B, D, C)
    dy, dgamma, dbeta = ops.bn_bwd(ycl, gz, co, bn2.weight, count_dev=cnt, row_mask=m8)
    np.testing.assert_allclose(cf3(dy.cpu()).numpy(), yr.grad.numpy(), atol=3e-5)
    np.testing.assert_allclose(dgamma.cpu().numpy(), bn.weight.grad.numpy(), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(dbeta.cpu().numpy(), bn.bias.grad.numpy(), rtol=1e-4, atol=1e-4)
    # the fused form the tower uses (routing pass + BatchNorm-backward sums in one launch): same routed gradient, sums in another order
    dy2, dgamma2, dbeta2 = ops.pool3d_bn_bwd(ycl, co, m8, pooled, cl3(dp).to(DEV), B, D, C, bn2.weight, cnt)
    np.testing.assert_allclose(cf3(dy2.cpu()).numpy(), yr.grad.numpy(), atol=3e-5)
    np.testing.assert_allclose(dgamma2.cpu().numpy(), dgamma.cpu().numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(dbeta2.cpu().numpy(), dbeta.cpu().numpy(), rtol=1e-5, atol=1e-5)
    act = m8[:B * D ** 3].bool().cpu()
    assert torch.equal(dy2.cpu().view(-1, C)[act], dy2.cpu().view(-1, C)[act])        # (finite everywhere it is defined)
    np.testing.assert_allclose(dy2.cpu().view(-1, C)[act].numpy(), dy.cpu().view(-1, C)[act].numpy(), atol=2e-6)
    # keep_inactive (level 0: its dy only feeds the weight gradient over the same mask): active rows identical, inactive rows untouched
    # - whatever pool3d_bwd_route left there - instead of zeroed
    gz3 = ops.pool3d_bwd_route(ycl, co, m8, pooled, cl3(dp).to(DEV), B, D, C)
    gz3.view(-1, C)[~act.to(DEV)] = 123.0
    dy3, dgamma3, dbeta3 = ops.bn_bwd(ycl, gz3, co, bn2.weight, count_dev=cnt, row_mask=m8, keep_inactive=True)
    assert torch.equal(dy3.cpu().view(-1, C)[act], dy.cpu().view(-1, C)[act]) and torch.equal(dgamma3, dgamma) and torch.equal(dbeta3, dbeta)
    assert bool((dy3.cpu().view(-1, C)[~act] == 123.0).all()) and bool((dy.cpu().view(-1, C)[~act] == 0.0).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_voxel_backward_row_list_forms_match_the_dense_forms(dtype):
    """tri_pool3d_bwd_route_rows (routing over the ACTIVE pooled sites) and tri_bn_bwd_rows (BatchNorm backward over the level's row
    list) against the dense, mask-skipping passes: the routed gradient bit for bit on every active row, dy on the active rows and
    dgamma / dbeta to fp32 summation-order accuracy, rows outside the list untouched."""
    g = torch.Generator().manual_seed(41)
    B, D, C = 5, 16, 32
    M = B * D ** 3
    mask = (torch.rand(B, D, D, D, generator=g) < 0.15)
    mask[1, :, 8:] = False
    y = (torch.randn(M, C, generator=g) * 1.5).to(dtype).to(DEV)
    y[~mask.reshape(-1).to(DEV)] = float("nan")                          # rows of inactive sites are never read
    m8 = torch.zeros((M + 31) // 32 * 32, dtype=torch.uint8)
    m8[:M] = mask.reshape(-1).to(torch.uint8)
    m8 = m8.to(DEV)
    rows = ops.mask_compact(m8, M)
    cnt = rows[1]
    gamma, beta = (torch.rand(C, generator=g) + 0.5).to(DEV), (torch.randn(C, generator=g) * 0.3).to(DEV)
    yf = y.float()[mask.reshape(-1).to(DEV)].double()
    stats = torch.stack([yf.sum(0).float(), (yf ** 2).sum(0).float()]).view(1, 2, C)
    co = ops.bn_finalize(stats, C, gamma, beta, None, None, None, count_dev=cnt)
    ycl = y.view(B, D, D, D, C)
    pooled, mask_out = ops.bn_relu_pool3d_fwd(ycl, co, m8, B, D, C)
    rows_out = ops.mask_compact(mask_out, B * (D // 2) ** 3)
    dp = torch.randn(pooled.shape, generator=g).to(dtype).to(DEV)
    g_dense = ops.pool3d_bwd_route(ycl, co, m8, pooled, dp, B, D, C)
    g_rows = ops.pool3d_bwd_route_rows(ycl, co, m8, pooled, dp, B, D, C, rows_out)
    act = mask.reshape(-1).to(DEV)
    assert torch.equal(g_rows.view(M, C)[act], g_dense.view(M, C)[act])
    gz = g_dense.clone()
    gz.view(M, C)[~act] = 123.0
    dy_a, dg_a, db_a = ops.bn_bwd(ycl, gz.clone(), co, gamma, count_dev=cnt, row_mask=m8, keep_inactive=True, out_scale=0.5)
    dy_b, dg_b, db_b = ops.bn_bwd_rows(ycl, gz.clone(), co, gamma, rows, out_scale=0.5)
    scale = float(dy_a.view(M, C)[act].float().abs().max())
    assert float((dy_a.view(M, C)[act].float() - dy_b.view(M, C)[act].float()).abs().max()) <= (1e-5 if dtype == torch.float32 else 2e-3) * scale
    assert bool((dy_b.view(M, C)[~act] == 123.0).all())
    np.testing.assert_allclose(dg_b.cpu().numpy(), dg_a.cpu().numpy(), rtol=1e-4, atol=1e-4 * float(dg_a.abs().max()))
    np.testing.assert_allclose(db_b.cpu().numpy(), db_a.cpu().numpy(), rtol=1e-4, atol=1e-4 * float(db_a.abs().max()))
    # (round 5) the level as SparseCNNEncoder runs it: tri_pool3d_bwd_route_rows_reduce (routing walk + BatchNorm-backward sums) ->
    # tri_bn_bwd_finalize -> tri_bn_bwd_apply_rows (level 0: keep_inactive + own row list) or tri_bn_bwd_apply (site mask)
    assert M > 16384 and ops._ROUTE_RED
    for keep, rws in ((True, rows), (False, None)):
        ref_dy, ref_dg, ref_db = ops.bn_bwd(ycl, g_dense.clone(), co, gamma, count_dev=cnt, row_mask=m8, keep_inactive=keep, out_scale=0.5)
        dy_c, dg_c, db_c = ops.pool3d_bn_bwd(ycl, co, m8, pooled, dp, B, D, C, gamma, cnt, out_scale=0.5, keep_inactive=keep, rows=rws,
                                             rows_out=rows_out)
        assert float((ref_dy.view(M, C)[act].float() - dy_c.view(M, C)[act].float()).abs().max()) <= (1e-5 if dtype == torch.float32 else 2e-3) * scale
        if not keep:
            assert bool((dy_c.view(M, C)[~act] == 0).all())
        np.testing.assert_allclose(dg_c.cpu().numpy(), ref_dg.cpu().numpy(), rtol=1e-4, atol=1e-4 * float(ref_dg.abs().max()))
        np.testing.assert_allclose(db_c.cpu().numpy(), ref_db.cpu().numpy(), rtol=1e-4, atol=1e-4 * float(ref_db.abs().max()))


@pytest.mark.parametrize("n,p", [(1, 1.0), (2047, 0.5), (2048, 0.0), (5 * 2048 + 3, 0.3), (1 << 20, 0.13), (1024 * 2048, 0.9), (1025 * 2048 + 17, 0.05)])
def test_mask_compact_matches_nonzero(n, p):
    """tri_mask_compact: positions of the non-zero mask bytes in ascending order + their count on the device - one block, block
    boundaries, an empty mask, the largest list the fused scan takes (1,024 blocks) and the first size past it (separate scan)."""
    g = torch.Generator().manual_seed(n % 1000)
    m = (torch.rand(n, generator=g) < p).to(torch.uint8)
    mpad = torch.zeros((n + 31) // 32 * 32, dtype=torch.uint8)
    mpad[:n] = m
    rows, count = ops.mask_compact(mpad.to(DEV), n)
    ref = torch.nonzero(m).flatten().int()
    assert int(count.item()) == ref.numel()
    assert torch.equal(rows[:ref.numel()].cpu(), ref)


@pytest.mark.parametrize("B,V,p", [(3, 16, 0.02), (2, 32, 0.13), (1, 48, 0.001), (5, 16, 0.0)])
def test_mask_pyramid_and_multi_list_compaction(B, V, p):
    """tri_mask_pyramid (site masks of levels 1-4 = 2x2x2 OR-pool, level by level) against max_pool3d, padding bytes zeroed, and
    tri_mask_compact_multi (all five lists in two launches) against nonzero() - what the voxel tower builds once per forward instead of a
    mask write in every pooling pass and two compaction launches per level."""
    g = torch.Generator().manual_seed(B * 100 + V)
    m = (torch.rand(B, 1, V, V, V, generator=g) < p).float()
    if p > 0:
        m[0, 0, V - 1, V - 1, V - 1] = 1                                  # the last site of a grid
    n0 = B * V ** 3
    m0 = torch.zeros((n0 + 31) // 32 * 32, dtype=torch.uint8)
    m0[:n0] = m.reshape(-1).to(torch.uint8)
    m0 = m0.to(DEV)
    outs = ops.mask_pyramid(m0, B, V)
    ref, masks, ns = m, [m0], [n0]
    for l in range(1, 5):
        ref = F.max_pool3d(ref, 2)
        n = B * (V >> l) ** 3
        got = outs[l - 1].cpu()
        assert got.numel() == (n + 31) // 32 * 32
        assert torch.equal(got[:n], ref.reshape(-1).to(torch.uint8)), f"level {l}"
        assert bool((got[n:] == 0).all()), f"level {l}: padding bytes must be zero"
        masks.append(outs[l - 1])
        ns.append(n)
    lists = ops.mask_compact_multi(masks, ns)
    for l, (rows, count) in enumerate(lists):
        refrows = torch.nonzero(masks[l][:ns[l]].cpu()).flatten().int()
        assert int(count.item()) == refrows.numel(), f"level {l}"
        assert torch.equal(rows[:refrows.numel()].cpu(), refrows), f"level {l}"
        one = ops.mask_compact(masks[l], ns[l])
        assert int(one[1].item()) == refrows.numel() and torch.equal(one[0][:refrows.numel()], rows[:refrows.numel()])


def test_window_kernels_and_multi_compaction_reject_what_they_cannot_index():
    """The 2x2x2-window kernels read the site mask two bytes at a time and index with 32-bit integers; tri_mask_compact_multi folds the scan
    into the write pass (<= 1,024 blocks per list): arguments outside that are errors, not wrong answers."""
    import ctypes
    B, D, C = 1, 4, 8
    y = torch.zeros(B, D, D, D, C, device=DEV)
    co = ops.bn_eval_coeffs(C, torch.ones(C, device=DEV), torch.zeros(C, device=DEV), torch.zeros(C, device=DEV), torch.ones(C, device=DEV))
    buf = torch.zeros(B * D ** 3 + 64, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="2-byte aligned mask"):
        ops.bn_relu_pool3d_fwd(y, co, buf[1:], B, D, C)                          # odd mask address
    with pytest.raises(RuntimeError, match="multiple of 16"):
        ops.mask_pyramid(buf, 1, 8)
    n = ops.MASK_MULTI_MAX + 2048                                                # one block too many for the fused scan
    big = torch.zeros((n,), dtype=torch.uint8, device=DEV)
    lib = ops.lib()
    n_arr = (ctypes.c_long * 1)(n)
    rows, cnt = torch.empty((n,), dtype=torch.int32, device=DEV), torch.empty((1,), dtype=torch.int32, device=DEV)
    scratch = torch.empty((lib.tri_mask_compact_multi_scratch(n_arr, 1),), dtype=torch.uint8, device=DEV)
    rc = lib.tri_mask_compact_multi((ctypes.c_void_p * 1)(big.data_ptr()), n_arr, 1, (ctypes.c_void_p * 1)(rows.data_ptr()),
                                    (ctypes.c_void_p * 1)(cnt.data_ptr()), ops.ptr(scratch), ops.stream())
    assert rc != 0
    big[5] = 1
    big[n - 1] = 1
    (r2, c2), = ops.mask_compact_multi([big], [n])                               # the Python wrapper routes such a list through tri_mask_compact
    assert int(c2.item()) == 2 and r2[:2].tolist() == [5, n - 1]


def test_maxpool2d_and_viewmax():
    g = torch.Generator().manual_seed(7)
    N, H, W, C = 6, 10, 10, 64
    x = torch.randint(0, 6, (N, C, H, W), generator=g).float()      # many ties: exercises the first-max rule
    xr = x.clone().requires_grad_()
    ref = F.max_pool2d(xr, 3, 2, 1)
    dout = torch.randn(ref.shape, generator=g)
    ref.backward(dout)
    xcl = x.permute(0, 2, 3, 1).contiguous().view(N, 1, H, W, C).to(DEV)
    out, parg = ops.maxpool2d_fwd(xcl)
    assert torch.equal(out.cpu().view(N, 5, 5, C).permute(0, 3, 1, 2), ref.detach())
    dx = ops.maxpool2d_bwd(parg, dout.permute(0, 2, 3, 1).contiguous().to(DEV), tuple(xcl.shape))
    np.testing.assert_allclose(dx.cpu().view(N, H, W, C).permute(0, 3, 1, 2).numpy(), xr.grad.numpy(), atol=1e-6)
    # odd extents take the per-pixel backward kernel, even ones the 2x2-block kernel: both against torch
    for (h2, w2) in ((9, 7), (8, 12)):
        x2 = torch.randint(0, 6, (2, 8, h2, w2), generator=g).float()
        x2r = x2.clone().requires_grad_()
        ref2 = F.max_pool2d(x2r, 3, 2, 1)
        d2 = ints(tuple(ref2.shape), -3, 3, 31)
        ref2.backward(d2)
        x2cl = x2.permute(0, 2, 3, 1).contiguous().view(2, 1, h2, w2, 8).to(DEV)
        o2, a2 = ops.maxpool2d_fwd(x2cl)
        assert torch.equal(o2.cpu().view(2, ref2.shape[2], ref2.shape[3], 8).permute(0, 3, 1, 2), ref2.detach())
        dx2 = ops.maxpool2d_bwd(a2, d2.permute(0, 2, 3, 1).contiguous().to(DEV), tuple(x2cl.shape))
        assert torch.equal(dx2.cpu().view(2, h2, w2, 8).permute(0, 3, 1, 2), x2r.grad)
    # BN + ReLU + max-pool in one pass == bn_act followed by the plain pool (values and winning taps)
    co = ops.bn_eval_coeffs(C, (torch.rand(C, generator=g) + 0.5).to(DEV), torch.randn(C, generator=g).to(DEV),
                            torch.full((C,), 2.5).to(DEV), torch.ones(C).to(DEV))
    z = ops.bn_act(xcl, co, relu=True)
    o1, a1 = ops.maxpool2d_fwd(z)
    o2, a2 = ops.maxpool2d_fwd(xcl, bn=co)
    assert torch.equal(o1, o2) and torch.equal(a1, a2)
    # avg-pool + view max (mv_cnn.py:29-31)
    B, V = 2, 3
    f = torch.randn(B * V, 512, 4, 4, generator=g)
    fr = f.clone().requires_grad_()
    y = F.adaptive_avg_pool2d(fr, 1).view(B, V, 512)
    refv = torch.max(y, 1)[0]
    dp = torch.randn(B, 512, generator=g)
    refv.backward(dp)
    fcl = f.permute(0, 2, 3, 1).contiguous().view(B * V, 1, 4, 4, 512).to(DEV)
    pooled, arg = ops.avgpool_viewmax_fwd(fcl, B, V)
    np.testing.assert_allclose(pooled.cpu().numpy(), refv.detach().numpy(), atol=1e-6)
    dxf = ops.avgpool_viewmax_bwd(dp.to(DEV), arg, tuple(fcl.shape), B, V)
    np.testing.assert_allclose(dxf.cpu().view(B * V, 4, 4, 512).permute(0, 3, 1, 2).numpy(), fr.grad.numpy(), atol=1e-7)
    # 12 views (config 5: more views than the kernel's 8 view slots), 16-bit storage, exact ties between views: torch.max returns
    # the FIRST maximal view and so must the argmax map (it decides which view receives the gradient)
    for store in (torch.float32, torch.float16):
        B, V, C = 3, 12, 192
        f = ints((B * V, C, 2, 2), -3, 3, 91)                      # small integers: many exact ties, sums exact in f16
        f[7], f[20], f[35] = f[2].clone(), f[13].clone(), f[24].clone()   # whole views repeated inside a shape (slots 7 / 2, 0 / 5, 3 / 0)
        y = F.adaptive_avg_pool2d(f, 1).view(B, V, C)
        refv, refi = torch.max(y, 1)
        fcl = f.permute(0, 2, 3, 1).contiguous().view(B * V, 1, 2, 2, C).to(DEV).to(store)
        pooled, arg = ops.avgpool_viewmax_fwd(fcl, B, V)
        assert torch.equal(pooled.cpu(), refv)
        first = (y == refv[:, None, :]).float().argmax(1)           # first view attaining the maximum
        assert torch.equal(arg.cpu().long(), first)


def test_layout_kernels_and_row_ops():
    from tricolo_amd.data import synthetic as syn
    batch = syn.make_batch(3, voxel_size=32, num_views=2, image_size=16, seed=77)
    locs, feats = batch["voxels"]["locs"], batch["voxels"]["feats"]
    dense, mask = ops.voxel_scatter(locs.to(DEV), feats.to(DEV), 3, 32)
    ref = torch.zeros(3, 32, 32, 32, 4)
    ref[locs[:, 0].long(), locs[:, 1].long(), locs[:, 2].long(), locs[:, 3].long(), :3] = feats
    assert torch.equal(dense.cpu(), ref)
    assert int(mask.sum().item()) == locs.shape[0]
    img = batch["images"].flatten(end_dim=1)
    out = ops.nchw3_to_nhwc4(img.to(DEV)).cpu()
    assert torch.equal(out[:, 0, :, :, :3], img.permute(0, 2, 3, 1)) and float(out[..., 3].abs().sum()) == 0.0
    g = torch.Generator().manual_seed(1)
    x = torch.randn(9, 512, generator=g)
    x[4] = 0
    xr = x.clone().requires_grad_()
    ref = F.normalize(xr, dim=1)
    dz = torch.randn(9, 512, generator=g)
    ref.backward(dz)
    z, norm = ops.l2norm_fwd(x.to(DEV))
    np.testing.assert_allclose(z.cpu().numpy(), ref.detach().numpy(), atol=1e-7)
    dx = ops.l2norm_bwd(z, norm, dz.to(DEV))
    np.testing.assert_allclose(dx.cpu()[[0, 1, 2, 3, 5, 6, 7, 8]].numpy(), xr.grad[[0, 1, 2, 3, 5, 6, 7, 8]].numpy(), rtol=1e-4, atol=1e-6)
    m = torch.randn(37, 96, generator=g)
    np.testing.assert_allclose(ops.colsum(m.to(DEV)).cpu().numpy(), m.sum(0).numpy(), atol=1e-5)


def test_adam_matches_torch_optim():
    from oracle.modules import adam_step_explicit
    g = torch.Generator().manual_seed(2)
    p = torch.randn(10007, generator=g)
    pd, m, v = p.clone().to(DEV), torch.zeros(10007, device=DEV), torch.zeros(10007, device=DEV)
    pr, mr, vr = p.clone(), torch.zeros(10007), torch.zeros(10007)
    step = torch.zeros(4, dtype=torch.int32, device=DEV)                     # [0] applied steps, [1] skipped elements, [2] flagged attempt, [3] skipped steps
    for s in range(1, 5):
        gr = torch.randn(10007, generator=g)
        ops.adam_tick(step)
        ops.adam_step(pd, gr.to(DEV), m, v, step, 3.5e-4, 0.9, 0.999, 1e-8, 1e-6)
        adam_step_explicit(pr, gr, mr, vr, s)
        np.testing.assert_allclose(pd.cpu().numpy(), pr.numpy(), atol=2e-7)
    assert step.tolist() == [4, 0, 0, 0]


def test_adam_skips_non_finite_gradient_elements():
    """Overflow guard: a gradient element that is inf / NaN - an f16 activation-gradient overflow - must not reach the fp32
    master weights or the Adam moments; the element is left alone, counted on the device, and everything else is updated as usual.
    Both update kernels: the flat one and the in-place segment reader FusedAdam uses at N = 1.  This is the per-ELEMENT fallback of the
    kernels (FusedAdam(guard=False)); the default per-step guard is test_adam_guard_skips_the_whole_step_on_a_non_finite_gradient."""
    from tricolo_amd.optim import FusedAdam
    gen = torch.Generator().manual_seed(5)
    w = [torch.nn.Parameter(torch.randn(64, 32, generator=gen).to(DEV)), torch.nn.Parameter(torch.randn(128, generator=gen).to(DEV))]
    ref = [p.detach().clone() for p in w]
    opt = FusedAdam(w, lr=1e-2, weight_decay=1e-6, guard=False)
    opt.prepare()
    for use_reduce in (False, True):                                          # segment kernel, then the packed (data-parallel) path
        before = [p.detach().clone() for p in w]
        grads = [torch.randn(p.shape, generator=gen).to(DEV) for p in w]
        grads[0][3, 5] = float("inf")
        grads[0][7, 0] = float("nan")
        grads[1][100] = float("-inf")
        for p, g_ in zip(w, grads):
            p.grad = g_
        opt.step(reduce_fn=(lambda flat: None) if use_reduce else None)
        torch.cuda.synchronize()
        for p, b_, g_ in zip(w, before, grads):
            bad = ~torch.isfinite(g_)
            assert torch.isfinite(p).all()
            assert torch.equal(p.detach()[bad], b_[bad])                       # untouched
            assert bool((p.detach()[~bad] != b_[~bad]).all())                  # everything else moved
            st = opt.state[p]
            assert torch.isfinite(st["exp_avg"]).all() and torch.isfinite(st["exp_avg_sq"]).all()
    assert opt.nonfinite_skipped() == 6 and opt.skipped_steps() == 0
    assert int(opt.state_dict()["state"][0]["step"]) == 2


@pytest.mark.parametrize("path", ["segments", "flat", "per_param", "graph"])
def test_adam_guard_skips_the_whole_step_on_a_non_finite_gradient(path):
    """Per-step overflow guard: ONE inf / NaN anywhere in a step's gradient - an f16 activation-gradient
    overflow poisons every gradient further down its tower - skips the whole optimizer step like torch.cuda.amp.GradScaler does:
    parameters, both moments and the step counter keep their values, skipped_steps() counts it, and the following healthy step is the
    step torch.optim.Adam would have taken had the bad one never happened.  All of FusedAdam's update paths: the in-place segment
    reader (N = 1), the packed flat gradient (data-parallel), the per-parameter form, and the segment path replayed from a HIP graph
    (the decision is taken on the device: the same captured graph applies one replay and skips the next)."""
    from tricolo_amd.optim import FusedAdam
    gen = torch.Generator().manual_seed(9)
    shapes = [(64, 36), (128,), (3, 3, 8)]
    init = [torch.randn(sh, generator=gen) for sh in shapes]
    w = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
    wr = [torch.nn.Parameter(t.clone()) for t in init]
    opt = FusedAdam(w, lr=1e-2, weight_decay=1e-6, flatten=path != "per_param")
    ropt = torch.optim.Adam(wr, lr=1e-2, weight_decay=1e-6)
    opt.prepare()
    kw = dict(reduce_fn=(lambda flat: None)) if path == "flat" else {}
    gbuf = [torch.zeros(sh, device=DEV) for sh in shapes]
    for p, g_ in zip(w, gbuf):
        p.grad = g_
    graph = None
    if path == "graph":
        opt.step()                                                             # warm-up on zero gradients (applied to the reference too)
        for p in wr:
            p.grad = torch.zeros_like(p)
        ropt.step()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            opt.step()
    applied0 = 1 if path == "graph" else 0
    plan = [False, True, False, True, True, False]                             # which steps carry a non-finite element
    n_bad = 0
    for i, bad in enumerate(plan):
        grads = [torch.randn(sh, generator=gen) for sh in shapes]
        before = [p.detach().clone() for p in w]
        mom = [opt.state[p]["exp_avg"].clone() for p in w]
        dirty = [g_.clone() for g_ in grads]
        if bad:
            dirty[i % 3].view(-1)[(7 * i) % dirty[i % 3].numel()] = float("inf") if i % 2 else float("nan")
            n_bad += 1
        for b_, g_ in zip(gbuf, dirty):
            b_.copy_(g_)
        if graph is not None:
            graph.replay()
        else:
            opt.step(**kw)
        torch.cuda.synchronize()
        if bad:
            for p, b_, m_ in zip(w, before, mom):
                assert torch.equal(p.detach(), b_) and torch.equal(opt.state[p]["exp_avg"], m_)
        else:
            for p, g_ in zip(wr, grads):
                p.grad = g_
            ropt.step()
            for p, r in zip(w, wr):
                np.testing.assert_allclose(p.detach().cpu().numpy(), r.detach().numpy(), atol=3e-7)
        assert opt.skipped_steps() == n_bad
    assert int(opt.state_dict()["state"][0]["step"]) == applied0 + len(plan) - n_bad
    assert opt.nonfinite_skipped() == 0                                        # the per-element fallback never saw a bad element


def test_adam_guard_record_is_reset_by_load_state_dict():
    """the guard flags ATTEMPT numbers (applied + skipped steps).  An in-process load_state_dict() back to an earlier step
    after an overflow must also reset the flag and the skip count - otherwise the stale flag sits above the restored run's attempts
    (their bad gradients fall back to the per-element guard) and the attempt that reaches it is skipped although its gradient is
    finite.  overflow -> state_dict at an early step -> more steps -> load_state_dict -> NaN step is skipped WHOLE, healthy steps apply."""
    from tricolo_amd.optim import FusedAdam
    gen = torch.Generator().manual_seed(19)
    w = [torch.nn.Parameter(torch.randn(64, 36, generator=gen).to(DEV)), torch.nn.Parameter(torch.randn(128, generator=gen).to(DEV))]
    opt = FusedAdam(w, lr=1e-2)
    opt.prepare()

    def step(bad=False):
        for p in w:
            p.grad = torch.randn(p.shape, generator=gen).to(DEV)
        if bad:
            w[0].grad.view(-1)[5] = float("nan")
        before = [p.detach().clone() for p in w]
        opt.step()
        torch.cuda.synchronize()
        return all(torch.equal(p.detach(), b_) for p, b_ in zip(w, before))     # True: the step left every parameter alone

    for _ in range(3):
        assert not step()
    early = opt.state_dict()                                                    # step 3, nothing skipped yet
    for _ in range(40):
        step()
    assert step(bad=True) and opt.skipped_steps() == 1                          # attempt 44 flagged
    for _ in range(3):
        assert not step()
    opt.load_state_dict(early)
    assert opt.skipped_steps() == 0 and int(opt.state_dict()["state"][0]["step"]) == 3
    assert not step()                                                           # attempt 4
    assert step(bad=True) and opt.skipped_steps() == 1 and opt.nonfinite_skipped() == 0     # attempt 5: skipped whole, not per element
    for _ in range(45):                                                         # runs past the old flag (attempt 44): every finite step applies
        assert not step()
    assert opt.skipped_steps() == 1 and int(opt.state_dict()["state"][0]["step"]) == 3 + 1 + 45


@pytest.mark.parametrize("tag", ["b8", "b5", "b16_sym", "b1"])
def test_ntxent_kernel_matches_reference_golden(golden, tag):
    gd = golden("ntxent")
    za, zb = torch.from_numpy(gd[f"{tag}/za"]).to(DEV), torch.from_numpy(gd[f"{tag}/zb"]).to(DEV)
    loss, dza, dzb = ops.ntxent_fwd_bwd(za, zb, float(gd[f"{tag}/T"]), float(gd[f"{tag}/alpha"]))
    assert abs(loss.item() - float(gd[f"{tag}/loss"])) < 2e-5
    np.testing.assert_allclose(dza.cpu().numpy(), gd[f"{tag}/dza"], atol=2e-6)
    np.testing.assert_allclose(dzb.cpu().numpy(), gd[f"{tag}/dzb"], atol=2e-6)
    sw, _, _ = ops.ntxent_fwd_bwd(zb, za, float(gd[f"{tag}/T"]), float(gd[f"{tag}/alpha"]), want_grad=False)
    assert abs(sw.item() - float(gd[f"{tag}/loss_swapped"])) < 2e-5


def test_ntxent_large_batch_against_float64():
    from oracle.modules import nt_xent_numpy
    g = torch.Generator().manual_seed(8)
    za, zb = torch.randn(300, 512, generator=g), torch.randn(300, 512, generator=g)
    zb[:150] += za[:150] * 2                                   # some strongly aligned pairs
    loss, dza, dzb = ops.ntxent_fwd_bwd(za.to(DEV), zb.to(DEV), 0.1, 0.25)
    l64, da, db = nt_xent_numpy(za.numpy(), zb.numpy(), 0.1, 0.25)
    assert abs(loss.item() - l64) < 2e-5
    np.testing.assert_allclose(dza.cpu().numpy(), da, atol=1e-6)
    np.testing.assert_allclose(dzb.cpu().numpy(), db, atol=1e-6)


@pytest.mark.parametrize("precision,tol", [("bf16x3", 2e-5), ("bf16", 2e-2), ("f16", 2e-3)])      # f16: single f16 products (ops.gru_mode)
@pytest.mark.parametrize("B,L", [(8, 96), (19, 7), (3, 2), (33, 13)])      # (round 6: six unrolled steps - lengths that are not multiples of 6, shorter than the prefetch depth)
def test_gru_recurrence_matches_explicit_equations(precision, tol, B, L):
    from oracle.modules import gru_explicit
    g = torch.Generator().manual_seed(3)
    xproj = torch.randn(L, B, 768, generator=g)
    w_hh = torch.randn(2, 384, 128, generator=g) / np.sqrt(128)
    b_hh = torch.randn(2, 384, generator=g) * 0.1
    xr, wr, br = xproj.clone().requires_grad_(), w_hh.clone().requires_grad_(), b_hh.clone().requires_grad_()
    # oracle: gi is given (x W_ih^T + b_ih already applied) -> use identity input weights
    finals, prevs = [], []
    for d in range(2):
        gi = xr[:, :, d * 384:(d + 1) * 384]
        h = torch.zeros(B, 128)
        steps = range(L - 1, -1, -1) if d == 1 else range(L)
        for t in steps:
            gh = h @ wr[d].t() + br[d]
            r = torch.sigmoid(gi[t, :, :128] + gh[:, :128])
            z = torch.sigmoid(gi[t, :, 128:256] + gh[:, 128:256])
            n = torch.tanh(gi[t, :, 256:] + r * gh[:, 256:])
            h = (1 - z) * n + z * h
        finals.append(h)
    ref = torch.cat(finals, dim=1)
    up = torch.randn(B, 256, generator=g)
    (ref * up).sum().backward()
    hfinal, hs, gates = ops.gru_fwd(xproj.to(DEV), w_hh.to(DEV), b_hh.to(DEV), B, L, precision)
    np.testing.assert_allclose(hfinal.cpu().numpy(), ref.detach().numpy(), atol=tol)
    dgi, dgh, hprev, dbias = ops.gru_bwd(up.to(DEV), w_hh.to(DEV), hs, gates, B, L, precision)
    db = dbias.sum(0).cpu()
    np.testing.assert_allclose(db[:, 3].numpy(), br.grad[:, 256:].numpy(), atol=tol * 50)
    np.testing.assert_allclose(db[:, :2].reshape(2, 256).numpy(), br.grad[:, :256].numpy(), atol=tol * 50)
    np.testing.assert_allclose(db[:, :3].reshape(2, 384).numpy(), xr.grad.sum((0, 1)).view(2, 384).numpy(), atol=tol * 50)
    np.testing.assert_allclose(dgi.cpu().view(L, B, 768).numpy(), xr.grad.numpy(), atol=tol * 5)
    # weight / bias gradients follow from the stored gate gradients: dW_hh = dgh^T hprev, db_hh = colsum(dgh)
    for d in range(2):
        dw = dgh[d].cpu().double().t() @ hprev[d].cpu().double()
        np.testing.assert_allclose(dw.numpy(), wr.grad[d].double().numpy(), atol=tol * 50)
        np.testing.assert_allclose(dgh[d].cpu().double().sum(0).numpy(), br.grad[d].double().numpy(), atol=tol * 50)


# ------------------------------------------------------------------------------------------- 16-bit activation storage
STORE16 = [(torch.bfloat16, "bf16"), (torch.float16, "f16")]
STORE16_IDS = ["bf16", "f16"]
BF16_CASES = [c for c in CONV_CASES if c[0] in ("vox_l0", "vox_l1", "vox_l3", "stem7x7", "c3x3s1", "c3x3s2", "c1x1s2", "odd14", "linear", "clip768")] + [
    # Cin % 64 == 0 layers run the LDS-DMA kernel in this mode; these two fill the GPU (no split-K) / use Cout % 128 != 0
    ("big_nosplit", 12, (1, 64, 64), 64, 64, (1, 3, 3), 1, (0, 1, 1), "torch"),
    ("cout192", 2, (1, 12, 12), 128, 192, (1, 3, 3), 1, (0, 1, 1), "torch"),
    # conv_halo2d_kernel geometries (2D 3x3 / 1 / pad 1): several whole images per tile with a partial last tile, 4x4 images,
    # rows that do not divide the tile (14, 20, 56 wide), two channel chunks / two output-channel tiles, a persistent
    # workgroup that walks several tiles
    ("h_8x8", 5, (1, 8, 8), 128, 128, (1, 3, 3), 1, (0, 1, 1), "torch"),
    ("h_4x4", 7, (1, 4, 4), 256, 64, (1, 3, 3), 1, (0, 1, 1), "torch"),
    ("h_14", 3, (1, 14, 14), 64, 128, (1, 3, 3), 1, (0, 1, 1), "torch"),
    ("h_28x20", 2, (1, 28, 20), 64, 64, (1, 3, 3), 1, (0, 1, 1), "torch"),
    ("h_56", 1, (1, 56, 56), 64, 64, (1, 3, 3), 1, (0, 1, 1), "torch"),
    ("h_many", 40, (1, 32, 32), 64, 64, (1, 3, 3), 1, (0, 1, 1), "torch"),
    # more tiles than CUs with four output-channel tiles and two channel chunks each (the weight stream crosses tile boundaries)
    ("h_320", 160, (1, 8, 8), 128, 256, (1, 3, 3), 1, (0, 1, 1), "torch"),
    # 192-position tiles of conv_halo_rows_kernel (planned where they save a round of workgroups: h_320 above - 216 tiles with a partial
    # last one instead of 320 - and layer3 of the bench shape: 256 tiles instead of 384, four channel chunks)
    ("h_tm3", 192, (1, 8, 8), 256, 256, (1, 3, 3), 1, (0, 1, 1), "torch"),
    # (round 5) layer3 / layer4 at 224 x 224 inputs: 14 x 14 and 7 x 7 maps, whose rows do not fill a 128- / 192-position tile - conv_dma_kernel
    # (halo tiles of 7 rows / two-three whole images, 77 % of a tile's positions, were measured: same step time, not kept)
    ("h_14x256", 24, (1, 14, 14), 256, 256, (1, 3, 3), 1, (0, 1, 1), "torch"),
    ("h_7x512", 50, (1, 7, 7), 512, 512, (1, 3, 3), 1, (0, 1, 1), "torch"),
    ("h_7x256", 5, (1, 7, 7), 256, 64, (1, 3, 3), 1, (0, 1, 1), "torch"),
    # conv_pw_kernel (1x1 / 2 shortcut convolutions; c1x1s2 above is the 64 -> 128 one): 128 -> 256 with a partial last row tile, 256 -> 512
    # (data gradient: K = 512, four rounds of activation fragments), 64-wide output-channel tiles and the 128-wide ones of a launch that fills the GPU
    ("pw_256", 7, (1, 16, 16), 128, 256, (1, 1, 1), 2, (0, 0, 0), "torch"),
    ("pw_512", 5, (1, 8, 8), 256, 512, (1, 1, 1), 2, (0, 0, 0), "torch"),
    ("pw_wide", 130, (1, 32, 32), 64, 128, (1, 1, 1), 2, (0, 0, 0), "torch"),
    # conv_stem_kernel (4 stored input channels, stride 2, 64 output channels): stem7x7 above (32 x 32 -> 16 x 16, one tile per
    # image) and: several tiles per image with a partial last one (OH = 24, TH = 8), 3x3 and 5x5 kernels, a persistent workgroup
    # that walks many tiles (more tiles than CUs), 112-wide output rows (7 position tiles per row, TH = 2)
    # conv_wgrad_c64_kernel (64 -> 64 channels, 3x3 / 1, >= 6 row tiles per CU): 8 rows of 32 per tile, and 4 rows of 56 (7 position
    # groups per tile, groups straddling image rows)
    ("c64_32", 390, (1, 32, 32), 64, 64, (1, 3, 3), 1, (0, 1, 1), "torch"),
    ("c64_56", 112, (1, 56, 56), 64, 64, (1, 3, 3), 1, (0, 1, 1), "torch"),
    ("stem_48", 2, (1, 48, 32), 3, 64, (1, 7, 7), 2, (0, 3, 3), "torch"),
    ("stem_3x3", 3, (1, 32, 64), 3, 64, (1, 3, 3), 2, (0, 1, 1), "torch"),
    ("stem_5x5", 2, (1, 20, 32), 3, 64, (1, 5, 5), 2, (0, 2, 2), "torch"),
    ("stem_many", 70, (1, 32, 32), 3, 64, (1, 7, 7), 2, (0, 3, 3), "torch"),
    ("stem_224", 1, (1, 56, 224), 3, 64, (1, 7, 7), 2, (0, 3, 3), "torch"),
    # 56-wide rows (two per tile, 112 of 128 positions used), four output-channel tiles, 7 tiles per CU
    ("h_56x4", 32, (1, 56, 56), 64, 256, (1, 3, 3), 1, (0, 1, 1), "torch"),
    # conv_c64_kernel (64 -> 64 channels, filter bank in registers; also big_nosplit and c64_32 above): 16-wide images (8 rows per brick),
    # 32-wide with 12 rows (3 bricks per image), more bricks than persistent workgroups (140 x 8 = 1,120)
    ("c64k_16", 5, (1, 16, 16), 64, 64, (1, 3, 3), 1, (0, 1, 1), "torch"),
    ("c64k_32x12", 3, (1, 12, 32), 64, 64, (1, 3, 3), 1, (0, 1, 1), "torch"),
    ("c64k_many", 140, (1, 32, 32), 64, 64, (1, 3, 3), 1, (0, 1, 1), "torch"),
    # conv_s2d_kernel (data gradient of the 64 -> 128 channel 3x3 / 2 layer, four parity classes from one slab): 16- and 32-pixel dOut rows,
    # more bricks than persistent workgroups (300 x 8 = 2,400 bricks of two rows)
    ("s2d_16", 5, (1, 32, 32), 64, 128, (1, 3, 3), 2, (0, 1, 1), "torch"),
    ("s2d_32", 2, (1, 64, 64), 64, 128, (1, 3, 3), 2, (0, 1, 1), "torch"),
    ("s2d_many", 300, (1, 32, 32), 64, 128, (1, 3, 3), 2, (0, 1, 1), "torch"),
]


@pytest.mark.parametrize("case", BF16_CASES, ids=[c[0] for c in BF16_CASES])
@pytest.mark.parametrize("store,prec", STORE16, ids=STORE16_IDS)
def test_conv_16bit_storage_integer_exact(case, store, prec):
    """The bf16 / f16 modes store activations in 16 bits: operands are exact, the fp32 accumulator is rounded once on store."""
    x, w, wp, xcl, g = make_case(case, integer=True, seed=51)
    if case[0].startswith("c64k") or case[0] in ("big_nosplit", "c64_32", "c64_56", "h_56"):
        assert (g.kernel_family[(False, 2)] & 255) == 9 and (g.kernel_family[(True, 2)] & 255) == 9      # conv_c64_kernel, both directions
    ref = cl3(F.conv3d(x, w, stride=case[6], padding=case[7]))
    packed = ops.pack_weight(wp.to(DEV), g, prec)
    out = ops.conv_fwd(xcl.to(DEV).to(store), g, packed)
    assert out.dtype == store
    assert torch.equal(out.cpu(), ref.to(store))
    # wgrad (fp32 result, exact) and dgrad (bf16 result, rounded once)
    wr = w.clone().requires_grad_()
    xr = x.clone().requires_grad_()
    y = F.conv3d(xr, wr, stride=case[6], padding=case[7])
    dy = ints(tuple(y.shape), -2, 2, 53)
    y.backward(dy)
    refw = wr.grad.permute(0, 2, 3, 4, 1).contiguous() if case[8] == "spconv" else wr.grad
    dw = ops.conv_wgrad(xcl.to(DEV).to(store), cl3(dy).to(DEV).to(store), g, wp.to(DEV), prec)
    assert torch.equal(dw.cpu(), refw)
    if case[3] != 3:
        dx = ops.conv_dgrad(cl3(dy).to(DEV).to(store), g, ops.pack_weight(wp.to(DEV), g, prec, transposed=True))
        assert torch.equal(dx.cpu(), cl3(xr.grad).to(store))
    if case[0].startswith("s2d"):
        assert (g.kernel_family[(True, 2)] & 255) == 10                  # conv_s2d_kernel
        # ... and the forward of the same layer: conv_dma_kernel (what bench.py times; the opt-in conv_s2f_kernel was dropped in round 6)
        assert (g.kernel_family[(False, 2)] & 255) == 2
        out2, stats = ops.conv_fwd(xcl.to(DEV).to(store), g, packed, want_stats=True)
        assert torch.equal(out2.cpu(), ref.to(store))
        exact = ref.to(store).double().reshape(-1, case[4])
        st = stats.cpu().double().sum(0)
        np.testing.assert_allclose(st[0].numpy(), exact.sum(0).numpy(), rtol=1e-6, atol=1e-2)
        np.testing.assert_allclose(st[1].numpy(), (exact ** 2).sum(0).numpy(), rtol=1e-6, atol=1e-2)
        tp = ops.pack_weight(wp.to(DEV), g, prec, transposed=True)
        base = ints(tuple(cl3(xr.grad).shape), -5, 5, 59)
        dx2 = ops.conv_dgrad(cl3(dy).to(DEV).to(store), g, tp, out=base.clone().to(DEV).to(store), accumulate=True)
        assert torch.equal(dx2.cpu(), (cl3(xr.grad) + base).to(store))
        for ty in ("4", "8") if case[0] == "s2d_16" else (("4",) if case[0] == "s2d_32" else ()):     # the larger bricks (batches of hundreds)
            os.environ["TRICOLO_S2D_TY"] = ty
            try:
                dx3 = ops.conv_dgrad(cl3(dy).to(DEV).to(store), g, tp)
                dx4 = ops.conv_dgrad(cl3(dy).to(DEV).to(store), g, tp, out=base.clone().to(DEV).to(store), accumulate=True)
            finally:
                del os.environ["TRICOLO_S2D_TY"]
            assert torch.equal(dx3.cpu(), cl3(xr.grad).to(store)) and torch.equal(dx4.cpu(), (cl3(xr.grad) + base).to(store))
    if case[5] == (1, 1, 1) and case[6] == 2:
        # conv_pw_kernel, both directions; BatchNorm records of the forward: one per 128-row tile
        assert (g.kernel_family[(False, 2)] & 255) == 12 and (g.kernel_family[(True, 2)] & 255) == 12
        out2, stats = ops.conv_fwd(xcl.to(DEV).to(store), g, packed, want_stats=True)
        assert torch.equal(out2.cpu(), ref.to(store)) and stats.shape[0] == g.num_mtiles[2] == (ref.numel() // case[4] + 127) // 128
        exact = ref.to(store).double().reshape(-1, case[4])
        st = stats.cpu().double().sum(0)
        np.testing.assert_allclose(st[0].numpy(), exact.sum(0).numpy(), rtol=1e-6, atol=1e-2)
        np.testing.assert_allclose(st[1].numpy(), (exact ** 2).sum(0).numpy(), rtol=1e-6, atol=1e-2)
        # the data gradient writes the whole dense tensor (zeros at the pixels the stride skips) over whatever was there
        tp = ops.pack_weight(wp.to(DEV), g, prec, transposed=True)
        dirty = torch.full(tuple(cl3(xr.grad).shape), 7.0).to(DEV).to(store)
        dx2 = ops.conv_dgrad(cl3(dy).to(DEV).to(store), g, tp, out=dirty)
        assert torch.equal(dx2.cpu(), cl3(xr.grad).to(store))
        # accumulate form (not the kernel's): conv_dma_kernel takes it
        base = ints(tuple(cl3(xr.grad).shape), -5, 5, 59)
        dx3 = ops.conv_dgrad(cl3(dy).to(DEV).to(store), g, tp, out=base.clone().to(DEV).to(store), accumulate=True)
        assert torch.equal(dx3.cpu(), (cl3(xr.grad) + base).to(store))
    if case[0].startswith("stem"):
        # one BatchNorm record per persistent workgroup of conv_stem_kernel: their sum is the whole tensor's column sum
        assert (g.kernel_family[(False, 2)] & 255) == 4
        out2, stats = ops.conv_fwd(xcl.to(DEV).to(store), g, packed, want_stats=True)
        assert torch.equal(out2.cpu(), ref.to(store)) and stats.shape[0] == g.num_mtiles[2]
        exact = ref.to(store).double().reshape(-1, case[4])
        st = stats.cpu().double().sum(0)
        np.testing.assert_allclose(st[0].numpy(), exact.sum(0).numpy(), rtol=1e-6, atol=1e-2)
        np.testing.assert_allclose(st[1].numpy(), (exact ** 2).sum(0).numpy(), rtol=1e-6, atol=1e-2)
    if case[5] == (1, 3, 3) and case[6] == 1:
        # the resolution-keeping 3x3 layers (conv_halo2d_kernel): BatchNorm partial sums of the stored values, and the
        # accumulate epilogue the residual branch of a BasicBlock uses
        out2, stats = ops.conv_fwd(xcl.to(DEV).to(store), g, packed, want_stats=True)
        assert torch.equal(out2.cpu(), ref.to(store))
        if case[0] in ("h_tm3", "h_320") and os.environ.get("TRICOLO_HALO_ROWS", "1") != "0" and os.environ.get("TRICOLO_HALO_TM3", "1") != "0":
            assert (g.kernel_family[(False, 2)] >> 8) == 3 and stats.shape[0] == (64 if case[0] == "h_tm3" else 54)   # 192-position tiles, one record per workgroup
        exact = ref.to(store).double().reshape(-1, case[4])
        st = stats.cpu().double().sum(0)
        np.testing.assert_allclose(st[0].numpy(), exact.sum(0).numpy(), rtol=1e-6, atol=1e-2)
        np.testing.assert_allclose(st[1].numpy(), (exact ** 2).sum(0).numpy(), rtol=1e-6, atol=1e-2)
        base = ints(tuple(cl3(xr.grad).shape), -5, 5, 59)
        dx2 = ops.conv_dgrad(cl3(dy).to(DEV).to(store), g, ops.pack_weight(wp.to(DEV), g, prec, transposed=True),
                             out=base.clone().to(DEV).to(store), accumulate=True)
        assert torch.equal(dx2.cpu(), (cl3(xr.grad) + base).to(store))
        # the data gradient that also takes the BatchNorm-backward sums of the pass that would read it next (tri_conv_dgrad_bn): the two
        # forms of a BasicBlock backward - relu(bn1(y)) behind conv2 (mask recomputed from y), relu(bn2(y) + x) behind the accumulated
        # conv1 gradient (mask from the saved output); a layer whose kernel has no fused form answers (dx, None)
        tp = ops.pack_weight(wp.to(DEV), g, prec, transposed=True)
        yv = ints(tuple(cl3(xr.grad).shape), -3, 3, 67)
        co = ops.BNCoeffs(case[3], DEV)
        co.scale.copy_(torch.linspace(-1.0, 1.5, case[3])); co.shift.copy_(torch.linspace(0.75, -0.5, case[3]))
        dx3, part = ops.conv_dgrad(cl3(dy).to(DEV).to(store), g, tp, bn_sums=(yv.to(DEV).to(store), co, None))
        assert torch.equal(dx3.cpu(), cl3(xr.grad).to(store))
        assert (part is not None) == ((g.kernel_family[(True, 2)] & 255) == 9 and case[2][2] <= 32)      # (conv_c64_kernel, 16- / 32-wide images)
        if part is not None:
            keep = (yv * co.scale.cpu() + co.shift.cpu() > 0).double()
            gm = cl3(xr.grad).to(store).double() * keep
            st = part.cpu().double().sum(0)
            np.testing.assert_allclose(st[0].numpy(), gm.reshape(-1, case[3]).sum(0).numpy(), rtol=1e-6, atol=1e-2)
            np.testing.assert_allclose(st[1].numpy(), (gm * yv.double()).reshape(-1, case[3]).sum(0).numpy(), rtol=1e-6, atol=1e-2)
            ro = ints(tuple(yv.shape), -1, 2, 69)
            mode, ops._DGRAD_BN_MODE = ops._DGRAD_BN_MODE, "1"               # (the accumulated form is off by default: TRICOLO_DGRAD_BN=2)
            try:
                dx4, part = ops.conv_dgrad(cl3(dy).to(DEV).to(store), g, tp, out=base.clone().to(DEV).to(store), accumulate=True,
                                           bn_sums=(yv.to(DEV).to(store), None, ro.to(DEV).to(store)))
            finally:
                ops._DGRAD_BN_MODE = mode
            assert part is not None and torch.equal(dx4.cpu(), (cl3(xr.grad) + base).to(store))
            gm = (cl3(xr.grad) + base).to(store).double() * (ro > 0).double()
            st = part.cpu().double().sum(0)
            np.testing.assert_allclose(st[0].numpy(), gm.reshape(-1, case[3]).sum(0).numpy(), rtol=1e-6, atol=1e-2)
            np.testing.assert_allclose(st[1].numpy(), (gm * yv.double()).reshape(-1, case[3]).sum(0).numpy(), rtol=1e-6, atol=1e-2)
    if case[0] in ("c64k_16", "stem_3x3", "h_8x8", "s2d_16"):
        # calls a family hands on to the generic kernel (conv_families[] `falls`): a row mask on the layers of conv_c64_kernel,
        # conv_stem_kernel, the halo kernels and conv_s2d_kernel, forward and data gradient - rows with a zero mask byte come out as zeros
        gen = torch.Generator().manual_seed(71)
        mo = (torch.rand(ref.numel() // case[4], generator=gen) < 0.6).to(torch.uint8)
        outm = ops.conv_fwd(xcl.to(DEV).to(store), g, packed, row_mask=mo.to(DEV))
        assert torch.equal(outm.cpu().reshape(-1, case[4]), (ref.reshape(-1, case[4]) * mo[:, None].float()).to(store))
        if case[3] != 3:
            mi = (torch.rand(x.numel() // case[3], generator=gen) < 0.6).to(torch.uint8)
            dxm = ops.conv_dgrad(cl3(dy).to(DEV).to(store), g, ops.pack_weight(wp.to(DEV), g, prec, transposed=True), row_mask=mi.to(DEV))
            assert torch.equal(dxm.cpu().reshape(-1, case[3]), (cl3(xr.grad).reshape(-1, case[3]) * mi[:, None].float()).to(store))
        if case[0] == "c64k_16":
            with pytest.raises(RuntimeError, match="conv_c64_kernel"):     # the layer's record count is conv_c64_kernel's: no statistics from the generic kernel
                ops.conv_fwd(xcl.to(DEV).to(store), g, packed, row_mask=mo.to(DEV), want_stats=True)


@pytest.mark.parametrize("rows", ["0", "2", "2,tm2", "2,tm2,noprod"])
def test_halo_kernels_ab_switch(rows):
    """TRICOLO_HALO_ROWS picks the kernel of the resolution-keeping 3x3 layers per plan (default: conv_halo_rows_kernel for 64 input
    channels and for launches with at most one tile per workgroup, conv_halo2d_kernel otherwise).  The switch is read once per
    process, so the two forced settings - conv_halo2d_kernel everywhere (0), the row-unit pipeline everywhere, including its
    weight-streaming multi-tile mode (2) - run the halo geometries of the exactness test above in a child process."""
    import subprocess
    import sys
    env = dict(os.environ, TRICOLO_HALO_ROWS=rows.split(",")[0])
    if "tm2" in rows:
        env["TRICOLO_HALO_TM3"] = "0"                                 # 128-position tiles only (A/B partner of the 192-position tiles)
    if "noprod" in rows:
        env["TRICOLO_HALO_PROD"] = "0"                                # every wave issues its own DMA pieces (A/B partner of the producer waves)
    k = "test_conv_16bit_storage_integer_exact and (h_ or big_nosplit or c64_32) and f16"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-k", k, "-p", "no:cacheprovider"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout


@pytest.mark.parametrize("switch", ["voxb32", "no_voxg", "no_s2g"])
def test_opt_in_kernels_child_process(switch):
    """Plans that are NOT on the default switch set keep their exactness coverage through a child process that sets the switch in its
    own environment (the parent - like bench.py - runs with no TRICOLO_* variable set, tests/conftest.py): conv_voxb_kernel on 32^3
    level-1 grids (TRICOLO_VOXB_32=1; conv_igemm_kernel is faster there); the voxel tower's coarse levels on conv_dma_kernel over compact
    row lists (TRICOLO_NO_VOXG=1, A/B partner of conv_voxg_kernel: the bench-geometry voxel test); layer4's opening layer on
    conv_dma_kernel (TRICOLO_NO_S2G=1).  Round 6 dropped the kernels that had lost their A/B for good (conv_vox1_kernel,
    conv_s2f_kernel, conv_s2g_kernel's 12-fragment variant) together with their switches."""
    import subprocess
    import sys
    env, k, f = {"voxb32": ({"TRICOLO_VOXB_32": "1"}, "test_voxel_level1_ranked_brick_kernel and 32-", __file__),
                 # conv_s2g_kernel's A/B partner: layer4's opening layer on conv_dma_kernel (the bench-geometry test of that layer)
                 "no_s2g": ({"TRICOLO_NO_S2G": "1", "TRICOLO_BENCH_PLAN_ANY_SWITCH": "1"}, "test_image_tower_bench_geometry_integer_exact and b6.conv1",
                            os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_bench_plan.py")),
                 "no_voxg": ({"TRICOLO_NO_VOXG": "1", "TRICOLO_NO_VOXB": "1", "TRICOLO_BENCH_PLAN_ANY_SWITCH": "1"},
                             "test_voxel_tower_bench_geometry_integer_exact and config4",
                             os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_bench_plan.py"))}[switch]
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(f), "-q", "-x", "-k", k, "-p", "no:cacheprovider"],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout.split("\n")[-2]


@pytest.mark.parametrize("store,prec", STORE16, ids=STORE16_IDS)
def test_conv_16bit_storage_masked_stats(store, prec):
    """Submanifold rule + BatchNorm partial sums through the LDS-DMA kernel (Cin = 64) and its split-K finish: rows with a zero mask
    byte are written as zeros whatever the input holds (a 6^3 grid: the 2^3 / 4^3 / 8^3 grids run conv_voxg_kernel, which has its
    own test - test_voxel_coarse_grid_kernel)."""
    case = ("vox_m", 3, (6, 6, 6), 64, 128, (3, 3, 3), 1, (1, 1, 1), "spconv")
    x, w, wp, xcl, g = make_case(case, integer=True, seed=61)
    assert (g.kernel_family[(False, 2)] & 255) == 2
    M = 3 * 216
    gen = torch.Generator().manual_seed(9)
    mask = (torch.rand(M, generator=gen) < 0.3).to(torch.uint8)
    mask[:256] = 0                                                  # two fully inactive 128-row tiles
    full = cl3(F.conv3d(x, w, padding=1)).reshape(M, -1)
    ref = (full * mask[:, None].float()).to(store)
    packed = ops.pack_weight(wp.to(DEV), g, prec)
    out, stats = ops.conv_fwd(xcl.to(DEV).to(store), g, packed, row_mask=mask.to(DEV), want_stats=True)
    assert torch.equal(out.cpu().reshape(M, -1), ref)
    st = stats.cpu().double().sum(0)
    exact = ref.double()                                            # statistics of what BatchNorm reads back (the stored bf16)
    np.testing.assert_allclose(st[0].numpy(), exact.sum(0).numpy(), rtol=1e-6, atol=1e-3)
    np.testing.assert_allclose(st[1].numpy(), (exact ** 2).sum(0).numpy(), rtol=1e-6, atol=1e-3)
    dy = ints((M, 128), -2, 2, 63) * mask[:, None].float()
    xr = x.clone().requires_grad_()
    wr = w.clone().requires_grad_()
    F.conv3d(xr, wr, padding=1).backward(cf3(dy.view(3, 6, 6, 6, 128)))
    dw = ops.conv_wgrad(xcl.to(DEV).to(store), dy.view(3, 6, 6, 6, 128).to(DEV).to(store), g, wp.to(DEV), prec,
                        row_mask=mask.to(DEV))                      # 64-position steps without an active site are skipped
    assert torch.equal(dw.cpu(), wr.grad.permute(0, 2, 3, 4, 1).contiguous())
    dx = ops.conv_dgrad(dy.view(3, 6, 6, 6, 128).to(DEV).to(store), g, ops.pack_weight(wp.to(DEV), g, prec, transposed=True),
                        row_mask=mask.to(DEV))
    assert torch.equal(dx.cpu().reshape(M, -1), (cl3(xr.grad).reshape(M, -1) * mask[:, None].float()).to(store))


@pytest.mark.parametrize("bf", [torch.bfloat16, torch.float16], ids=STORE16_IDS)
def test_elementwise_kernels_16bit_storage(bf):
    g = torch.Generator().manual_seed(61)
    N, H, W, C = 4, 8, 8, 64
    M = N * H * W
    y = (torch.randn(M, C, generator=g) * 2).to(bf)
    res = torch.randn(M, C, generator=g).to(bf)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    yf, rf = y.float(), res.float()
    stats = torch.stack([yf.double().sum(0).float(), (yf.double() ** 2).sum(0).float()]).view(1, 2, C)
    rm, rv, nbt = torch.zeros(C, device=DEV), torch.ones(C, device=DEV), torch.zeros((), dtype=torch.long, device=DEV)
    co = ops.bn_finalize(stats.to(DEV), C, gamma.to(DEV), beta.to(DEV), rm, rv, nbt, count_host=M)
    out = ops.bn_act(y.to(DEV), co, relu=True, res=res.to(DEV))
    assert out.dtype == bf
    mean, var = yf.mean(0), yf.var(0, unbiased=False)
    ref = F.relu((yf - mean) / torch.sqrt(var + 1e-5) * gamma + beta + rf)
    np.testing.assert_allclose(out.float().cpu().numpy(), ref.numpy(), rtol=1e-2, atol=1e-2)       # one bf16 rounding of the result
    dout = torch.randn(M, C, generator=g).to(bf)
    gz = ops.relu_bwd(dout.to(DEV), out, inplace=False)
    assert torch.equal(gz.cpu(), (dout.float() * (out.float().cpu() > 0)).to(bf))
    dy, dgamma, dbeta = ops.bn_bwd(y.to(DEV), gz, co, gamma.to(DEV), count_host=M, inplace=False)
    yr, gr, br = yf.clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    F.batch_norm(yr, None, None, gr, br, True, 0.1, 1e-5).backward(gz.float().cpu())
    np.testing.assert_allclose(dy.float().cpu().numpy(), yr.grad.numpy(), rtol=2e-2, atol=2e-2)
    np.testing.assert_allclose(dgamma.cpu().numpy(), gr.grad.numpy(), rtol=1e-3, atol=1e-2)
    np.testing.assert_allclose(dbeta.cpu().numpy(), br.grad.numpy(), rtol=1e-3, atol=1e-2)
    # max-pool 3x3/2 with ties, bf16 storage
    x = torch.randint(0, 6, (N, C, 10, 10), generator=g).float()
    xr = x.clone().requires_grad_()
    refp = F.max_pool2d(xr, 3, 2, 1)
    dp = torch.randint(-3, 4, refp.shape, generator=g).float()
    refp.backward(dp)
    xcl = x.permute(0, 2, 3, 1).contiguous().view(N, 1, 10, 10, C).to(DEV).to(bf)
    po, parg = ops.maxpool2d_fwd(xcl)
    assert torch.equal(po.float().cpu().view(N, 5, 5, C).permute(0, 3, 1, 2), refp.detach())
    dxp = ops.maxpool2d_bwd(parg, dp.permute(0, 2, 3, 1).contiguous().to(DEV).to(bf), tuple(xcl.shape))
    assert torch.equal(dxp.float().cpu().view(N, 10, 10, C).permute(0, 3, 1, 2), xr.grad)


@pytest.mark.parametrize("store,prec", [(torch.float32, "bf16x3"), (torch.float16, "f16")], ids=["bf16x3", "f16"])
def test_wgrad_grouped_reduce_is_bitwise_the_per_layer_reduce(store, prec):
    """tri_conv_wgrad_partial + ONE tri_wgrad_reduce_grouped over many layers (more than TRI_WGRAD_GROUP_MAX = 24, so the
    list is cut into two launches) against tri_conv_wgrad layer by layer: same partial kernels, same summation order."""
    names = ("vox_l0", "vox_l1", "stem7x7", "c3x3s1", "c3x3s2", "c1x1s2", "odd14", "linear", "vox_l3")
    cases = [c for c in CONV_CASES if c[0] in names]
    batch = ops.WgradBatch(torch.device(DEV), group_jobs=False)   # (shared partial launches cut the layers differently: next test)
    refs, outs = [], []
    for i in range(27):
        case = cases[i % len(cases)]
        x, w, wp, xcl, g = make_case(case, integer=False, seed=100 + i)
        gen = torch.Generator().manual_seed(500 + i)
        dy = torch.randn((g.B, *g.out_grid, g.cout), generator=gen)
        xd, dyd = xcl.to(DEV).to(store), dy.to(DEV).to(store)
        scale = 1.0 if i % 2 else 0.25
        refs.append(ops.conv_wgrad(xd, dyd, g, wp.to(DEV), prec, out_scale=scale))
        outs.append(ops.conv_wgrad(xd, dyd, g, wp.to(DEV), prec, out_scale=scale, batch=batch))
    assert len(batch.descs) == 27
    batch.flush()
    assert batch.descs == [] and batch.off == 0
    torch.cuda.synchronize()
    for i, (r, o) in enumerate(zip(refs, outs)):
        assert torch.equal(r, o), f"layer {i}: max abs diff {(r - o).abs().max().item()}"
    # the arena is reused by the next batch of the stream (same slabs, no new allocation)
    n_chunks = len(batch.chunks)
    b2 = ops.WgradBatch(torch.device(DEV))
    case = cases[3]
    x, w, wp, xcl, g = make_case(case, integer=True, seed=7)
    dy = ints((g.B, *g.out_grid, g.cout), -2, 2, 9)
    o = ops.conv_wgrad(xcl.to(DEV).to(store), dy.to(DEV).to(store), g, wp.to(DEV), prec, batch=b2)
    b2.flush()
    assert len(b2.chunks) == n_chunks and b2.chunks is batch.chunks
    assert torch.equal(o, ops.conv_wgrad(xcl.to(DEV).to(store), dy.to(DEV).to(store), g, wp.to(DEV), prec))


WGRAD_JOB_CASES = {
    # family conv_wgrad_dma_kernel<64,128>: four long 64 -> 64 layers -> 35 steps per split (the plan ring refills) ...
    "c64_ring": [("j", 48, (1, 32, 32), 64, 64, (1, 3, 3), 1, (0, 1, 1), "torch")] * 4,
    # ... <128,128>: six layers of one shape (47 steps per split, ring), and a mixed group whose jobs get different split counts
    "c128_ring": [("j", 96, (1, 16, 16), 128, 128, (1, 3, 3), 1, (0, 1, 1), "torch")] * 6,
    "mixed": [("j", 6, (1, 16, 16), 128, 128, (1, 3, 3), 1, (0, 1, 1), "torch"), ("j", 6, (1, 16, 16), 128, 256, (1, 3, 3), 2, (0, 1, 1), "torch"),
              ("j", 6, (1, 8, 8), 256, 256, (1, 3, 3), 1, (0, 1, 1), "torch"), ("j", 6, (1, 16, 16), 128, 256, (1, 1, 1), 2, (0, 0, 0), "torch"),
              ("j", 5, (1, 4, 4), 512, 512, (1, 3, 3), 1, (0, 1, 1), "torch"), ("j", 5, (1, 4, 4), 512, 512, (1, 3, 3), 1, (0, 1, 1), "torch"),
              ("j", 5, (1, 4, 4), 512, 512, (1, 3, 3), 1, (0, 1, 1), "torch"), ("j", 5, (1, 4, 4), 512, 512, (1, 3, 3), 1, (0, 1, 1), "torch"),
              ("j", 7, (1, 32, 32), 64, 64, (1, 3, 3), 1, (0, 1, 1), "torch"), ("j", 3, (1, 8, 8), 64, 64, (1, 3, 3), 1, (0, 1, 1), "torch")],
}


@pytest.mark.parametrize("store,prec", STORE16, ids=STORE16_IDS)
@pytest.mark.parametrize("group", list(WGRAD_JOB_CASES))
def test_wgrad_jobs_share_one_partial_launch(group, store, prec):
    """WgradBatch job queue -> tri_conv_wgrad_partial_group: several layers' partial kernels in ONE launch (fewer, longer splits per
    layer; gather plan through the LDS ring beyond 16 steps per split), then the grouped reduce.  Integer data: every layer's dW is
    exactly the reference's whatever the split; a family's queue launches when its tile budget is full or TRI_WGRAD_JOBS_MAX jobs wait."""
    cases = WGRAD_JOB_CASES[group]
    batch = ops.WgradBatch(torch.device(DEV), group_jobs=True)
    outs, refs, launches, queued = [], [], 0, 0
    for i, case in enumerate(cases):
        x, w, wp, xcl, g = make_case(case, integer=True, seed=300 + i)
        fam, tiles, steps = g.wgrad_group(ops._abf(torch.empty(0, dtype=store)))
        # (3: the 256-row DMA tiles, switched off; 4 / 5: the kernel-row slab kernel's 128- / 64-row tiles on the resolution-keeping and
        # stride-2 3x3 layers, 7: its 64-row tiles at stride 2; no layer is given 6)
        assert fam in (1, 2, 3, 4, 5, 7) and tiles > 0 and steps == (g.B * int(np.prod(g.out_grid)) + 63) // 64
        dy = ints((g.B, *g.out_grid, g.cout), -2, 2, 700 + i)
        xr = x.clone().requires_grad_()
        wr = w.clone().requires_grad_()
        F.conv3d(xr, wr, stride=case[6], padding=case[7]).backward(cf3(dy))
        refs.append(wr.grad)
        before = len(batch.descs)
        outs.append(ops.conv_wgrad(xcl.to(DEV).to(store), dy.to(DEV).to(store), g, wp.to(DEV), prec, out_scale=0.5 if i % 2 else 1.0, batch=batch))
        launches += len(batch.descs) > before
        queued = max(queued, len(batch.jobs))
    assert queued > 1 and len(batch.jobs) + len(batch.descs) == len(cases)
    if group == "mixed" and os.environ.get("TRICOLO_WGRAD_WIDE") != "1":
        if os.environ.get("TRICOLO_NO_KROW_WGRAD") == "1":
            # the tile budget launched the 128-row family once on the way; both families still hold jobs (one queue per family)
            assert launches == 1 and sorted(batch.queues) == [1, 2]
        else:                                       # stride-2 / 1x1 layers on the im2col families, 3x3 / 1 layers on the kernel-row ones
            assert sorted(batch.queues) == [1, 4, 5]          # (the stride-2 3x3 layer shares the stride-1 layers' launch: family 4)
    batch.flush()
    assert batch.jobs == [] and batch.descs == []
    torch.cuda.synchronize()
    for i, (o, r) in enumerate(zip(outs, refs)):
        assert torch.equal(o.cpu(), r * (0.5 if i % 2 else 1.0)), f"job {i}: max abs diff {(o.cpu() - r).abs().max().item()}"


@pytest.mark.parametrize("store,prec", STORE16[:1], ids=STORE16_IDS[:1])
def test_overflow_noted_by_the_grouped_weight_gradient_reduce(store, prec):
    """Round 6: the grouped reduce flags an inf / NaN it STORES in the optimizer's record (tri_wgrad_reduce_grouped_noted) and FusedAdam leaves
    the tensors it vouched for out of its own scan.  A conv-weight gradient that overflows inside the backward skips the whole step although
    nobody scans it; a healthy one applies (against torch.optim.Adam); a vouched-for gradient somebody modifies AFTER the reduce (its version
    counter moved) is scanned again; and a gradient that never went through the reduce is scanned as before."""
    from tricolo_amd.optim import FusedAdam
    cases = WGRAD_JOB_CASES["mixed"][:3]
    made = [make_case(c, integer=True, seed=410 + i) for i, c in enumerate(cases)]
    gen = torch.Generator().manual_seed(77)
    ws = [torch.nn.Parameter((0.01 * torch.randn(m[2].shape, generator=gen)).to(DEV)) for m in made]     # parameters in the packed layout's shape
    other = torch.nn.Parameter(torch.randn(128, generator=gen).to(DEV))
    rws = [torch.nn.Parameter(w.detach().cpu().clone()) for w in ws]
    rother = torch.nn.Parameter(other.detach().cpu().clone())
    opt = FusedAdam(ws + [other], lr=1e-2)
    ropt = torch.optim.Adam(rws + [rother], lr=1e-2)
    opt.prepare()

    def backward(poison=None):
        opt.zero_grad(set_to_none=True)
        batch = ops.WgradBatch(torch.device(DEV), group_jobs=True)
        outs = []
        for i, (case, (x, w, wp, xcl, g)) in enumerate(zip(cases, made)):
            dy = ints((g.B, *g.out_grid, g.cout), -2, 2, 900 + i).to(store)
            if poison == i:
                dy.view(-1)[11] = float("inf")
            outs.append(ops.conv_wgrad(xcl.to(DEV).to(store), dy.to(DEV), g, ws[i], prec, batch=batch))
        batch.flush()
        for w, o in zip(ws, outs):
            w.grad = o
        other.grad = torch.randn(128, generator=gen).to(DEV)
        return outs

    def step_applied():
        before = [p.detach().clone() for p in ws + [other]]
        opt.step()
        torch.cuda.synchronize()
        same = [torch.equal(p.detach(), b_) for p, b_ in zip(ws + [other], before)]
        assert all(same) or not any(same)
        return not same[0]

    # 1. healthy step: every conv gradient is vouched for, the scan list is just `other`; the update is torch's
    outs = backward()
    assert all(getattr(o, "_tri_noted", None) == (opt._step_dev.data_ptr(), o._version) for o in outs) and not hasattr(other.grad, "_tri_noted")
    for r, p in zip(rws + [rother], ws + [other]):
        r.grad = p.grad.detach().cpu().clone()
    assert step_applied()
    ropt.step()
    for p, r in zip(ws + [other], rws + [rother]):
        np.testing.assert_allclose(p.detach().cpu().numpy(), r.detach().numpy(), atol=3e-7)
    assert opt.skipped_steps() == 0
    # 2. an inf born inside the backward of layer 1: noted by the reduce, step skipped whole
    outs = backward(poison=1)
    assert not torch.isfinite(outs[1]).all() and torch.isfinite(outs[0]).all()
    assert not step_applied() and opt.skipped_steps() == 1 and opt.nonfinite_skipped() == 0
    # 3. a vouched-for gradient poked afterwards: its version moved, so it is scanned
    outs = backward()
    outs[2].view(-1)[5] = float("nan")
    assert not step_applied() and opt.skipped_steps() == 2
    # 4. a gradient the reduce never saw
    backward()
    other.grad.view(-1)[3] = float("inf")
    assert not step_applied() and opt.skipped_steps() == 3
    # 5. and the next healthy step applies
    backward()
    assert step_applied() and opt.skipped_steps() == 3 and opt.nonfinite_skipped() == 0


KROW_CASES = [
    # name, images, (1, H, W), cin, cout: every image width the kernel-row slab kernel takes, both tile heights (Cout % 128), several
    # input-channel chunks, a last step that runs past the tensor, image heights that do not divide the rows of a step
    ("k4_512", 13, (1, 4, 4), 512, 512),
    ("k8_256", 9, (1, 8, 8), 256, 256),
    ("k16_128", 7, (1, 16, 16), 128, 128),
    ("k32_64", 5, (1, 32, 32), 64, 64),
    ("k64_64_128", 2, (1, 64, 64), 64, 128),
    ("k16_128_192", 3, (1, 8, 16), 128, 192),
    ("k8_h6", 5, (1, 6, 8), 64, 64),
    ("k32_long", 40, (1, 32, 32), 64, 64),
    # widths that do not divide 64 (the 224^2 configuration: 56 / 28 / 14 / 7): steps of floor(64 / W) rows, dead tail of the tile
    ("k56_64", 2, (1, 56, 56), 64, 64),
    ("k28_128", 3, (1, 28, 28), 128, 128),
    ("k14_256", 5, (1, 14, 14), 256, 256),
    ("k7_512", 11, (1, 7, 7), 512, 512),
    ("k12_h5", 3, (1, 5, 12), 64, 128),
    # stride-2 form (first conv of layer2 / 3 / 4): grid = INPUT grid, de-interleaved slab rows
    ("s2_k16_64_128", 5, (1, 32, 32), 64, 128, 2),
    ("s2_k8_128_256", 7, (1, 16, 16), 128, 256, 2),
    ("s2_k4_256_512", 13, (1, 8, 8), 256, 512, 2),
    ("s2_k32_64_64", 2, (1, 64, 64), 64, 64, 2),
    ("s2_k8_h6", 3, (1, 12, 16), 64, 128, 2),
]


@pytest.mark.parametrize("store,prec", STORE16, ids=STORE16_IDS)
@pytest.mark.parametrize("case", KROW_CASES, ids=[c[0] for c in KROW_CASES])
def test_conv_wgrad_krow_integer_exact(case, store, prec):
    """conv_wgrad_krow_kernel (one kernel row of taps per workgroup from one input slab): dW of every geometry it takes,
    launched alone and as jobs of a shared launch (two copies with different data), bit-exact on integer data against torch's conv
    backward.  TRICOLO_NO_KROW_WGRAD=1 is the A/B partner (conv_wgrad_dma_kernel)."""
    name, N, grid, cin, cout = case[:5]
    stride = case[5] if len(case) > 5 else 1
    full = (name, N, grid, cin, cout, (1, 3, 3), stride, (0, 1, 1), "torch")
    outs, refs = [], []
    batch = ops.WgradBatch(torch.device(DEV), group_jobs=True)
    for rep in range(2):
        x, w, wp, xcl, g = make_case(full, integer=True, seed=40 + rep)
        if os.environ.get("TRICOLO_NO_KROW_WGRAD") != "1":
            assert g.wgrad_krow and g.wgrad_group(ops._abf(torch.empty(0, dtype=store)))[0] == (4 if cout % 128 == 0 else (7 if stride == 2 else 5))
        dy = ints((N, *g.out_grid, cout), -2, 2, 50 + rep)
        wr = w.clone().requires_grad_()
        F.conv3d(x, wr, stride=stride, padding=(0, 1, 1)).backward(cf3(dy))
        refs.append(wr.grad)
        xd, dyd = xcl.to(DEV).to(store), dy.to(DEV).to(store)
        if rep == 0:
            alone = ops.conv_wgrad(xd, dyd, g, wp.to(DEV), prec).cpu()
            assert torch.equal(alone, wr.grad), f"alone: max abs diff {(alone - wr.grad).abs().max().item()}"
        outs.append(ops.conv_wgrad(xd, dyd, g, wp.to(DEV), prec, out_scale=0.5 if rep else 1.0, batch=batch))
    assert len(batch.jobs) == 2
    batch.flush()
    torch.cuda.synchronize()
    for rep, (o, r) in enumerate(zip(outs, refs)):
        assert torch.equal(o.cpu(), r * (0.5 if rep else 1.0)), f"job {rep}: max abs diff {(o.cpu() - r).abs().max().item()}"


@pytest.mark.parametrize("M,B,D,norm", [(3, 32, 512, True), (3, 5, 512, True), (2, 8, 512, True), (3, 300, 512, True), (3, 7, 64, False)],
                         ids=["tri_b32", "tri_b5", "bi_b8", "tri_b300", "tri_nonorm"])
def test_ntxent_all_pairs_equals_the_pair_by_pair_loop(M, B, D, norm):
    """NTXentLoss.all_pairs (4 + 1 launches for every pair of the step, tricolo_net.py:56-63) against the per-pair calls
    (themselves pinned to the real NTXentLoss by the golden test above) and against float64: pair losses, their sum in Python's
    order, and each embedding's gradient summed over its pairs - with upstream gradients on the total AND on one pair loss.
    The per-pair calls are the M = 2 case of the same kernels: pair losses are EQUAL, and so are the gradients of the one-pair case."""
    from itertools import combinations

    from oracle.modules import nt_xent_numpy
    from tricolo_amd.loss.nt_xent import NTXentLoss
    g = torch.Generator().manual_seed(31 + B)
    zs = [torch.randn(B, D, generator=g) for _ in range(M)]
    zs[1][: B // 2] += 2 * zs[0][: B // 2]
    T, alpha = 0.1, 0.25
    loss_fn = NTXentLoss(T, alpha)
    zd = [z.to(DEV).requires_grad_() for z in zs]
    pairs, total = loss_fn.all_pairs(zd, norm=norm)
    assert len(pairs) == M * (M - 1) // 2
    zr = [z.to(DEV).requires_grad_() for z in zs]
    ref_pairs = [loss_fn(zr[a], zr[b], norm=norm) for a, b in combinations(range(M), 2)]
    ref_total = sum(ref_pairs)
    for l, r in zip(pairs, ref_pairs):
        assert l.item() == r.item()
    assert total.item() == sum(p.item() for p in [torch.tensor(x.item(), dtype=torch.float32) for x in pairs]) or \
        abs(total.item() - ref_total.item()) < 1e-5
    (total * 1.5 + pairs[0] * 0.5).backward()
    (ref_total * 1.5 + ref_pairs[0] * 0.5).backward()
    for a, b in zip(zd, zr):
        if M == 2:                                                  # upstream 1.5 + 0.5 = 2.0 on both sides
            assert torch.equal(a.grad, b.grad)
        np.testing.assert_allclose(a.grad.cpu().numpy(), b.grad.cpu().numpy(), rtol=1e-5, atol=2e-7)
    if norm:
        # float64 restatement: gradient of 1.5 * sum(pairs) + 0.5 * pair0
        acc = [np.zeros((B, D)) for _ in range(M)]
        for k, (a, b) in enumerate(combinations(range(M), 2)):
            l64, da, db = nt_xent_numpy(zs[a].numpy(), zs[b].numpy(), T, alpha)
            assert abs(pairs[k].item() - l64) < 2e-5
            wgt = 1.5 + (0.5 if k == 0 else 0.0)
            acc[a] += wgt * da
            acc[b] += wgt * db
        for m in range(M):
            np.testing.assert_allclose(zd[m].grad.cpu().numpy(), acc[m], atol=3e-6)


def test_ntxent_all_pairs_declines_shapes_outside_the_fused_range():
    from tricolo_amd.loss.nt_xent import NTXentLoss
    loss_fn = NTXentLoss(0.1, 0.25)
    assert loss_fn.all_pairs([torch.randn(600, 512, device=DEV) for _ in range(3)]) is None        # B > 512: per-pair path
    assert loss_fn.all_pairs([torch.randn(8, 512, device=DEV) for _ in range(4)]) is None          # four modalities
    assert loss_fn.all_pairs([torch.randn(8, 510, device=DEV) for _ in range(2)]) is None          # D % 4


@pytest.mark.parametrize("store", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_stem_bn_backward_from_the_pooled_gradient(store):
    """conv -> BN -> ReLU -> MaxPool2d(3,2,1) backward with the max-pool routing folded into the two BatchNorm passes
    (tri_maxpool_bn_bwd_*) against maxpool2d_bwd + bn_bwd(relu=True): integer-valued data make every sum exact, so the two
    paths must agree bit for bit; real-valued data agree up to the order of the fp32 partial sums.  Also against autograd."""
    for integer in (True, False):
        g = torch.Generator().manual_seed(21)
        N, C, H, W = 3, 64, 12, 20
        y = (ints((N, H, W, C), -4, 4, 5) if integer else torch.randn(N, H, W, C, generator=g) * 2 + 0.3)
        gamma = ints((C,), 1, 3, 6) if integer else torch.rand(C, generator=g) + 0.5
        beta = ints((C,), -2, 2, 7) if integer else torch.randn(C, generator=g) * 0.3
        yd = y.view(N, 1, H, W, C).to(DEV).to(store)
        M = N * H * W
        yf = yd.float().view(M, C)
        stats = torch.stack([yf.double().sum(0).float(), (yf.double() ** 2).sum(0).float()]).view(1, 2, C)
        co = ops.bn_finalize(stats, C, gamma.to(DEV), beta.to(DEV), None, None, None, count_host=M)
        pooled, arg = ops.maxpool2d_fwd(yd, want_arg=True, bn=co)
        dpool = (ints(tuple(pooled.shape), -3, 3, 8) if integer else torch.randn(pooled.shape, generator=g)).to(DEV).to(store)
        dz = ops.maxpool2d_bwd(arg, dpool, tuple(yd.shape))
        dy_a, dg_a, db_a = ops.bn_bwd(yd, dz.clone(), co, gamma.to(DEV), count_host=M, inplace=False, relu=True, out_scale=0.5)
        dy_b, dg_b, db_b = ops.maxpool_bn_bwd(yd, arg, dpool, co, gamma.to(DEV), out_scale=0.5)
        if integer:
            assert torch.equal(dg_a, dg_b) and torch.equal(db_a, db_b) and torch.equal(dy_a, dy_b)
        else:
            np.testing.assert_allclose(dg_a.cpu().numpy(), dg_b.cpu().numpy(), rtol=2e-5, atol=2e-5)
            np.testing.assert_allclose(db_a.cpu().numpy(), db_b.cpu().numpy(), rtol=2e-5, atol=2e-5)
            tol = 2e-5 if store == torch.float32 else 4e-3
            np.testing.assert_allclose(dy_a.float().cpu().numpy(), dy_b.float().cpu().numpy(), rtol=tol, atol=tol)
    if store == torch.float32:                                   # the real-valued case against autograd
        yr = y.permute(0, 3, 1, 2).clone().requires_grad_()
        gr, br = gamma.clone().requires_grad_(), beta.clone().requires_grad_()
        out = F.max_pool2d(F.relu(F.batch_norm(yr, None, None, gr, br, True, 0.1, 1e-5)), 3, 2, 1)
        out.backward(dpool.cpu().view(N, H // 2, W // 2, C).permute(0, 3, 1, 2))
        np.testing.assert_allclose(dy_b.cpu().view(N, H, W, C).numpy(), yr.grad.permute(0, 2, 3, 1).numpy(), atol=5e-5, rtol=1e-4)
        np.testing.assert_allclose(dg_b.cpu().numpy() * 2, gr.grad.numpy(), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("store", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("tiny_gamma", [False, True], ids=["plain", "tiny_gamma"])
def test_stem_bn_backward_sums_from_the_pooled_tensors(store, tiny_gamma):
    """tri_maxpool_bn_bwd_reduce_pooled (sums of g and g * y over WINDOWS, the winning activation recovered from the pooled output as
    (p - shift) / scale) against the sums taken from y and the tap map (tri_maxpool_bn_bwd_reduce) and against float64.  Integer data:
    every window's recovered activation is exact, the sums are equal bit for bit.  Real data: dgamma / dbeta within the storage
    type's rounding of the float64 sums.  tiny_gamma: channels with gamma = 0 or |shift| >> |gamma| take the stored y through the
    tap map (the recovery would divide by ~0) and stay as accurate as the others."""
    gen = torch.Generator().manual_seed(77)
    N, C, H, W = 3, 64, 12, 20
    M = N * H * W
    for integer in (True, False):
        y = (ints((N, H, W, C), -4, 4, 5) if integer else torch.randn(N, H, W, C, generator=gen) * 2 + 0.3)
        gamma = (ints((C,), 1, 3, 6) if integer else torch.rand(C, generator=gen) + 0.5)
        beta = (ints((C,), -2, 2, 7) if integer else torch.randn(C, generator=gen) * 0.3)
        if tiny_gamma:
            gamma[3], gamma[17], beta[17], gamma[40], beta[40] = 0.0, 1e-3, 1.5, -2e-4, 0.75
            # trained-like channels with |beta / gamma| ~ 10 (the recovery threshold must follow the storage type)
            gamma[50], beta[50], gamma[51], beta[51] = 0.1, 1.0, 0.05, -0.6
        yd = y.view(N, 1, H, W, C).to(DEV).to(store)
        yf = yd.float().view(M, C)
        if integer and not tiny_gamma:       # mean 0 / variance 1 statistics make scale = gamma, shift = beta exactly: an exact recovery
            co = ops.BNCoeffs(C, DEV)
            co.scale.copy_(gamma); co.shift.copy_(beta); co.mean.zero_(); co.invstd.fill_(1.0)
        else:
            stats = torch.stack([yf.double().sum(0).float(), (yf.double() ** 2).sum(0).float()]).view(1, 2, C)
            co = ops.bn_finalize(stats, C, gamma.to(DEV), beta.to(DEV), None, None, None, count_host=M)
        pooled, arg = ops.maxpool2d_fwd(yd, want_arg=True, bn=co)
        dpool = (ints(tuple(pooled.shape), -3, 3, 8) if integer else torch.randn(pooled.shape, generator=gen)).to(DEV).to(store)
        part_a, _ = ops._maxpool_bn_bwd_sums(yd, arg, dpool, co, gamma.to(DEV), None)
        part_b, nb = ops._maxpool_bn_bwd_sums(yd, arg, dpool, co, gamma.to(DEV), pooled)
        assert nb == ops.lib().tri_maxpool_bn_bwd_pooled_num_blocks(N, H, W) and part_b.shape[0] == nb
        sa, sb = part_a.double().sum(0).cpu(), part_b.double().sum(0).cpu()
        if integer and not tiny_gamma:
            assert torch.equal(sa, sb)
            continue
        # float64 reference of the two sums from the stored tensors
        z = F.relu(yf.double().cpu() * co.scale.double().cpu() + co.shift.double().cpu()).view(N, H, W, C).permute(0, 3, 1, 2).requires_grad_()
        F.max_pool2d(z, 3, 2, 1).backward(dpool.double().cpu().view(N, H // 2, W // 2, C).permute(0, 3, 1, 2))
        gfull = (z.grad * (z.detach() > 0)).permute(0, 2, 3, 1).reshape(M, C)
        ref = torch.stack([gfull.sum(0), (gfull * yf.double().cpu()).sum(0)])
        scale_ = float(ref.abs().max())
        eps = 2.0 ** -10 if store == torch.float16 else 2.0 ** -7
        # (the y-based form rounds the routed gradient to the storage type per position: it is the looser of the two)
        np.testing.assert_allclose(sb.numpy(), ref.numpy(), rtol=0, atol=eps * scale_)
        np.testing.assert_allclose(sa.numpy(), ref.numpy(), rtol=0, atol=4 * eps * scale_)
        # ... and channel by channel against that channel's own mass (a flat bound scaled by the largest channel hides a small one's error)
        mass = torch.stack([gfull.abs().sum(0), (gfull * yf.double().cpu()).abs().sum(0)])
        assert bool(((sb - ref).abs() <= eps * mass + 1e-6 * scale_).all()), ((sb - ref).abs() / (mass + 1e-30)).max()


@pytest.mark.parametrize("store,prec", STORE16, ids=STORE16_IDS)
@pytest.mark.parametrize("N,HW,k", [(5, 64, 7), (3, 32, 7), (2, 32, 3)])
def test_stem_weight_gradient_with_the_bn_apply_pass_folded_in(N, HW, k, store, prec):
    """ops.maxpool_bn_bwd_wgrad (tri_conv_stem_wgrad_bn: conv_stem_wgrad_kernel forms dy while it stages its dOut tile) against
    ops.maxpool_bn_bwd + ops.conv_wgrad on real-valued data: the staging computes exactly the values the apply pass stores (same routing
    order, roundings and FMA chain), so dW, dgamma and dbeta are bit-identical.  Odd image counts, both stem kernel heights in use."""
    case = ("stem", N, (1, HW, HW), 3, 64, (1, k, k), 2, (0, k // 2, k // 2), "torch")
    x, w, wp, xcl, g = make_case(case, integer=False, seed=41)
    gen = torch.Generator().manual_seed(43)
    C, H, W = 64, HW // 2, HW // 2                                    # conv output grid
    y = (torch.randn(N, 1, H, W, C, generator=gen) * 1.5 + 0.2).to(DEV).to(store)
    gamma, beta = (torch.rand(C, generator=gen) + 0.5).to(DEV), (torch.randn(C, generator=gen) * 0.3).to(DEV)
    M = N * H * W
    yf = y.float().view(M, C)
    stats = torch.stack([yf.double().sum(0).float(), (yf.double() ** 2).sum(0).float()]).view(1, 2, C)
    co = ops.bn_finalize(stats, C, gamma, beta, None, None, None, count_host=M)
    pooled, arg = ops.maxpool2d_fwd(y, want_arg=True, bn=co)
    dpool = torch.randn(pooled.shape, generator=gen).to(DEV).to(store)
    xd = xcl.to(DEV).to(store)
    dy, dg_a, db_a = ops.maxpool_bn_bwd(y, arg, dpool, co, gamma, out_scale=0.5)
    dw_a = ops.conv_wgrad(xd, dy, g, wp.to(DEV), prec, out_scale=0.5)
    dw_b, dg_b, db_b = ops.maxpool_bn_bwd_wgrad(xd, y, arg, dpool, co, gamma, g, wp.to(DEV), prec, out_scale=0.5)
    assert torch.equal(dg_a, dg_b) and torch.equal(db_a, db_b)
    assert torch.equal(dw_a, dw_b), f"max abs diff {(dw_a - dw_b).abs().max().item()} of {dw_a.abs().max().item()}"
    batch = ops.WgradBatch(torch.device(DEV))                          # and through a batch (deferred reduce)
    dw_c, _, _ = ops.maxpool_bn_bwd_wgrad(xd, y, arg, dpool, co, gamma, g, wp.to(DEV), prec, out_scale=0.5, batch=batch)
    batch.flush()
    assert torch.equal(dw_a, dw_c)
    ref = torch.nn.grad.conv2d_weight(x[:, :, 0].float(), w[:, :, 0].shape, cf3(dy.float().cpu())[:, :, 0], stride=2, padding=k // 2) * 0.5
    np.testing.assert_allclose(dw_b.cpu()[:, :, 0].numpy(), ref.numpy(), rtol=2e-2, atol=2e-2 * float(ref.abs().max()))


@pytest.mark.parametrize("store,prec", [(torch.float32, "bf16x3"), (torch.float16, "f16"), (torch.bfloat16, "bf16")], ids=["bf16x3", "f16", "bf16"])
@pytest.mark.parametrize("name", ["vox_l0", "vox_l1", "vox_m64", "vox_l3"])
def test_conv_wgrad_over_a_compact_row_list(name, store, prec):
    """Weight gradient of a submanifold layer contracted over the active sites only (row_pos / row_count from
    tri_mask_compact) == the masked weight gradient: dOut of inactive sites is zero, so both are the same sum; integer data
    make it exact.  Occupancies from empty to full, list lengths that are not multiples of the 32 / 64-position steps."""
    cases = {c[0]: c for c in CONV_CASES}
    cases["vox_m64"] = ("vox_m64", 2, (8, 8, 8), 64, 128, (3, 3, 3), 1, (1, 1, 1), "spconv")
    case = cases[name]
    x, w, wp, xcl, g = make_case(case, integer=True, seed=81)
    M = g.M
    for frac, seed in ((0.13, 1), (1.0, 2), (0.0, 3), (0.004, 4)):
        gen = torch.Generator().manual_seed(seed)
        mask = (torch.rand(M, generator=gen) < frac).to(torch.uint8)
        mpad = torch.zeros((M + 31) // 32 * 32, dtype=torch.uint8)
        mpad[:M] = mask
        dy = ints((M, g.cout), -2, 2, 83 + seed) * mask[:, None].float()
        xd = (xcl.reshape(M, -1) * 1.0).view(xcl.shape).to(DEV).to(store)
        dyd = dy.view(g.B, *g.out_grid, g.cout).to(DEV).to(store)
        ref = ops.conv_wgrad(xd, dyd, g, wp.to(DEV), prec, row_mask=mpad.to(DEV))
        rows = ops.mask_compact(mpad.to(DEV), M)
        assert int(rows[1].item()) == int(mask.sum())
        out = ops.conv_wgrad(xd, dyd, g, wp.to(DEV), prec, rows=rows)
        assert torch.equal(out, ref), f"occupancy {frac}: max abs diff {(out - ref).abs().max().item()}"
        # garbage in the rows of inactive sites must not matter: the list never visits them
        junk = dyd.clone().view(M, -1)
        junk[(mask == 0).to(DEV)] = 7.0
        out2 = ops.conv_wgrad(xd, junk.view(dyd.shape), g, wp.to(DEV), prec, rows=rows)
        assert torch.equal(out2, ref)


@pytest.mark.parametrize("store,prec", STORE16, ids=STORE16_IDS)
def test_wgrad_jobs_over_compact_row_lists(store, prec):
    """Row-list layers (the voxel tower's levels 2-4 and a long level-1-like list) through the job queue: one grouped partial launch per
    kernel family, each job contracting over its own compact list (device-side lengths, the plan ring refilled from the list for the
    long one), against the masked single-layer call.  Integer data: exact whatever the split; an empty list gives a zero gradient."""
    specs = [("l4", 40, (2, 2, 2), 256, 512, 0.9), ("l3", 40, (4, 4, 4), 128, 256, 0.45), ("l2", 40, (8, 8, 8), 64, 128, 0.25),
             ("l2e", 3, (8, 8, 8), 64, 128, 0.0), ("long", 48, (16, 16, 16), 64, 128, 0.6), ("l1", 24, (16, 16, 16), 32, 64, 0.2)]
    batch = ops.WgradBatch(torch.device(DEV), group_jobs=True)
    outs, refs = [], []
    for i, (name, B, grid, cin, cout, frac) in enumerate(specs):
        case = (name, B, grid, cin, cout, (3, 3, 3), 1, (1, 1, 1), "spconv")
        x, w, wp, xcl, g = make_case(case, integer=True, seed=400 + i)
        M = g.M
        gen = torch.Generator().manual_seed(450 + i)
        mask = (torch.rand(M, generator=gen) < frac).to(torch.uint8)
        mpad = torch.zeros((M + 31) // 32 * 32, dtype=torch.uint8)
        mpad[:M] = mask
        dy = (ints((M, cout), -2, 2, 470 + i) * mask[:, None].float()).sign()      # {-1, 0, 1}: sums stay exact over the long list
        xd, dyd = xcl.sign().to(DEV).to(store), dy.view(B, *g.out_grid, cout).to(DEV).to(store)
        refs.append(ops.conv_wgrad(xd, dyd, g, wp.to(DEV), prec, row_mask=mpad.to(DEV)))
        rows = ops.mask_compact(mpad.to(DEV), M)
        junk = dyd.clone().view(M, -1)
        junk[(mask == 0).to(DEV)] = 7.0                              # rows of inactive sites are never visited
        outs.append(ops.conv_wgrad(xd, junk.view(dyd.shape), g, wp.to(DEV), prec, rows=rows, batch=batch))
    assert len(batch.jobs) + len(batch.descs) == len(specs) and len(batch.jobs) >= 2
    batch.flush()
    torch.cuda.synchronize()
    for (name, *_), o, r in zip(specs, outs, refs):
        assert torch.equal(o, r), f"{name}: max abs diff {(o - r).abs().max().item()}"
    assert float(outs[3].abs().max()) == 0.0


def _blob_mask(B, V, seed, p_empty=0.3):
    """Site mask [B, V, V, V] of solid blobs (a box and an ellipsoid per sample, like the synthetic voxel grids), some samples empty:
    whole bricks and whole x-runs without an active site, runs cut by a blob boundary, sites on the grid faces."""
    g = torch.Generator().manual_seed(seed)
    zz, yy, xx = torch.meshgrid(torch.arange(V), torch.arange(V), torch.arange(V), indexing="ij")
    m = torch.zeros(B, V, V, V, dtype=torch.bool)
    for b in range(B):
        if b > 0 and torch.rand((), generator=g) < p_empty:
            continue
        lo = torch.randint(0, V // 2, (3,), generator=g)
        hi = lo + torch.randint(2, V // 2 + 1, (3,), generator=g)
        m[b] |= (zz >= lo[0]) & (zz < hi[0]) & (yy >= lo[1]) & (yy < hi[1]) & (xx >= lo[2]) & (xx < hi[2])
        c = torch.randint(0, V, (3,), generator=g).float()
        r = torch.randint(2, max(V // 3, 3), (3,), generator=g).float()
        m[b] |= ((zz - c[0]) / r[0]) ** 2 + ((yy - c[1]) / r[1]) ** 2 + ((xx - c[2]) / r[2]) ** 2 <= 1.0
    m[0, 0, 0, 0] = True                                           # a corner site: every out-of-grid tap direction at once
    m[0, V - 1, V - 1, V - 1] = True
    return m


@pytest.mark.parametrize("store,prec", STORE16, ids=STORE16_IDS)
@pytest.mark.parametrize("B,V", [(3, 32), (2, 64)])
def test_voxel_level0_brick_kernel(B, V, store, prec):
    """conv_vox0_kernel (conv_vox.hip): level 0 of the voxel tower (sparse_cnn.py:12, 3 -> 32 channels) over the dense grid by the
    site mask.  Integer data: every active row equals the masked dense convolution exactly, rows of inactive sites are not written,
    the BatchNorm records (one per workgroup) sum to the column sums of the active rows; and without a mask it is the plain conv."""
    case = ("vox0", B, (V, V, V), 3, 32, (3, 3, 3), 1, (1, 1, 1), "spconv")
    x, w, wp, xcl, g = make_case(case, integer=True, seed=71)
    assert g.brick(False, 2), "level-0 geometry should plan the brick kernel in the 16-bit modes"
    m = _blob_mask(B, V, seed=73)
    mf = m.float()
    x = x * mf[:, None]                                             # submanifold invariant: inactive sites are exactly zero
    xcl = xcl * mf[..., None]
    ref = cl3(F.conv3d(x, w, padding=1)).to(store)
    packed = ops.pack_weight(wp.to(DEV), g, prec)
    M = B * V ** 3
    mask = m.reshape(M).to(torch.uint8)
    junk = torch.full((B, V, V, V, 32), 777.0, dtype=store, device=DEV)
    out, stats = ops.conv_fwd(xcl.to(DEV).to(store), g, packed, row_mask=mask.to(DEV), want_stats=True, out=junk)
    assert stats.shape[0] == g.num_mtiles[2]
    o = out.cpu().reshape(M, 32)
    act = mask.bool()
    assert torch.equal(o[act], ref.reshape(M, 32)[act])
    assert bool((o[~act] == 777.0).all()), "rows of inactive sites must not be written"
    exact = ref.reshape(M, 32)[act].double()
    st = stats.cpu().double().sum(0)
    np.testing.assert_allclose(st[0].numpy(), exact.sum(0).numpy(), rtol=1e-6, atol=1e-2)
    np.testing.assert_allclose(st[1].numpy(), (exact ** 2).sum(0).numpy(), rtol=1e-6, atol=1e-2)
    if B * V ** 3 <= 3 * 32 ** 3:                                   # no mask: every site active (the dense convolution)
        xd, _, _, xdcl, _ = make_case(case, integer=True, seed=79)
        out2 = ops.conv_fwd(xdcl.to(DEV).to(store), g, packed)
        assert torch.equal(out2.cpu(), cl3(F.conv3d(xd, w, padding=1)).to(store))
    with pytest.raises(RuntimeError):                               # a compact row list is refused (the kernel walks the grid by the mask)
        ops.conv_fwd(xcl.to(DEV).to(store), g, packed, rows=ops.mask_compact(mask.to(DEV), M))


@pytest.mark.parametrize("store,prec", STORE16, ids=STORE16_IDS)
@pytest.mark.parametrize("B,V", [(3, 32), (30, 32), (2, 64)])
def test_voxel_level0_weight_gradient_brick_kernel(B, V, store, prec):
    """conv_vox0_wgrad_kernel (conv_vox.hip): dW of level 0 (sparse_cnn.py:12, 3 -> 32 channels) contracted over the active sites of
    the dense grid - both operands read transposed from LDS, kernel rows padded to 4 taps in the per-workgroup slabs (kw_shift = 2 in
    the reduce).  Integer data: exactly the weight gradient of the masked dense convolution, whatever lies in dOut's inactive rows;
    B = 30: more bricks than persistent workgroups x 1 ... x 2; with and without a WgradBatch; an all-inactive mask gives zeros."""
    case = ("vox0", B, (V, V, V), 3, 32, (3, 3, 3), 1, (1, 1, 1), "spconv")
    x, w, wp, xcl, g = make_case(case, integer=True, seed=171)
    assert g.wgrad_brick
    m = _blob_mask(B, V, seed=173)
    mf = m.float()
    x = (x * mf[:, None]).sign()
    xcl = (xcl * mf[..., None]).sign()
    M = B * V ** 3
    mask = torch.zeros((M + 31) // 32 * 32, dtype=torch.uint8)
    mask[:M] = m.reshape(M).to(torch.uint8)
    dy = ints((B, V, V, V, 32), -1, 1, 175) * mf[..., None]
    xr, wr = x.clone().requires_grad_(), w.clone().requires_grad_()
    F.conv3d(xr, wr, padding=1).backward(cf3(dy))
    ref = wr.grad.permute(0, 2, 3, 4, 1).contiguous()               # spconv layout [Cout, kd, kh, kw, Cin]
    assert float(ref.abs().max()) < 2 ** 24
    junk = dy.clone().view(M, 32)
    junk[~m.reshape(M)] = 9.0                                       # rows of inactive sites are never read
    xd, dyd = xcl.to(DEV).to(store), junk.view(B, V, V, V, 32).to(DEV).to(store)
    out = ops.conv_wgrad(xd, dyd, g, wp.to(DEV), prec, row_mask=mask.to(DEV), out_scale=0.5)
    assert torch.equal(out.cpu(), ref * 0.5), f"max abs diff {(out.cpu() - ref * 0.5).abs().max().item()}"
    batch = ops.WgradBatch(torch.device(DEV))
    out2 = ops.conv_wgrad(xd, dyd, g, wp.to(DEV), prec, row_mask=mask.to(DEV), batch=batch)
    batch.flush()
    assert torch.equal(out2.cpu(), ref)
    out3 = ops.conv_wgrad(xd, dyd, g, wp.to(DEV), prec, row_mask=torch.zeros_like(mask).to(DEV))
    assert float(out3.abs().max()) == 0.0


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("store,prec", STORE16, ids=STORE16_IDS)
@pytest.mark.parametrize("B,V", [(5, 16), (40, 16), (90, 16), (3, 32), (18, 32)])
def test_voxel_level1_ranked_brick_kernel(B, V, store, prec):
    """conv_voxb_kernel (conv_voxg.hip): level 1 of the voxel tower (sparse_cnn.py:17, 32 -> 64 channels) on 16^3 and 32^3 grids - bricks of
    256 sites, the active interior sites ranked in the kernel as MFMA rows, the active region sites loaded into a zero-padded slab and
    cleared again, filter bank stationary in registers, persistent workgroups (B = 40 / 18: several bricks per workgroup).  Integer data:
    active rows equal the masked dense convolution exactly whatever the input holds at inactive sites, rows of inactive sites stay
    unwritten, the per-workgroup BatchNorm records sum to the active rows' column sums; without a mask it is the plain convolution
    (256 rows per brick: two passes of eight tiles)."""
    if V == 32 and os.environ.get("TRICOLO_VOXB_32") != "1":
        pytest.skip("32^3 level-1 grids run conv_igemm_kernel by default: conv_voxb_kernel there is covered by test_opt_in_kernels_child_process[voxb32]")
    case = ("vox1", B, (V, V, V), 32, 64, (3, 3, 3), 1, (1, 1, 1), "spconv")
    x, w, wp, xcl, g = make_case(case, integer=True, seed=81)
    assert g.brick(False, 2) and (g.kernel_family[(False, 2)] & 255) == 14
    m = _blob_mask(B, V, seed=83)
    mf = m.float()
    xm = x * mf[:, None]
    ref = cl3(F.conv3d(xm, w, padding=1)).to(store)
    packed = ops.pack_weight(wp.to(DEV), g, prec)
    M = B * V ** 3
    mask = m.reshape(M).to(torch.uint8)
    act = mask.bool()
    dirty = xcl.clone().reshape(M, 32)
    dirty[~act] = 3.0                                               # never read
    junk = torch.full((B, V, V, V, 64), 777.0, dtype=store, device=DEV)
    out, stats = ops.conv_fwd(dirty.view(B, V, V, V, 32).to(DEV).to(store), g, packed, row_mask=mask.to(DEV), want_stats=True, out=junk)
    assert stats.shape[0] == g.num_mtiles[2]
    o = out.cpu().reshape(M, 64)
    assert torch.equal(o[act], ref.reshape(M, 64)[act]), f"max abs diff {(o[act].float() - ref.reshape(M, 64)[act].float()).abs().max().item()}"
    assert bool((o[~act] == 777.0).all()), "rows of inactive sites must not be written"
    exact = ref.reshape(M, 64)[act].double()
    st = stats.cpu().double().sum(0)
    np.testing.assert_allclose(st[0].numpy(), exact.sum(0).numpy(), rtol=1e-6, atol=1e-2)
    np.testing.assert_allclose(st[1].numpy(), (exact ** 2).sum(0).numpy(), rtol=1e-6, atol=1e-2)
    if B <= 5:
        out2 = ops.conv_fwd(xcl.to(DEV).to(store), g, packed)
        assert torch.equal(out2.cpu(), cl3(F.conv3d(x, w, padding=1)).to(store))
    with pytest.raises(RuntimeError, match="conv_voxb_kernel"):               # a compact row list is refused (the kernel walks the grid by the mask)
        ops.conv_fwd(xcl.to(DEV).to(store), g, packed, rows=ops.mask_compact(mask.to(DEV), M))


VOXG_CASES = [
    # B, D, cin, cout: the bench shapes' levels 2-4 (32^3 x 32), config 2 (x 64), config 5's levels 3-4, small batches (fewer workgroups than
    # CUs, partial last unit), odd batch sizes
    (32, 8, 64, 128), (32, 4, 128, 256), (32, 2, 256, 512),
    (64, 8, 64, 128), (64, 2, 256, 512),
    (64, 8, 128, 256), (64, 4, 256, 512),
    (3, 8, 64, 128), (5, 4, 128, 256), (7, 2, 256, 512), (1, 2, 64, 64),
]


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("store,prec", STORE16, ids=STORE16_IDS)
@pytest.mark.parametrize("B,D,cin,cout", VOXG_CASES, ids=[f"B{c[0]}_D{c[1]}_{c[2]}to{c[3]}" for c in VOXG_CASES])
def test_voxel_coarse_grid_kernel(B, D, cin, cout, store, prec):
    """conv_voxg_kernel (conv_voxg.hip): SubMConv3d on 2^3 / 4^3 / 8^3 grids (sparse_cnn.py:22-32) - a unit of whole samples staged in a
    zero-padded LDS slab, the unit's active sites ranked in the kernel and gathered from the slab as MFMA rows, weights straight into
    registers.  Integer data: active rows equal the masked dense convolution exactly, rows of inactive sites stay unwritten (and whatever
    the input holds at inactive sites is ignored), the per-unit BatchNorm records sum to the active rows' column sums; the data gradient
    (mirrored taps, transposed operand) equals autograd's at the active sites; every site active (512 rows per 8^3 sample: three passes)
    is the plain convolution; an all-inactive mask writes nothing and zero statistics."""
    case = ("voxg", B, (D, D, D), cin, cout, (3, 3, 3), 1, (1, 1, 1), "spconv")
    x, w, wp, xcl, g = make_case(case, integer=True, seed=181)
    assert g.brick(False, 2) and (g.kernel_family[(False, 2)] & 255) == 13 and (g.kernel_family[(True, 2)] & 255) == 13
    m = _blob_mask(B, D, seed=183 + D, p_empty=0.15) if D > 2 else (torch.rand(B, D, D, D, generator=torch.Generator().manual_seed(7)) < 0.9)
    mf = m.float()
    M = B * D ** 3
    mask = torch.zeros((M + 31) // 32 * 32, dtype=torch.uint8)
    mask[:M] = m.reshape(M).to(torch.uint8)
    act = m.reshape(M)
    xm = x * mf[:, None]
    ref = cl3(F.conv3d(xm, w, padding=1)).to(store).reshape(M, cout)
    packed = ops.pack_weight(wp.to(DEV), g, prec)
    dirty = xcl.clone().reshape(M, cin)
    dirty[~act] = 5.0                                               # inactive input rows are never used, whatever they hold
    junk = torch.full((B, D, D, D, cout), 777.0, dtype=store, device=DEV)
    out, stats = ops.conv_fwd(dirty.view(B, D, D, D, cin).to(DEV).to(store), g, packed, row_mask=mask.to(DEV), want_stats=True, out=junk)
    assert stats.shape[0] == g.num_mtiles[2]
    o = out.cpu().reshape(M, cout)
    assert torch.equal(o[act], ref[act]), f"max abs diff {(o[act].float() - ref[act].float()).abs().max().item()}"
    assert bool((o[~act] == 777.0).all()), "rows of inactive sites must not be written"
    exact = ref[act].double()
    st = stats.cpu().double().sum(0)
    np.testing.assert_allclose(st[0].numpy(), exact.sum(0).numpy(), rtol=1e-6, atol=1e-2)
    np.testing.assert_allclose(st[1].numpy(), (exact ** 2).sum(0).numpy(), rtol=1e-6, atol=1e-2)
    # data gradient at the active sites (what SparseCNNEncoder._backward_impl asks for)
    dy = ints((B, D, D, D, cout), -2, 2, 185) * mf[..., None]
    xr = xm.clone().requires_grad_()
    F.conv3d(xr, w, padding=1).backward(cf3(dy))
    refdx = cl3(xr.grad).to(store).reshape(M, cin)
    dyd = dy.clone().reshape(M, cout)
    dyd[~act] = -3.0
    junk2 = torch.full((B, D, D, D, cin), 555.0, dtype=store, device=DEV)
    dx = ops.conv_dgrad(dyd.view(B, D, D, D, cout).to(DEV).to(store), g, ops.pack_weight(wp.to(DEV), g, prec, transposed=True),
                        row_mask=mask.to(DEV), out=junk2)
    dxc = dx.cpu().reshape(M, cin)
    assert torch.equal(dxc[act], refdx[act]) and bool((dxc[~act] == 555.0).all())
    with pytest.raises(RuntimeError):                               # a compact row list is refused (the kernel walks the grid by the mask)
        ops.conv_fwd(xcl.to(DEV).to(store), g, packed, rows=ops.mask_compact(mask.to(DEV), M))
    if B <= 7:
        out2, stats2 = ops.conv_fwd(xcl.to(DEV).to(store), g, packed, want_stats=True)      # no mask: every site active
        full = cl3(F.conv3d(x, w, padding=1)).to(store)
        assert torch.equal(out2.cpu(), full)
        np.testing.assert_allclose(stats2.cpu().double().sum(0)[0].numpy(), full.double().reshape(M, cout).sum(0).numpy(), rtol=1e-6, atol=1e-2)
        junk3 = torch.full((B, D, D, D, cout), 777.0, dtype=store, device=DEV)
        out3, stats3 = ops.conv_fwd(xcl.to(DEV).to(store), g, packed, row_mask=torch.zeros_like(mask).to(DEV), want_stats=True, out=junk3)
        assert bool((out3 == 777.0).all()) and float(stats3.abs().max()) == 0.0


def test_packed_operand_order_is_checked():
    """conv_voxg_kernel / conv_voxb_kernel read FRAGMENT-MAJOR packed operands, every other kernel row-major ones; the C entry points cannot
    tell which order a buffer is in, so the Python layer tags the buffers (pack_weight's `storage` selects the plan mode) and conv_fwd /
    conv_dgrad refuse an operand packed for another plan instead of computing garbage."""
    case = ("voxg", 2, (4, 4, 4), 128, 256, (3, 3, 3), 1, (1, 1, 1), "spconv")
    x, w, wp, xcl, g = make_case(case, integer=True, seed=5)
    assert g.packed_frag(False, "f16") == 1 and g.packed_frag(False, "f16", storage=torch.float32) == 0 and g.packed_frag(False, "bf16x3") == 0
    p16 = ops.pack_weight(wp.to(DEV), g, "f16")                      # fragment-major (16-bit storage -> conv_voxg_kernel)
    p32 = ops.pack_weight(wp.to(DEV), g, "bf16", storage=torch.float32)      # row-major (fp32 storage -> conv_igemm_kernel)
    assert p16[0].tri_frag == 1 and p32[0].tri_frag == 0
    ref = cl3(F.conv3d(x, w, padding=1))
    assert torch.equal(ops.conv_fwd(xcl.to(DEV), g, p32).cpu(), ref)
    assert torch.equal(ops.conv_fwd(xcl.to(DEV).half(), g, p16).cpu(), ref.half())
    with pytest.raises(RuntimeError, match="ordered for another plan"):
        ops.conv_fwd(xcl.to(DEV), g, p16)
    with pytest.raises(RuntimeError, match="ordered for another plan"):
        ops.conv_fwd(xcl.to(DEV).half(), g, (p32[0].half(), None))
    # the batched packer picks the same order as the single-layer call
    packer = ops.WeightPacker()
    packer.add("f", wp.to(DEV), g)
    packer.add("t", wp.to(DEV), g, transposed=True)
    bufs = packer.run("f16", torch.device(DEV))
    assert bufs["f"][0].tri_frag == 1 and torch.equal(bufs["f"][0], p16[0])
    assert torch.equal(bufs["t"][0], ops.pack_weight(wp.to(DEV), g, "f16", transposed=True)[0])


S2G_CASES = [  # (N, H, W, cin, cout): 3x3 / 2 / pad 1 layers conv_s2g_kernel takes by default (>= 128 input channels, <= 16 outputs per image)
    (192, 8, 8, 256, 512),        # layer4[0].conv1 at the bench shape: units of 6 images = 96 rows, 256 workgroups
    (384, 8, 8, 256, 512),        # config-3 batch
    (7, 8, 8, 128, 64),           # an odd batch, one channel tile (the plan halves down to one image per unit here: a short last unit
                                  # needs >= 256 units x channel tiles - tests/test_gpu_guard_bands.py s2g_31x4x4_short_unit)
    (5, 8, 4, 128, 128),          # a non-square map; units of 1-2 images after the halving (few images)
    (2, 4, 4, 192, 64),           # 2x2 outputs per image, 6 chunks
]


@pytest.mark.parametrize("case", S2G_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}_{c[3]}to{c[4]}" for c in S2G_CASES])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_stride2_slab_kernel(case, dtype):
    """conv_s2g_kernel (family 15): forward of the 3x3 / 2 layers that open layer3 / layer4 - space-to-depth LDS slab, weights straight into
    MFMA registers (fragment-major operand), BatchNorm records per unit of images.  Integer-exact against F.conv2d, statistics against the
    stored values; partial last units, every unit size the plan picks, both 16-bit storage types."""
    N, H, W, cin, cout = case
    prec = "f16" if dtype == torch.float16 else "bf16"
    g = ops.ConvGeom(N, (1, H, W), cin, cin, cout, (1, 3, 3), 2, (0, 1, 1), (cin * 9, 1, 9))
    assert (g.kernel_family[(False, 2)] & 255) == 15, "plan: not conv_s2g_kernel"
    assert (g.kernel_family[(True, 2)] & 255) != 15                            # the data gradient keeps its own kernels
    x = ints((N, cin, H, W), -2, 2, 71)
    w = ints((cout, cin, 3, 3), -2, 2, 72)
    ref = F.conv2d(x, w, stride=2, padding=1).permute(0, 2, 3, 1).contiguous()
    xd = x.permute(0, 2, 3, 1).contiguous().view(N, 1, H, W, cin).to(DEV).to(dtype)
    packed = ops.pack_weight(w.to(DEV), g, prec)
    assert packed[0].tri_frag == 1
    junk = torch.full((N, 1, H // 2, W // 2, cout), 777.0, dtype=dtype, device=DEV)
    out, stats = ops.conv_fwd(xd, g, packed, want_stats=True, out=junk)
    assert torch.equal(out.cpu().view(ref.shape).float(), ref.to(dtype).float()), f"{ops._igemm_symbol(g, False, False, xd)}: forward differs"
    exact = ref.to(dtype).double().reshape(-1, cout)
    st = stats.cpu().double().sum(0)
    np.testing.assert_allclose(st[0].numpy(), exact.sum(0).numpy(), rtol=1e-6, atol=1e-1)
    np.testing.assert_allclose(st[1].numpy(), (exact ** 2).sum(0).numpy(), rtol=1e-6, atol=1e-1)
    with pytest.raises(RuntimeError, match="conv_s2g_kernel"):                 # no bias / activation epilogue on this kernel
        ops.conv_fwd(xd, g, packed, bias=torch.zeros(cout, device=DEV), act=1)
    # fp32 activations (the bf16x3 parity mode) never take this kernel: row-major operand, generic plan
    assert (g.kernel_family[(False, 1)] & 255) != 15 and (g.kernel_family[(False, 0)] & 255) != 15


@pytest.mark.parametrize("form", [0, 1, 2, 3], ids=["load_voffset", "load_soffset", "store_voffset", "store_soffset"])
def test_raw_buffer_b128_builtins_toolchain_probe(form):
    """Toolchain regression probe: `__builtin_amdgcn_raw_buffer_load_b128` / `store_b128` on random data, 16 bytes per
    lane, registers reused right behind every access (csrc/misc.hip buffer_b128_probe_kernel through the C ABI).  Form 0 - per-lane
    offset, scalar offset 0 - is what the 16 load sites of the conv kernels use and MUST be exact.  The scalar-offset forms and the 16-byte
    store are what miscompiled inside gru.hip on ROCm 7.2 (profiles/r5/NOTES_voxel.md) and are used nowhere in the library: they are
    reported (xfail when wrong), so a toolchain bump that fixes - or breaks - a form shows up here before it reaches a kernel."""
    from tricolo_amd._C import lib
    n16 = 800_000 + 37                                              # not a multiple of the 1024-element workgroup tile
    g = torch.Generator().manual_seed(1234 + form)
    src = torch.randint(-2 ** 31, 2 ** 31 - 1, (n16, 4), generator=g, dtype=torch.int64).to(torch.int32).to(DEV)
    bad_runs = 0
    for rep in range(4):                                            # (the gru.hip failure moved between runs)
        dst = torch.full_like(src, 0x5A5A5A5A)
        rc = lib().tri_debug_buffer_b128_probe(src.data_ptr(), dst.data_ptr(), n16, form, torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        bad = int((dst != src).any(dim=1).sum().item())
        bad_runs += bad > 0
        if form == 0:
            assert bad == 0, f"raw_buffer_load_b128(voffset, soffset 0): {bad} of {n16} 16-byte elements differ - the form every conv kernel uses"
    if form != 0 and bad_runs:
        pytest.xfail(f"form {form}: wrong elements in {bad_runs} of 4 runs on this toolchain (known hazard, form unused in the library)")
