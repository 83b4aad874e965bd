"""tests/bn_reference.py is neither wrong nor vacuous: an fp32 torch emulation of the three-pass BatchNorm scheme (fp32 (sum, sum of
squares) records of 128 rows summed in double, fp32 coefficient vectors, fp32 elementwise passes, fp32 per-block backward sums summed in
double) passes every bound in the three storage types, and eight mutations of it are rejected.  No GPU."""
import pytest
import torch

from tests import bn_reference as R

STORES = [torch.float32, torch.float16, torch.bfloat16]
MUTATIONS = ["unbiased_count", "mean_g_dropped", "mask_ge", "last_row_left_out", "eps_1e-3", "dbeta_unscaled", "inactive_rows_counted",
             "neighbour_scale"]
# In 16-bit storage a mutation whose effect is below the store's rounding cannot fail.  These must fail there too:
MUST_FAIL_16 = {"mask_ge", "last_row_left_out", "eps_1e-3", "dbeta_unscaled", "neighbour_scale"}
OUT_SCALE = 0.5


def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()          # the product is exact in double: one rounding, as v_fma_f32


def _bnb_rows(M):
    if M <= 16384:
        return 16
    if M <= 32768:
        return 32
    if M < 65536:
        return 64
    return max(256, ((M + 2047) // 2048 + 63) // 64 * 64)


def _block_sums(t, rows):
    """fp32 sums over blocks of `rows` rows, then the records in double."""
    M, C = t.shape
    pad = (M + rows - 1) // rows * rows
    tp = torch.zeros(pad, C, dtype=torch.float32)
    tp[:M] = t
    return tp.reshape(-1, rows, C).sum(1, dtype=torch.float32).double().sum(0)


def emulate(inp, mode, mut=None, rm=None, rv=None):
    """The scheme of bn_pool.hip in fp32 torch.  -> namespace co (mean, invstd, scale, shift fp32), out, dy, dgamma, dbeta, g_masked,
    running_mean, running_var; inactive rows of dy zero."""
    M, C, store = inp.M, inp.C, inp.store
    live = inp.rows[:M].bool() if inp.rows is not None else torch.ones(M, dtype=torch.bool)
    n_live = int(live.sum())
    n = float(M if mut == "inactive_rows_counted" else n_live)
    y = torch.where(live[:, None], inp.y.float(), torch.zeros(()))
    g = torch.where(live[:, None], inp.g.float(), torch.zeros(()))
    ga, be = inp.gamma.double(), inp.beta.double()
    s, q = _block_sums(y, 128), _block_sums(y * y, 128)
    mean = s / n
    var = torch.clamp(q / n - mean * mean, min=0.0)
    invstd = 1.0 / torch.sqrt(var + (1e-3 if mut == "eps_1e-3" else float(torch.tensor(1e-5, dtype=torch.float32))))
    o = R.SimpleNamespace()
    o.co = R.SimpleNamespace(mean=mean.float(), invstd=invstd.float(), scale=(ga * invstd).float(), shift=(be - mean * ga * invstd).float())
    if rm is not None:
        unb = var * n / (n - 1) if n > 1 else var
        o.running_mean, o.running_var = (0.9 * rm.double() + 0.1 * mean).float(), (0.9 * rv.double() + 0.1 * unb).float()
    scale = o.co.scale.clone()
    if mut == "neighbour_scale":
        scale[10] = scale[9]
    pre = _fma(y, scale, o.co.shift)
    if mode == "relu_out":
        pre = pre + inp.res.float()
    o.out = torch.relu(pre).to(store)
    if mode == "relu":
        z = _fma(y, o.co.scale, o.co.shift)
        gm = torch.where((z >= 0) if mut == "mask_ge" else (z > 0), g, torch.zeros(()))
    elif mode == "relu_out":
        gm = torch.where(o.out.float() > 0, g, torch.zeros(()))
    else:
        gm = g
    gm = torch.where(live[:, None], gm, torch.zeros(()))
    o.g_masked = gm.to(store)
    gs, ys = gm, y
    if mut == "last_row_left_out":
        last = int(torch.nonzero(live)[-1])
        gs = gm.clone()
        gs[last] = 0
    rows = _bnb_rows(M)
    sg, sgy = _block_sums(gs, rows), _block_sums(gs * ys, rows)
    mu, is_ = o.co.mean.double(), o.co.invstd.double()
    dga = is_ * (sgy - mu * sg)
    o.dgamma = (dga * OUT_SCALE).float()
    o.dbeta = (sg * (1.0 if mut == "dbeta_unscaled" else OUT_SCALE)).float()
    na = n - 1 if mut == "unbiased_count" else n
    k1 = ga * is_
    k3 = -ga * is_ * is_ * dga / na
    k2 = (0 if mut == "mean_g_dropped" else -k1 * sg / na) - k3 * mu
    k1, k2, k3 = k1.float(), k2.float(), k3.float()
    dy = k1 * gm + k2 + k3 * y
    o.dy = torch.where(live[:, None], dy, torch.zeros(())).to(store)
    return o


def run_checks(rep, case, inp, mode, emu, rm=None, rv=None):
    st = R.bn_stats(inp.y, inp.gamma, inp.beta, rows=inp.rows, running_mean=rm, running_var=rv)
    R.check_stats(rep, case, emu.co, st, running=(emu.running_mean, emu.running_var) if rm is not None else None)
    res = inp.res if mode == "relu_out" else None
    ref, bound, pre, band = R.bn_act(R._active(inp.y, inp.rows), st, relu=True, res=None if res is None else R._active(res, inp.rows), store=inp.store)
    R.check(rep, "elementwise", case, "bn_act", R._active(emu.out, inp.rows), ref, bound)
    b = R.bn_bwd(inp.y, inp.g, st, inp.gamma, mode=mode, relu_out=emu.out, rows=inp.rows, out_scale=OUT_SCALE, store=inp.store)
    R.check_bwd(rep, case, b, emu.dy, emu.dgamma, emu.dbeta, rows=inp.rows, g_masked=emu.g_masked if mode == "relu_out" else None, inactive=0.0)
    return b


@pytest.mark.parametrize("store", STORES, ids=["fp32", "f16", "bf16"])
@pytest.mark.parametrize("M", [777, 49152])
def test_faithful_emulation_passes_every_bound(M, store):
    rep = R.Report()
    for mode, row_p in (("final", None), ("relu", None), ("relu_out", None), ("relu", 0.4), ("final", 0.13)):
        inp = R.make_inputs(M, 64, store, seed=M + 7, r100=True, row_p=row_p)
        rm, rv = torch.randn(64) * 0.1, torch.rand(64) + 0.5
        emu = emulate(inp, mode, rm=rm, rv=rv)
        b = run_checks(rep, f"M={M} {mode} rows={row_p}", inp, mode, emu, rm, rv)
        # the inputs themselves: at most half of each exemption cap may lie inside the band, counted from the reference alone
        share, worst = R.band_share(b.undecided)
        assert share <= 0.5 * R.MASK_CAP_TENSOR and worst <= 0.5 * R.MASK_CAP_CHANNEL, (mode, share, worst)
    print("\n".join(rep.lines()))
    assert all(v <= 1.0 for v, _ in rep.used.values())


@pytest.mark.parametrize("mut", MUTATIONS)
def test_mutations_are_rejected_in_fp32_storage(mut):
    _rejected(mut, torch.float32, must=True)


@pytest.mark.parametrize("store", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("mut", MUTATIONS)
def test_mutations_in_16bit_storage(mut, store):
    _rejected(mut, store, must=mut in MUST_FAIL_16)


def _rejected(mut, store, must):
    M = 777
    row_p = 0.4 if mut == "inactive_rows_counted" else None
    mode = "relu"
    inp = R.make_inputs(M, 64, store, seed=M + 7, r100=True, row_p=row_p)
    run_checks(R.Report(), "faithful", inp, mode, emulate(inp, mode))          # the same case passes unmutated
    try:
        run_checks(R.Report(), mut, inp, mode, emulate(inp, mode, mut=mut))
    except AssertionError as e:
        print(f"{mut} rejected: {str(e)[:200]}")
        return
    assert not must, f"mutation {mut} passed every bound in {store}"
    print(f"{mut} is below the rounding of {store}: not rejected (allowed)")


def test_pool3d_reference_matches_the_dense_sparse_conv_oracle():
    """R.pool3d (written from the semantics) against oracle/spconv_dense.py + autograd on a small level: pooled values, the output site
    mask, and - through R.bn_bwd on the routed gradient - dy, dgamma and dbeta, with an empty half sample, a full window, exact ties
    (a constant channel: the first child wins) and NaN in the inactive rows of what R.pool3d is given."""
    import torch.nn.functional as F

    from oracle import spconv_dense as sp
    g = torch.Generator().manual_seed(5)
    B, D, C = 2, 8, 32
    mask = (torch.rand(B, 1, D, D, D, generator=g) < 0.3).double()
    mask[1, :, 4:] = 0
    mask[0, :, :2, :2, :2] = 1
    y = torch.randn(B, C, D, D, D, generator=g).double()
    y[:, 2] = 0.75
    y = y * mask
    bn = torch.nn.BatchNorm1d(C).double()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(C, generator=g) * 0.3)
    yr = y.clone().requires_grad_()
    t = sp.masked_batchnorm(bn, sp.SparseConvTensor.from_dense(yr, mask))
    t = sp.SparseMaxPool3d(2, 2)(sp.SparseConvTensor.from_dense(F.relu(t.dense), t.mask))
    dp = torch.randn(t.dense.shape, generator=g).double()
    t.dense.backward(dp)
    cl = lambda x: x.permute(0, 2, 3, 4, 1).contiguous()
    M = B * D ** 3
    m8 = mask.reshape(-1).to(torch.uint8)
    ycl = cl(y).clone()
    ycl.reshape(M, C)[~m8.bool()] = float("nan")
    st = R.bn_stats(ycl, bn.weight, bn.bias, rows=m8)
    fwd = R.pool3d(ycl, st, m8, B, D, store=torch.float32)
    assert torch.equal(fwd.mask_out.reshape(t.mask.shape).double(), t.mask)
    torch.testing.assert_close(fwd.pooled, cl(t.dense.detach()), rtol=1e-12, atol=1e-12)
    dpl = cl(dp).clone()
    dpl.reshape(-1, C)[~fwd.mask_out] = float("nan")
    bwd = R.pool3d(ycl, st, m8, B, D, store=torch.float32, pooled=fwd.pooled.float(), dpooled=dpl)
    assert not bool(bwd.undecided.any())
    b = R.bn_bwd(ycl, bwd.g, st, bn.weight, rows=m8, store=torch.float32)
    torch.testing.assert_close(b.dy, cl(yr.grad).reshape(M, C)[m8.bool()], rtol=1e-9, atol=1e-9)
    torch.testing.assert_close(b.dgamma, bn.weight.grad, rtol=1e-9, atol=1e-9)
    torch.testing.assert_close(b.dbeta, bn.bias.grad, rtol=1e-9, atol=1e-9)
