"""Float64 anchors of the BatchNorm / pooling passes (tricolo_amd/csrc/bn_pool.hip) at the layer shapes and routing branches the product
runs, through tricolo_amd.ops on the default switch set.  References and bounds: tests/bn_reference.py (derived there, proven on the CPU in
tests/test_bn_reference_cpu.py).  Every case carries the stress channels of bn_reference.make_inputs.

Left out, on purpose: the 9.6 M-row stem of the 224^2 configuration (768 x 112 x 112 x 64: its float64 reference needs ~25 GB per tensor
copy) and level 0 of the 64^3 voxel configuration (16.8 M sites x 32 channels, the same); the stem at 192 x 64^3 and voxel level 0 at
32 x 32^3 run the same kernels and routing branches."""
import functools

import pytest
import torch

from tests import bn_reference as R
from tests.guard_bands import same_bytes

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tricolo_amd import ops

DEV = "cuda"
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
STORES = [F32, F16, BF16]
IDS = {F32: "fp32", F16: "f16", BF16: "bf16"}
PREC = {F32: "bf16x3", F16: "f16", BF16: "bf16"}
OUT_SCALE = 1.0 / 4096


@pytest.fixture(scope="module")
def rep():
    r = R.Report()
    yield r
    print("\nlargest share of each bound used in this file:")
    for line in r.lines():
        print("  " + line)


def _rep(rep, store):
    """Observations are kept per storage type."""
    class View:
        def note(self, kind, value, case):
            rep.note(f"{IDS[store]} {kind}", value, case)
    return View()


def records(y, rows=None, tile=128):
    """Statistics records as the conv epilogue delivers them: (sum, sum of squares) of 128-row tiles, built in float64, rounded to fp32."""
    C = y.shape[-1]
    y2 = R.f64(y.reshape(-1, C))
    if rows is not None:
        y2 = torch.where(rows[:y2.shape[0], None].bool(), y2, torch.zeros((), dtype=torch.float64, device=y.device))
    M = y2.shape[0]
    pad = (M + tile - 1) // tile * tile
    yp = torch.zeros(pad, C, dtype=torch.float64, device=y.device)
    yp[:M] = y2
    yp = yp.reshape(-1, tile, C)
    return torch.stack([yp.sum(1), (yp * yp).sum(1)], 1).float().contiguous()


def finalize(rep, case, inp, y=None, gamma=None, beta=None, count_dev=None, running=False):
    y = inp.y if y is None else y
    gamma, beta = inp.gamma if gamma is None else gamma, inp.beta if beta is None else beta
    C = y.shape[-1]
    rm = rv = nbt = rm0 = rv0 = None
    if running:
        gen = torch.Generator().manual_seed(5)
        rm, rv = (torch.randn(C, generator=gen) * 0.1).to(DEV), (torch.rand(C, generator=gen) + 0.5).to(DEV)
        rm0, rv0, nbt = rm.clone(), rv.clone(), torch.zeros((), dtype=torch.long, device=DEV)
    n = y.numel() // C
    co = ops.bn_finalize(records(y, inp.rows), C, gamma, beta, rm, rv, nbt, count_dev=count_dev, count_host=0 if count_dev is not None else n)
    st = R.bn_stats(y, gamma, beta, rows=inp.rows, running_mean=rm0, running_var=rv0)
    R.check_stats(rep, case, co, st, running=(rm, rv) if running else None)
    if running:
        assert int(nbt.item()) == 1
    return co, st


# ------------------------------------------------------------------------------------------------ image tower
TOWER = [(196608, 64), (49152, 128), (12288, 256), (3072, 512)]                    # batch 32, 6 views, 128^2
TOWER_224 = [(2408448, 64), (37632, 512)]                                          # 768 images of 224^2: 16-bit storage only
TOWER_CASES = [(M, C, s) for (M, C) in TOWER for s in STORES] + [(M, C, s) for (M, C) in TOWER_224 for s in (F16, BF16)]


@pytest.mark.parametrize("M,C,store", TOWER_CASES, ids=[f"{M}x{C}-{IDS[s]}" for M, C, s in TOWER_CASES])
def test_image_tower_layer(rep, M, C, store):
    """bn_finalize, bn_act (plain, identity residual, down-sample residual), bn_bwd in its three mask forms and bn_bwd_pair against float64
    at the layer shapes of the bench step - (196608, 64) and (2408448, 64) run the capped-block regime of the backward sums (256- and
    1,216-row blocks), and every tensor here runs the grid-stride loop of the elementwise passes more than once."""
    rp = _rep(rep, store)
    case = f"tower {M}x{C} {IDS[store]}"
    inp = R.make_inputs(M, C, store, seed=M % 1000 + C, device=DEV, grad_scale=64.0 if store != F32 else 1.0)
    co, st = finalize(rp, case, inp, running=True)
    gen = torch.Generator().manual_seed(C)
    gamma_b, beta_b = (torch.rand(C, generator=gen) + 0.5).to(DEV), (torch.randn(C, generator=gen) * 0.3).to(DEV)
    shadow = R.SimpleNamespace(rows=None)
    cob, stb = finalize(rp, case + " shortcut", shadow, y=inp.res, gamma=gamma_b, beta=beta_b)
    outs = {}
    for name, kw, rkw in (("plain", {}, {}), ("identity", dict(res=inp.res), dict(res=inp.res)),
                          ("downsample", dict(res=inp.res, res_co=cob), dict(res=inp.res, res_st=stb))):
        out = ops.bn_act(inp.y, co, relu=True, **kw)
        ref, bound, _, _ = R.bn_act(inp.y, st, relu=True, store=store, **rkw)
        R.check(rp, "elementwise", case, f"bn_act {name}", out, ref, bound)
        outs[name] = out
        del ref, bound
    cnt = M
    for mode, kw in (("final", {}), ("relu", dict(relu=True)), ("relu_out", dict(relu_out=outs["identity"]))):
        gm = torch.empty_like(inp.g) if mode == "relu_out" else None
        dy, dgamma, dbeta = ops.bn_bwd(inp.y, inp.g, co, inp.gamma, count_host=cnt, inplace=False, out_scale=OUT_SCALE, g_masked=gm, **kw)
        b = R.bn_bwd(inp.y, inp.g, st, inp.gamma, mode=mode, relu_out=outs["identity"], out_scale=OUT_SCALE, store=store)
        R.check_bwd(rp, f"{case} bn_bwd {mode}", b, dy, dgamma, dbeta, g_masked=gm)
        del b, dy
    if (M, C) in TOWER[1:]:                                   # the three down-sampling BasicBlocks
        out = outs["downsample"]
        gm = torch.empty_like(inp.g)
        dya, dga, dba, dyb, dgb, dbb = ops.bn_bwd_pair(inp.y, co, inp.gamma, inp.res, cob, gamma_b, inp.g, out, M, g_masked=gm, out_scale=OUT_SCALE)
        a = R.bn_bwd(inp.y, inp.g, st, inp.gamma, mode="relu_out", relu_out=out, out_scale=OUT_SCALE, store=store)
        R.check_bwd(rp, f"{case} bn_bwd_pair a", a, dya, dga, dba, g_masked=gm)
        bb = R.bn_bwd(inp.res, a.g_masked, stb, gamma_b, mode="final", out_scale=OUT_SCALE, store=store)
        R.check_bwd(rp, f"{case} bn_bwd_pair b", bb, dyb, dgb, dbb)


@pytest.mark.parametrize("store", STORES, ids=["fp32", "f16", "bf16"])
def test_mean_over_std_100_channel(rep, store):
    """One run with a channel at |mean| / std = 100: held to the r-dependent bounds like every other channel, and reported."""
    own = R.Report()
    inp = R.make_inputs(12288, 256, store, seed=100, device=DEV, r100=True)
    co, st = finalize(own, f"r100 {IDS[store]}", inp)
    out = ops.bn_act(inp.y, co, relu=True)
    ref, bound, _, _ = R.bn_act(inp.y, st, relu=True, store=store)
    R.check(own, "elementwise", "r100", "bn_act", out, ref, bound)
    dy, dgamma, dbeta = ops.bn_bwd(inp.y, inp.g, co, inp.gamma, count_host=inp.M, inplace=False, relu=True)
    R.check_bwd(own, "r100 bn_bwd relu", R.bn_bwd(inp.y, inp.g, st, inp.gamma, mode="relu", store=store), dy, dgamma, dbeta)
    fr = R.fraction(co.invstd[8:9], st.invstd[8:9], st.b_invstd[8:9])
    print(f"|mean|/std = 100, {IDS[store]}: r^2 = {float(st.r2[8]):.4g}, invstd uses {float(fr):.3g} of its bound; " + "; ".join(own.lines()))
    for k, (v, c) in own.used.items():
        rep.note(f"{IDS[store]} r100 {k}", v, c)


# ------------------------------------------------------------------------------------------------ regime edges
EDGE_M = [1, 2, 15, 17, 511, 512, 513, 16384, 16385, 32768, 32769, 65535, 65536, 65537, 131071]


EDGE_CASES = [(M, C) for i, M in enumerate(EDGE_M) for C in (64, (32, 96, 512)[i % 3])]       # C = 64 and one second channel count per row count


@pytest.mark.parametrize("store", [F32, F16], ids=["fp32", "f16"])
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "rowmask"])
@pytest.mark.parametrize("M,C", EDGE_CASES)
def test_bn_bwd_regime_edges(rep, monkeypatch, M, C, masked, store):
    """Every regime of bnb_rows (16 / 32 / 64 rows per block, the capped regime from 65,536 rows on) and of the one-launch small path
    (M <= 512, C >= 64), one row to either side of each edge, with and without a row mask and a device-side count."""
    rp = _rep(rep, store)
    case = f"edge {M}x{C} {'rowmask' if masked else 'plain'} {IDS[store]}"
    calls = _count_calls(monkeypatch, ("tri_bn_bwd_small", "tri_bn_bwd_reduce"))
    inp = R.make_inputs(M, C, store, seed=M + C, device=DEV, row_p=0.4 if masked else None)
    cnt = ops.mask_count(inp.rows, M) if masked else None
    co, st = finalize(rp, case, inp, count_dev=cnt)
    g = inp.g.clone()
    if masked:
        g[~inp.rows[:M].bool()] = 123.0
    dy, dgamma, dbeta = ops.bn_bwd(inp.y, g, co, inp.gamma, count_dev=cnt, count_host=0 if masked else M, row_mask=inp.rows, inplace=False,
                                   out_scale=0.5)
    small = M <= 512 and C >= 64
    assert calls == {"tri_bn_bwd_small": int(small), "tri_bn_bwd_reduce": int(not small)}, calls
    assert ops.lib().tri_bn_bwd_num_blocks(M) == -(-M // (16 if M <= 16384 else 32 if M <= 32768 else 64 if M < 65536 else 256))
    b = R.bn_bwd(inp.y, inp.g, st, inp.gamma, mode="final", rows=inp.rows, out_scale=0.5, store=store)
    R.check_bwd(rp, case, b, dy, dgamma, dbeta, rows=inp.rows, inactive=0.0)
    if masked:                                                  # keep_inactive: the same values, inactive rows untouched
        dy2 = g.clone()
        _, dg2, db2 = ops.bn_bwd(inp.y, dy2, co, inp.gamma, count_dev=cnt, row_mask=inp.rows, inplace=True, out_scale=0.5, keep_inactive=True)
        R.check_bwd(rp, case + " keep_inactive", b, dy2, dg2, db2, rows=inp.rows, inactive=123.0)


def _count_calls(monkeypatch, names):
    """Count the calls of entry points of the native library (inside the test only)."""
    real = ops.lib()
    calls = {n: 0 for n in names}

    class Counting:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if name not in calls:
                return fn

            def counted(*a):
                calls[name] += 1
                return fn(*a)
            return counted
    proxy = Counting()
    monkeypatch.setattr(ops, "lib", lambda: proxy)
    return calls


@pytest.mark.parametrize("store", [F32, F16], ids=["fp32", "f16"])
@pytest.mark.parametrize("M,C", [(256, 64), (4096, 64)])
@pytest.mark.parametrize("active", [0, 1])
def test_row_counts_of_zero_and_one_from_a_device_counter(rep, M, C, active, store):
    """No active row: every output exactly zero and the running statistics untouched.  One active row: variance 0, dy = 0 within bounds."""
    rp = _rep(rep, store)
    inp = R.make_inputs(M, C, store, seed=M + active, device=DEV, row_p=0.5)
    rows = torch.zeros_like(inp.rows)
    if active:
        rows[int(torch.nonzero(inp.rows)[3])] = 1
    inp.rows = rows
    cnt = ops.mask_count(rows, M)
    assert int(cnt.item()) == active
    case = f"count {active} {M}x{C} {IDS[store]}"
    rm, rv, nbt = torch.full((C,), 0.25, device=DEV), torch.full((C,), 1.5, device=DEV), torch.zeros((), dtype=torch.long, device=DEV)
    co = ops.bn_finalize(records(inp.y, rows), C, inp.gamma, inp.beta, rm, rv, nbt, count_dev=cnt)
    st = R.bn_stats(inp.y, inp.gamma, inp.beta, rows=rows, running_mean=torch.full((C,), 0.25, device=DEV),
                    running_var=torch.full((C,), 1.5, device=DEV))
    if active:
        R.check_stats(rp, case, co, st, running=(rm, rv))
    else:
        for v in (co.mean, co.invstd, co.scale, co.shift):
            assert bool((v == 0).all())
        assert bool((rm == 0.25).all()) and bool((rv == 1.5).all())
    g = inp.g.clone()
    dy, dgamma, dbeta = ops.bn_bwd(inp.y, g, co, inp.gamma, count_dev=cnt, row_mask=rows, inplace=False, out_scale=0.5)
    if active:
        R.check_bwd(rp, case, R.bn_bwd(inp.y, inp.g, st, inp.gamma, rows=rows, out_scale=0.5, store=store), dy, dgamma, dbeta, rows=rows, inactive=0.0)
    else:
        assert bool((dy == 0).all()) and bool((dgamma == 0).all()) and bool((dbeta == 0).all())


# ------------------------------------------------------------------------------------------------ stem
@pytest.mark.parametrize("store", STORES, ids=["fp32", "f16", "bf16"])
def test_stem_bn_relu_maxpool_forward_and_backward(rep, store):
    """The stem of the bench step (192 images, 64 x 64 x 64 out of the 7x7 conv): BatchNorm + ReLU + 3x3 / 2 max-pool in one pass - pooled
    values and the tap map - and its backward through the two BatchNorm passes, with and without the forward's pooled tensor.
    A tap may differ from the float64 first maximum only where the float64 value of the chosen tap is within the bound of that maximum;
    the backward is then checked with the map it was given."""
    N, S, C = 192, 64, 64
    M = N * S * S
    rp = _rep(rep, store)
    case = f"stem {N}x{S}x{S}x{C} {IDS[store]}"
    inp = R.make_inputs(M, C, store, seed=11, device=DEV, grad_scale=64.0 if store != F32 else 1.0)
    co, st = finalize(rp, case, inp)
    y = inp.y.reshape(N, 1, S, S, C)
    pooled, arg = ops.maxpool2d_fwd(y, bn=co)
    ref = R.stem_pool(y, st, store=store)
    R.check(rp, "elementwise", case, "pooled", pooled.reshape(-1, C), ref.pooled.reshape(-1, C), ref.b_pooled.reshape(-1, C))
    tap = arg.reshape(ref.tap.shape).long()
    assert int(tap.max()) <= 8
    differs = tap != ref.tap
    chosen = torch.gather(ref.z, 3, tap.unsqueeze(3)).squeeze(3)
    # the pass chose tap k over the float64 winner j because z32_k >= z32_j; each fp32 value is within its bound b of the float64 one, so
    # z64_k >= z32_k - b_k >= z32_j - b_k >= z64_j - b_j - b_k: within twice the largest bound of the window
    close = chosen >= ref.pooled - 2 * ref.b_z.max(3).values
    assert not bool((differs & ~close).any()), (case, "tap map", int((differs & ~close).sum()))
    share, worst = R.band_share(differs)
    rp.note("tap exemption, share of a tensor", share, case)
    assert share <= R.MASK_CAP_TENSOR and worst <= R.MASK_CAP_CHANNEL, (share, worst)
    del ref, chosen, close
    Mo = pooled.numel() // C
    dpool = torch.randn(Mo, C, generator=torch.Generator().manual_seed(12)) * (64.0 if store != F32 else 1.0)
    dpool[:, 2:4] = torch.randn(Mo, 2, generator=torch.Generator().manual_seed(13))      # (variance 0: see make_inputs)
    dpool = dpool.to(DEV).to(store).reshape(pooled.shape)
    rb = R.stem_pool(y, st, store=store, dpool=dpool, tap=arg)
    b = R.bn_bwd(y, rb.g, st, inp.gamma, mode="final", out_scale=OUT_SCALE, store=store, undecided=rb.undecided, g_unmasked=rb.g_unmasked)
    # the plain max-pool backward over the same map (tri_maxpool2d_bwd): at most four windows meet in one pixel, summed in fp32
    dx = ops.maxpool2d_bwd(arg, dpool, y.shape)
    mass = R.stem_pool(y, st, store=store, dpool=dpool.abs(), tap=arg).g_unmasked.reshape(-1, C)
    R.check(rp, "elementwise", case, "maxpool2d_bwd", dx.reshape(-1, C), rb.g_unmasked.reshape(-1, C),
            R.eps_of(store) * rb.g_unmasked.abs().reshape(-1, C) + R.tiny_of(store) + 8 * R.U32 * mass)
    del rb, mass, dx
    for with_pooled in (False, True):
        dy, dgamma, dbeta = ops.maxpool_bn_bwd(y, arg, dpool, co, inp.gamma, out_scale=OUT_SCALE, pooled=pooled if with_pooled else None)
        R.check_bwd(rp, f"{case} maxpool_bn_bwd pooled={with_pooled}", b, dy, dgamma, dbeta)


@pytest.mark.parametrize("store", [F16, F32], ids=["f16", "fp32"])
def test_stem_on_an_odd_map_through_maxpool_bn_bwd_wgrad(rep, store):
    """ops.maxpool_bn_bwd_wgrad on 2 images whose 7x7 / 2 stem conv gives 15 x 15 x 64 (tap map and pooled tensor 8 x 8: the last pooled
    row and column are partial windows) - the smallest shape of the odd-size form: dw, dgamma and dbeta bit for bit those of
    ops.maxpool2d_bwd, ops.bn_bwd(relu=True, count_host=g.M), ops.conv_wgrad, and the two stages against float64: the routed gradient
    within maxpool2d_bwd's bound, dgamma / dbeta / dy within bn_bwd's for the routed gradient as stored."""
    N, S, C = 2, 15, 64
    rp = _rep(rep, store)
    case = f"stem {N}x{S}x{S}x{C} {IDS[store]}"
    inp = R.make_inputs(N * S * S, C, store, seed=15, device=DEV, grad_scale=64.0 if store != F32 else 1.0)
    co, st = finalize(rp, case, inp)
    y = inp.y.reshape(N, 1, S, S, C)
    pooled, arg = ops.maxpool2d_fwd(y, bn=co)
    assert tuple(pooled.shape) == (N, 1, 8, 8, C)
    gen = torch.Generator().manual_seed(16)
    dpool = torch.randn(pooled.numel() // C, C, generator=gen) * (64.0 if store != F32 else 1.0)
    dpool[:, 2:4] = torch.randn(pooled.numel() // C, 2, generator=gen)                   # (variance 0: see make_inputs)
    dpool = dpool.to(DEV).to(store).reshape(pooled.shape)
    x0 = torch.randn(N, 1, 2 * S, 2 * S, 4, generator=gen)
    x0[..., 3] = 0.0                                                                     # (3 image channels stored as 4)
    x0, like = x0.to(DEV).to(store), torch.empty(C, 3, 1, 7, 7, device=DEV)
    geom = ops.ConvGeom(N, (1, 2 * S, 2 * S), 3, 4, C, (1, 7, 7), 2, (0, 3, 3), (3 * 49, 1, 49))
    assert geom.out_grid == (1, S, S) and geom.M == N * S * S
    dw, dgamma, dbeta = ops.maxpool_bn_bwd_wgrad(x0, y, arg, dpool, co, inp.gamma, geom, like, PREC[store], out_scale=OUT_SCALE, pooled=pooled)
    dz = ops.maxpool2d_bwd(arg, dpool, tuple(y.shape))
    routed = dz.clone()
    dy, dgamma2, dbeta2 = ops.bn_bwd(y, dz, co, inp.gamma, count_host=geom.M, relu=True, out_scale=OUT_SCALE)
    dw2 = ops.conv_wgrad(x0, dy, geom, like, PREC[store], out_scale=OUT_SCALE)
    assert same_bytes(dw, dw2) and same_bytes(dgamma, dgamma2) and same_bytes(dbeta, dbeta2)
    assert bool(torch.isfinite(dw).all()) and float(dw.abs().max()) > 0
    rb = R.stem_pool(y, st, store=store, dpool=dpool, tap=arg)
    mass = R.stem_pool(y, st, store=store, dpool=dpool.abs(), tap=arg).g_unmasked.reshape(-1, C)
    R.check(rp, "elementwise", case, "maxpool2d_bwd", routed.reshape(-1, C), rb.g_unmasked.reshape(-1, C),
            R.eps_of(store) * rb.g_unmasked.abs().reshape(-1, C) + R.tiny_of(store) + 8 * R.U32 * mass)
    b = R.bn_bwd(y.reshape(-1, C), routed.reshape(-1, C), st, inp.gamma, mode="relu", out_scale=OUT_SCALE, store=store)
    R.check_bwd(rp, f"{case} maxpool_bn_bwd_wgrad", b, dy.reshape(-1, C), dgamma, dbeta)


# ------------------------------------------------------------------------------------------------ running statistics
def test_running_statistics_over_three_updates(rep):
    M, C = 196608, 64
    rp = _rep(rep, F16)
    inp = R.make_inputs(M, C, F16, seed=3, device=DEV)
    gen = torch.Generator().manual_seed(8)
    rm0, rv0 = torch.randn(C, generator=gen).to(DEV) * 0.1, (torch.rand(C, generator=gen) + 0.5).to(DEV)
    rm, rv, nbt = rm0.clone(), rv0.clone(), torch.zeros((), dtype=torch.long, device=DEV)
    cnt = torch.full((1,), M, dtype=torch.int32, device=DEV)
    rec = records(inp.y)
    for _ in range(3):
        co = ops.bn_finalize(rec, C, inp.gamma, inp.beta, rm, rv, nbt, count_dev=cnt)
    st = R.bn_stats(inp.y, inp.gamma, inp.beta, running_mean=rm0, running_var=rv0, updates=3)
    R.check_stats(rp, "running x3 196608x64", co, st, running=(rm, rv))
    assert int(nbt.item()) == 3


# ------------------------------------------------------------------------------------------------ conv epilogue -> bn_finalize
EPILOGUE = [("c3x3", 192, 32, 64, 64, (1, 3, 3), 1, (0, 1, 1), None), ("c1x1s2", 768, 32, 64, 128, (1, 1, 1), 2, (0, 0, 0), 1536),
            ("c1x1", 768, 32, 64, 64, (1, 1, 1), 1, (0, 0, 0), 6144)]                       # ..., records (128 rows each; the 64 -> 64 channel 3x3 kernel of 16-bit storage writes one per brick: 512)


@pytest.mark.parametrize("store", STORES, ids=["fp32", "f16", "bf16"])
@pytest.mark.parametrize("layer", EPILOGUE, ids=[e[0] for e in EPILOGUE])
def test_statistics_from_the_conv_epilogue(rep, layer, store):
    """The producer / consumer contract at real record counts: ops.conv_fwd(want_stats=True) on real-valued input, ops.bn_finalize on the
    records it wrote, against bn_stats of the tensor it wrote: 512 / 1,536 and 6,144 records, 2, 6 and 24 trips of bn_finalize_kernel's 256 lanes."""
    name, B, S, cin, cout, k, s, p, nrec = layer
    rp = _rep(rep, store)
    gen = torch.Generator().manual_seed(cin + cout)
    x = (torch.randn(B, 1, S, S, cin, generator=gen) + 0.3).to(DEV).to(store)
    w = (torch.randn(cout, cin, *k, generator=gen) / (cin * k[1] * k[2]) ** 0.5)
    w[3] *= 0.02                                                                  # a channel with a small spread ...
    w[4] = w[4] * 0.05 + 0.3                                                     # ... and one with a large mean (the input's mean is 0.3)
    ntaps = k[0] * k[1] * k[2]
    geom = ops.ConvGeom(B, (1, S, S), cin, cin, cout, k, s, p, (cin * ntaps, 1, ntaps))
    y, stats = ops.conv_fwd(x, geom, ops.pack_weight(w.contiguous().to(DEV), geom, PREC[store]), want_stats=True)
    assert y.dtype == store and (stats.shape[0] == nrec if nrec else stats.shape[0] > 256), stats.shape
    M = y.numel() // cout
    gamma, beta = (torch.rand(cout, generator=gen) + 0.5).to(DEV), (torch.randn(cout, generator=gen) * 0.3).to(DEV)
    co = ops.bn_finalize(stats, cout, gamma, beta, None, None, None, count_host=M)
    st = R.bn_stats(y, gamma, beta)
    R.check_stats(rp, f"epilogue {name} {IDS[store]} ({stats.shape[0]} records)", co, st)
    print(f"epilogue {name} {IDS[store]}: largest |mean|/std of a channel {float(st.r2.max()) ** 0.5:.3g}")


# ------------------------------------------------------------------------------------------------ heads
@pytest.mark.parametrize("store", STORES, ids=["fp32", "f16", "bf16"])
@pytest.mark.parametrize("B,V,HW,C", [(32, 6, 16, 512), (64, 12, 49, 512)])
def test_avgpool_viewmax_against_float64(rep, B, V, HW, C, store):
    """Global average pool + maximum over the views.  Inputs on a 1/64 grid: every fp32 sum is exact, so the winning view is decided
    without a tie band and must equal the float64 one; views 1, 4 and the last are copies of view 0 (first maximal view wins)."""
    rp = _rep(rep, store)
    H = int(HW ** 0.5)
    gen = torch.Generator().manual_seed(B + HW)
    x = torch.randint(-128, 129, (B, V, H, H, C), generator=gen).float() / 64
    x[:, 1], x[:, 4], x[:, V - 1] = x[:, 0], x[:, 0], x[:, 0]
    x = x.reshape(B * V, 1, H, H, C).to(DEV).to(store)
    dout = torch.randn(B, C, generator=gen).to(DEV)
    out, arg = ops.avgpool_viewmax_fwd(x, B, V)
    ref, rarg, bound, means, rdx = R.avgpool_viewmax(x, B, V, dout=dout, scale=64.0)
    assert torch.equal(arg.long(), rarg), int((arg.long() != rarg).sum())
    assert int((rarg == 0).sum()) > B * C // (V * 2) and not bool(((rarg == 1) | (rarg == 4) | (rarg == V - 1)).any())
    case = f"viewmax {B}x{V}x{HW}x{C} {IDS[store]}"
    R.check(rp, "elementwise", case, "out", out, ref, bound)
    dx = ops.avgpool_viewmax_bwd(dout, arg, x.shape, B, V, dtype=store, scale=64.0)
    R.check(rp, "elementwise", case, "dx", dx.reshape(-1, C), rdx.reshape(-1, C), R.eps_of(store) * rdx.abs().reshape(-1, C) + R.tiny_of(store) + 8 * R.U32 * rdx.abs().reshape(-1, C))


@pytest.mark.parametrize("store", STORES, ids=["fp32", "f16", "bf16"])
def test_eval_mode_coefficients_and_apply(rep, store):
    rp = _rep(rep, store)
    inp = R.make_inputs(3072, 512, store, seed=77, device=DEV)
    gen = torch.Generator().manual_seed(78)
    rm, rv = (torch.randn(512, generator=gen) * 0.5).to(DEV), (torch.rand(512, generator=gen) * 2 + 0.01).to(DEV)
    rv[2] = 0.0
    co = ops.bn_eval_coeffs(512, inp.gamma, inp.beta, rm, rv)
    st = R.eval_stats(inp.gamma, inp.beta, rm, rv)
    case = f"eval 3072x512 {IDS[store]}"
    R.check_stats(rp, case, co, st)
    for relu in (True, False):
        out = ops.bn_act(inp.y, co, relu=relu)
        ref, bound, _, _ = R.bn_act(inp.y, st, relu=relu, store=store)
        R.check(rp, "elementwise", case, f"bn_act relu={relu}", out, ref, bound)


# ------------------------------------------------------------------------------------------------ ReLU backward
@pytest.mark.parametrize("store", STORES, ids=["fp32", "f16", "bf16"])
@pytest.mark.parametrize("M,C", [(196608, 64), (4096 * 256 * 3 // 16 + 37, 64)])
def test_relu_bwd_mask_is_exact(M, C, store):
    """g = dout * (out > 0) from a saved output, out of place and in place: exact, with zeros, negative zeros and the smallest subnormal in
    the saved output; the second size ends inside a grid-stride pass."""
    gen = torch.Generator().manual_seed(M % 977)
    out = torch.relu(torch.randn(M, C, generator=gen))
    out[::7, 1], out[::5, 2] = -0.0, R.tiny_of(store)
    out, dout = out.to(DEV).to(store), torch.randn(M, C, generator=gen).to(DEV).to(store)
    assert bool((out[::5, 2] > 0).all())
    ref = torch.where(R.f64(out) > 0, R.f64(dout), torch.zeros((), dtype=torch.float64, device=DEV))
    g = ops.relu_bwd(dout, out, inplace=False)
    assert torch.equal(R.f64(g), ref)
    d2 = dout.clone()
    assert ops.relu_bwd(d2, out, inplace=True) is d2 and torch.equal(R.f64(d2), ref)


# ------------------------------------------------------------------------------------------------ voxel tower
VOX_CH = [32, 64, 128, 256, 512]
POOL_ENTRIES = ("tri_pool3d_bwd_route", "tri_pool3d_bwd_route_rows", "tri_pool3d_bwd_route_rows_reduce", "tri_pool3d_bwd_route_reduce",
                "tri_bn_bwd_rows", "tri_bn_bwd_apply_rows", "tri_bn_bwd_apply", "tri_bn_bwd_reduce", "tri_bn_bwd_small", "tri_bn_bwd_finalize")


@functools.lru_cache(maxsize=4)
def _mask_pyramid(B, V, p):
    """Site masks of the five levels: level 0 at occupancy p with sample 1 empty and one full 2x2x2 window, each further level the OR of
    its 2x2x2 children."""
    gen = torch.Generator().manual_seed(int(p * 1000) + V)
    m = torch.rand(B, V, V, V, generator=gen) < p
    m[1] = False
    m[0, :2, :2, :2] = True
    out = [m]
    for _ in range(4):
        D = out[-1].shape[1]
        out.append(R._windows3d(out[-1].reshape(B, D, D, D, 1), B, D).any(4).reshape(B, D // 2, D // 2, D // 2))
    return out


VOXEL_CASES = [("bench", 32, 32, l, p, s) for p in (0.13, 0.01) for l in range(5) for s in STORES] + \
              [("config5", 64, 64, l, 0.13, F16) for l in range(1, 5)]


@pytest.mark.parametrize("name,B,V,l,p,store", VOXEL_CASES, ids=[f"{n}-l{l}-p{p}-{IDS[s]}" for n, _, _, l, p, s in VOXEL_CASES])
def test_voxel_level_forward_and_backward(rep, monkeypatch, name, B, V, l, p, store):
    """One level of the voxel tower as SparseCNNEncoder runs it: statistics over the active sites from a device count, BatchNorm + ReLU +
    2x2x2 max-pool with the output site mask, and ops.pool3d_bn_bwd with rows / rows_out / keep_inactive (level 0), fused and unfused - so
    that its four branches and, at 256 rows, tri_bn_bwd_small are reached, which is asserted on the entry points called.  Inactive rows of
    y and of the pooled gradient hold NaN; sample 1 is empty; one window is full.  The backward takes the forward's stored pooled tensor as
    its input (checked first), see bn_reference.pool3d."""
    D, C = V >> l, VOX_CH[l]
    M, Mo = B * D ** 3, B * (D // 2) ** 3
    rp = _rep(rep, store)
    case = f"voxel {name} level {l} ({B}x{D}^3x{C}) p={p} {IDS[store]}"
    masks = _mask_pyramid(B, V, p)
    gs = 64.0 if store != F32 else 1.0
    inp = R.make_inputs(M, C, store, seed=l + int(p * 100), device=DEV, grad_scale=gs, live=masks[l])
    assert not bool(masks[l][1].any()) and bool(torch.isnan(inp.y[~inp.rows[:M].bool()].float()).all())
    rows = ops.mask_compact(inp.rows, M)
    cnt = rows[1]
    assert int(cnt.item()) == int(masks[l].sum())
    co, st = finalize(rp, case, inp, count_dev=cnt)
    y = inp.y.reshape(B, D, D, D, C)
    pooled, mask_out = ops.bn_relu_pool3d_fwd(y, co, inp.rows, B, D, C)
    ref = R.pool3d(y, st, inp.rows, B, D, store=store)
    R.check(rp, "elementwise", case, "pooled", pooled.reshape(-1, C), ref.pooled.reshape(-1, C), ref.b_pooled.reshape(-1, C))
    assert torch.equal(mask_out[:Mo].bool(), ref.mask_out) and not bool(mask_out[Mo:].any()), (case, "site mask")
    if l < 4:
        assert torch.equal(ref.mask_out.cpu(), masks[l + 1].reshape(-1))
    live_out = ref.mask_out
    del ref
    gen = torch.Generator().manual_seed(l + 50)
    dp = torch.randn(Mo, C, generator=gen) * gs
    dp[:, 2:4] = torch.randn(Mo, 2, generator=gen)                                   # (variance 0: see make_inputs)
    dp = dp.to(DEV)
    dp[~live_out] = float("nan")
    dp = dp.to(store).reshape(pooled.shape)
    rows_out = ops.mask_compact(mask_out, Mo) if l < 4 else None
    rb = R.pool3d(y, st, inp.rows, B, D, store=store, pooled=pooled, dpooled=dp)
    b = R.bn_bwd(y, rb.g, st, inp.gamma, mode="final", rows=inp.rows, out_scale=OUT_SCALE, store=store, undecided=rb.undecided, g_unmasked=rb.g_abs)
    del rb
    big, keep = M > 16384, l == 0
    calls = _count_calls(monkeypatch, POOL_ENTRIES)
    for fused in (True, False):
        for k in calls:
            calls[k] = 0
        dy, dgamma, dbeta = ops.pool3d_bn_bwd(y, co, inp.rows, pooled, dp, B, D, C, inp.gamma, cnt, out_scale=OUT_SCALE, fused=fused,
                                              keep_inactive=keep, rows=rows if keep else None, rows_out=rows_out)
        if big and fused:
            want = {"tri_pool3d_bwd_route_rows_reduce": 1, "tri_bn_bwd_finalize": 1, "tri_bn_bwd_apply_rows" if keep else "tri_bn_bwd_apply": 1}
        elif big and keep:
            want = {"tri_pool3d_bwd_route_rows": 1, "tri_bn_bwd_rows": 1}
        elif big:
            want = {"tri_pool3d_bwd_route_rows": 1, "tri_bn_bwd_reduce": 1, "tri_bn_bwd_finalize": 1, "tri_bn_bwd_apply": 1}
        elif fused:
            want = {"tri_pool3d_bwd_route_reduce": 1, "tri_bn_bwd_finalize": 1, "tri_bn_bwd_apply": 1}
        elif M <= 512:
            want = {"tri_pool3d_bwd_route": 1, "tri_bn_bwd_small": 1}
        else:
            want = {"tri_pool3d_bwd_route": 1, "tri_bn_bwd_reduce": 1, "tri_bn_bwd_finalize": 1, "tri_bn_bwd_apply": 1}
        assert {k: v for k, v in calls.items() if v} == want, (case, fused, calls)
        # (level 0 leaves the inactive rows of dy unwritten: nothing to observe there)
        R.check_bwd(rp, f"{case} pool3d_bn_bwd fused={fused}", b, dy, dgamma, dbeta, rows=inp.rows, inactive=None if keep else 0.0)
