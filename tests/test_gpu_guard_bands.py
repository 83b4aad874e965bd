"""Guard-band tests (tests/guard_bands.py): a call's result does not depend on memory outside its operands, and the call leaves that
memory alone.  Default switch set; no TRICOLO_* variable is set here.

Every case runs twice - once with 0xFF bands (NaN in every float type, "active" in a site mask), once with 0x00 bands - with EVERY
operand inside bands: the test's own inputs through Guard.put, what tricolo_amd.ops allocates (outputs, BatchNorm records, packed
operands, scratch, workspaces and weight-gradient slabs of exactly the planned size) through guarded_ops.  It asserts that all bands
are intact after both runs, that the outputs of the 0xFF run match the reference of the kernel's existing test (named per group), and
that the outputs of the two runs are bit-identical.

The last test runs eager training steps under the recording wrapper and asserts that every entry point they launch was launched by
a guarded case of this file (or is named in EXEMPT)."""
import collections
import functools
from itertools import combinations

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import bn_reference as R
from tests.guard_bands import POISON, ZERO, guarded_ops, recording, same_bytes, stream_entry_points
from tests.test_gpu_ops import BF16_CASES, CONV_CASES, KROW_CASES, STORE16, WGRAD_JOB_CASES, _blob_mask, cf3, cl3, ints, make_case
from tricolo_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
IDS = {F32: "fp32", F16: "f16", BF16: "bf16"}
PREC = {F32: "bf16x3", F16: "f16", BF16: "bf16"}
STORES = [F32, F16, BF16]
FP32_MODES = ((F32, "bf16"), (F32, "bf16x3"))
S16 = tuple(STORE16)
LAUNCHED = set()                     # entry points launched by the guarded cases of this process (the completeness test reads it)


def twice(body):
    """Run body(guard) -> {name: device tensor} under 0xFF and under 0x00 bands; bands are checked on exit of each context.  The two
    runs' outputs must be bit-identical; returns the 0xFF run's (on the host)."""
    res = []
    for fill in (POISON, ZERO):
        try:
            with guarded_ops(fill) as g:
                out = body(g)
                out = {k: v.detach().cpu() for k, v in out.items() if v is not None}
        except RuntimeError as e:
            if any(w in str(e) for w in ("illegal memory access", "HIP error", "hipError")):       # a GPU fault ends the job: nothing more runs on the device
                pytest.exit(f"GPU fault in a guarded case ({fill:#04x} bands): {e}", returncode=3)
            raise
        LAUNCHED.update(g.launched)
        res.append(out)
    a, b = res
    assert a.keys() == b.keys()
    for k in a:
        assert same_bytes(a[k], b[k]), f"{k}: differs between the 0xFF-band and the 0x00-band run - it depends on memory outside the operands"
    return a


def col_sums_ok(stats, exact, atol):
    """BatchNorm records sum to the column sums (and sums of squares) of the stored values, as in tests/test_gpu_ops.py."""
    st = stats.double().sum(0)
    np.testing.assert_allclose(st[0].numpy(), exact.sum(0).numpy(), rtol=1e-6, atol=atol)
    np.testing.assert_allclose(st[1].numpy(), (exact ** 2).sum(0).numpy(), rtol=1e-6, atol=atol)


# ================================================================================================ conv forward and data gradient
ConvCase = collections.namedtuple("ConvCase", "name case modes dirs form acc epi", defaults=(False,))     # epi: also a bias + ReLU epilogue call
_BY = {c[0]: c for c in CONV_CASES + BF16_CASES}


def _vox(name, B, D, cin, cout):
    return (name, B, (D, D, D), cin, cout, (3, 3, 3), 1, (1, 1, 1), "spconv")


def _s2(name, N, H, W, cin, cout):
    return (name, N, (1, H, W), cin, cout, (1, 3, 3), 2, (0, 1, 1), "torch")


BOTH = ("fwd", "dgrad")
# the smallest existing case of each family with a partial last tile (tests/test_gpu_ops.py); references: test_conv_fwd_integer_exact,
# test_conv_dgrad_integer_exact, test_conv_16bit_storage_integer_exact, test_conv_16bit_storage_masked_stats, test_voxel_level0_brick_kernel,
# test_voxel_level1_ranked_brick_kernel, test_voxel_coarse_grid_kernel, test_stride2_slab_kernel - exact equality on integer data
CONV_TABLE = [
    # conv_igemm_kernel: fp32 storage in both operand modes (split-K plans with their workspace), a compact row list, a row mask
    ConvCase("igemm_vox_l3", _BY["vox_l3"], FP32_MODES, BOTH, "dense", True),
    ConvCase("igemm_odd14", _BY["odd14"], FP32_MODES, BOTH, "dense", False, True),
    ConvCase("igemm_clip768", _BY["clip768"], FP32_MODES, BOTH, "dense", False),
    ConvCase("igemm_vox_l1_rows", _BY["vox_l1"], FP32_MODES, BOTH, "rows", False),
    ConvCase("igemm_vox_l1_rowmask", _BY["vox_l1"], FP32_MODES, BOTH, "rowmask", False),
    # conv_halo_rows_kernel (h_4x4, h_320 with the 192-position tile in the forward); h_14 plans conv_dma_kernel split-K
    ConvCase("halo_h_4x4", _BY["h_4x4"], S16, BOTH, "dense", True),
    ConvCase("halo_h_14", _BY["h_14"], S16, BOTH, "dense", False),
    ConvCase("halo_h_320", _BY["h_320"], S16, BOTH, "dense", False),
    ConvCase("dma_h_7x256", _BY["h_7x256"], S16, BOTH, "dense", True, True),
    ConvCase("dma_vox_m_rowmask", _vox("vox_m", 3, 6, 64, 128), S16, BOTH, "rowmask", False),
    ConvCase("pw_256", _BY["pw_256"], S16, BOTH, "dense", True),            # (accumulate: conv_dma_kernel takes it)
    ConvCase("stem_48", _BY["stem_48"], S16, ("fwd",), "dense", False),
    ConvCase("stem_5x5", _BY["stem_5x5"], S16, ("fwd",), "dense", False),
    ConvCase("c64k_32x12", _BY["c64k_32x12"], S16, BOTH, "dense", True),
    ConvCase("c64k_16", _BY["c64k_16"], S16, BOTH, "dense", False),
    ConvCase("s2d_16", _BY["s2d_16"], S16, BOTH, "dense", True),            # forward: conv_dma_kernel; data gradient: conv_s2d_kernel
    ConvCase("s2g_7x8x8", _s2("s2g_7", 7, 8, 8, 128, 64), S16, BOTH, "dense", False),
    ConvCase("s2g_2x4x4", _s2("s2g_2", 2, 4, 4, 192, 64), S16, BOTH, "dense", False),
    # conv_s2g_kernel with a SHORT LAST UNIT: enough output-channel tiles (1,024 channels) that the plan keeps two images per unit - 16 units
    # for 31 images, one image in the last (ns < ipu: slab pieces past the unit, the reused row 0, the r < nrows store predicate)
    ConvCase("s2g_31x4x4_short_unit", _s2("s2g_31", 31, 4, 4, 128, 1024), S16, ("fwd",), "dense", False),
    ConvCase("vox0_3x32", _vox("vox0", 3, 32, 3, 32), S16, ("fwd",), "sitemask", False),
    ConvCase("voxb_5x16", _vox("voxb", 5, 16, 32, 64), S16, ("fwd",), "sitemask", False),
    ConvCase("voxg_3x8", _vox("voxg", 3, 8, 64, 128), S16, BOTH, "sitemask", False),
    ConvCase("voxg_5x4", _vox("voxg", 5, 4, 128, 256), S16, BOTH, "sitemask", False),
    ConvCase("voxg_7x2", _vox("voxg", 7, 2, 256, 512), S16, BOTH, "sitemask", False),
    ConvCase("voxg_1x2", _vox("voxg", 1, 2, 64, 64), S16, BOTH, "sitemask", False),
    # conv_halo2d_kernel: the smallest shape the planner routes there by default in BOTH directions (found with the planner on the CPU:
    # 7 images of 56 x 56, 128 -> 128 channels; 171.5 tiles of 128 positions)
    ConvCase("halo2d_7x56", ("halo2d", 7, (1, 56, 56), 128, 128, (1, 3, 3), 1, (0, 1, 1), "torch"), S16, BOTH, "dense", True),
]
CONV_RUNS = [(cc, store, prec) for cc in CONV_TABLE for store, prec in cc.modes]
# families whose row tile can be partial at all: the others (conv_vox0 6, conv_c64 9, conv_s2d 10, conv_voxb 14) walk bricks that their
# plans only form whole (image heights divide the brick rows - the geometry is refused otherwise -, grids are whole bricks); their edge is
# the persistent workgroup's last brick, which every case here has
FAMILIES_WITH_PARTIAL_TILES = {0, 2, 3, 4, 5, 12, 13, 15}


def plan_mode(store, prec):
    """Plan index of ops._conv_mode for a storage type and a precision mode."""
    return 1 if prec == "bf16x3" else (2 if store != F32 else 0)


def geom_of(case):
    """ops.ConvGeom of a case tuple, as tests.test_gpu_ops.make_case builds it (the planner answers without a GPU)."""
    name, B, grid, cin, cout, k, s, p, layout = case
    ntaps = k[0] * k[1] * k[2]
    strides = (ntaps * cin, cin, 1) if layout == "spconv" else (cin * ntaps, 1, ntaps)
    return ops.ConvGeom(B, grid, cin, 4 if cin == 3 else cin, cout, k, s, p, strides)


def partial_last_tile(g, transposed, code):
    """True when the launch's rows do not fill its last row tile: 128-row tiles (conv_igemm / conv_dma / conv_pw / conv_stem position
    tiles), 64 x the tile field of the halo kernels, whole samples per unit of conv_voxg_kernel, whole images per unit of conv_s2g_kernel
    (one BatchNorm record per unit: images per unit = ceil(B / records), never more than the plan's)."""
    fam, field = code & 255, (code >> 8) & 255
    M = g.M_in if transposed else g.M
    if fam in (3, 5):
        return M % (64 * field) != 0
    if fam == 13:
        return g.B % max((code >> 24) & 127, 1) != 0 or (g.B * g.in_grid[0] ** 3) % 32 != 0
    if fam == 15:
        ipu = -(-g.B // g.num_mtiles[2])
        return ipu > 1 and g.B % ipu != 0
    return fam in FAMILIES_WITH_PARTIAL_TILES and M % 128 != 0


@functools.lru_cache(maxsize=None)
def _conv_ref(cc):
    """Integer data and exact references of one case, computed once on the CPU and shared by its storage types (never modified)."""
    case = cc.case
    x, w, wp, xcl, g = make_case(case, integer=True, seed=51)
    M, Mi = g.M, g.M_in
    r = dict(wp=wp, mask=None, mask_in=None)
    if cc.form == "sitemask":
        B, D = case[1], case[2][0]
        m = _blob_mask(B, D, seed=183 + D, p_empty=0.15) if D > 2 else (torch.rand(B, D, D, D, generator=torch.Generator().manual_seed(7)) < 0.9)
        x, xcl = x * m.float()[:, None], xcl * m.float()[..., None]             # submanifold invariant: inactive sites are exactly zero
        act = m.reshape(M)
    elif cc.form in ("rows", "rowmask"):
        act = torch.rand(M, generator=torch.Generator().manual_seed(9)) < 0.3
        act[:256] = False                                                       # two fully inactive 128-row tiles
    else:
        act = None
    if act is not None:
        mpad = torch.zeros((M + 31) // 32 * 32, dtype=torch.uint8)
        mpad[:M] = act.to(torch.uint8)
        r.update(mask=mpad, act=act)
    xr = x.clone().requires_grad_()
    y = F.conv3d(xr, w, stride=case[6], padding=case[7])
    dy = ints(tuple(y.shape), -2, 2, 53)
    if cc.form == "sitemask":
        dy = dy * act.view(case[1], 1, *case[2]).float()
    r.update(xcl=xcl, y=cl3(y.detach()), dy=cl3(dy))
    if "dgrad" in cc.dirs:
        y.backward(dy)
        r.update(dx=cl3(xr.grad), base=ints(tuple(cl3(xr.grad).shape), -5, 5, 59), yv=ints(tuple(cl3(xr.grad).shape), -3, 3, 67))
    return r


@pytest.mark.parametrize("cc,store,prec", CONV_RUNS, ids=[f"{cc.name}-{IDS[s]}-{p}" for cc, s, p in CONV_RUNS])
def test_conv_forward_and_data_gradient(cc, store, prec):
    r = _conv_ref(cc)
    geom = geom_of(cc.case)
    cin_s, cout = geom.cin_stored, geom.cout
    M, Mi = geom.M, geom.M_in
    mode = plan_mode(store, prec)
    s2g = (geom.kernel_family[(False, mode)] & 255) == 15
    atol = 1e-3 if store == F32 else (1e-1 if s2g else 1e-2)
    # tri_conv_dgrad_bn: the data gradient that also takes the BatchNorm-backward sums of relu(bn1(y)) (conv_c64_kernel, 16- / 32-wide images)
    dgrad_bn = "dgrad" in cc.dirs and cc.form == "dense" and (geom.kernel_family[(True, mode)] & 255) == 9 and geom.in_grid[2] <= 32
    bn_scale, bn_shift = torch.linspace(-1.0, 1.5, geom.cin), torch.linspace(0.75, -0.5, geom.cin)
    bias = ints((cout,), -2, 2, 4)

    def body(g):
        out = {}
        wp = g.put(r["wp"])
        x = g.put(r["xcl"].to(store))
        mask = g.put(r["mask"])
        packed = ops.pack_weight(wp, geom, prec, storage=store)
        kw = {}
        if cc.form == "rows":
            rows = ops.mask_compact(mask, M)
            kw = dict(rows=rows)
            out["row_count"] = rows[1]
        elif cc.form in ("rowmask", "sitemask"):
            kw = dict(row_mask=mask)
        if cc.form in ("rows", "sitemask"):                                     # rows outside the list / of inactive sites are not written
            kw["out"] = g.put(torch.full((geom.B, *geom.out_grid, cout), 777.0, dtype=store))
        if "fwd" in cc.dirs:
            out["y"], out["stats"] = ops.conv_fwd(x, geom, packed, want_stats=True, **kw)
            if cc.epi:                                                          # bias + ReLU epilogue (test_conv_fwd_mask_bias_act_stats): the bias vector between bands too
                out["y_epi"] = ops.conv_fwd(x, geom, packed, bias=g.put(bias), act=1)
        if "dgrad" in cc.dirs:
            tp = ops.pack_weight(wp, geom, prec, transposed=True, storage=store)
            dy = g.put(r["dy"].to(store))
            kd = {k: v for k, v in kw.items() if k != "out"}
            if cc.form in ("rows", "sitemask"):
                kd["out"] = g.put(torch.full((geom.B, *geom.in_grid, cin_s), 555.0, dtype=store))
            out["dx"] = ops.conv_dgrad(dy, geom, tp, **kd)
            if cc.acc:
                out["dx_acc"] = ops.conv_dgrad(dy, geom, tp, out=g.put(r["base"].to(store)), accumulate=True)
            if dgrad_bn:
                co = ops.BNCoeffs(geom.cin, DEV)
                co.scale.copy_(bn_scale)
                co.shift.copy_(bn_shift)
                out["dx_bn"], out["part"] = ops.conv_dgrad(dy, geom, tp, bn_sums=(g.put(r["yv"].to(store)), co, None))
        return out

    got = twice(body)
    act = r.get("act")
    if "fwd" in cc.dirs:
        y, ref = got["y"].reshape(M, cout), r["y"].to(store).reshape(M, cout)
        if cc.form == "dense":
            assert torch.equal(y, ref), f"forward: max abs diff {(y.float() - ref.float()).abs().max().item()}"
            exact = ref.double()
        elif cc.form == "rowmask":
            ref = (r["y"].reshape(M, cout) * act[:, None].float()).to(store)
            assert torch.equal(y, ref)
            exact = ref.double()
        else:
            assert torch.equal(y[act], ref[act]) and bool((y[~act] == 777.0).all()), "forward: active rows / untouched inactive rows"
            exact = ref[act].double()
        col_sums_ok(got["stats"], exact, atol)
        if cc.epi:
            assert torch.equal(got["y_epi"].reshape(M, cout), F.relu(r["y"].reshape(M, cout) + bias).to(store))
    if "dgrad" in cc.dirs:
        dx, ref = got["dx"].reshape(Mi, cin_s), r["dx"].to(store).reshape(Mi, cin_s)
        if cc.form == "dense":
            assert torch.equal(dx, ref), f"data gradient: max abs diff {(dx.float() - ref.float()).abs().max().item()}"
        elif cc.form == "rowmask":
            assert torch.equal(dx, (r["dx"].reshape(Mi, cin_s) * act[:, None].float()).to(store))
        else:
            assert torch.equal(dx[act], ref[act]) and bool((dx[~act] == 555.0).all())
        if cc.acc:
            assert torch.equal(got["dx_acc"], (r["dx"] + r["base"]).to(store))
        if dgrad_bn:
            assert torch.equal(got["dx_bn"].reshape(Mi, cin_s), ref)
            gm = ref.double() * (r["yv"].reshape(Mi, cin_s) * bn_scale + bn_shift > 0).double()
            st = got["part"].double().sum(0)
            np.testing.assert_allclose(st[0].numpy(), gm.sum(0).numpy(), rtol=1e-6, atol=1e-2)
            np.testing.assert_allclose(st[1].numpy(), (gm * r["yv"].reshape(Mi, cin_s).double()).sum(0).numpy(), rtol=1e-6, atol=1e-2)
    if cc.form == "rows":
        assert int(got["row_count"]) == int(act.sum())


# ================================================================================================ weight gradient
def _krow(name):
    c = {k[0]: k for k in KROW_CASES}[name]
    return (c[0], c[1], c[2], c[3], c[4], (1, 3, 3), 1, (0, 1, 1), "torch")


WGRAD_SINGLE = [_krow(n) for n in ("k4_512", "k8_h6", "k7_512", "k12_h5", "k16_128_192")] + [_s2("s2k_7x8x8", 7, 8, 8, 128, 64)]
STEM_WGRAD = [(3, 32, 7), (2, 32, 3)]


def wgrad_geometries():
    """(case tuple, storage) of every weight-gradient launch below, for the planner's family check on the CPU."""
    for case in WGRAD_SINGLE + WGRAD_JOB_CASES["mixed"] + [_vox("vox0", 3, 32, 3, 32)]:
        for store, _ in STORE16:
            yield case, store
    for store in STORES:
        yield _BY["vox_l1"], store
    for N, HW, k in STEM_WGRAD:
        yield ("stem", N, (1, HW, HW), 3, 64, (1, k, k), 2, (0, k // 2, k // 2), "torch"), F16


@functools.lru_cache(maxsize=None)
def _wgrad_ref(case, seed, sign=False):
    x, w, wp, xcl, g = make_case(case, integer=True, seed=seed)
    dy = ints((g.B, *g.out_grid, g.cout), -2, 2, seed + 10)
    if sign:
        x, xcl, dy = x.sign(), xcl.sign(), dy.sign()
    wr = w.clone().requires_grad_()
    F.conv3d(x, wr, stride=case[6], padding=case[7]).backward(cf3(dy))
    ref = wr.grad.permute(0, 2, 3, 4, 1).contiguous() if case[8] == "spconv" else wr.grad
    return xcl, dy, wp, ref


@pytest.mark.parametrize("store,prec", STORE16, ids=[IDS[s] for s, _ in STORE16])
@pytest.mark.parametrize("case", WGRAD_SINGLE, ids=[c[0] for c in WGRAD_SINGLE])
def test_weight_gradient_single_layer_and_batch(case, store, prec):
    """test_conv_wgrad_krow_integer_exact: the kernel-row slab kernel alone (tri_conv_wgrad, exact-size workspace) and as two jobs of one
    shared launch (exact-size slabs), bit-exact on integer data."""
    refs = [_wgrad_ref(case, 40 + rep) for rep in range(2)]
    geom = geom_of(case)

    def body(g):
        out = {}
        batch = ops.WgradBatch(torch.device(DEV), group_jobs=True)
        for rep, (xcl, dy, wp, _) in enumerate(refs):
            xd, dyd, like = g.put(xcl.to(store)), g.put(dy.to(store)), g.put(wp)
            if rep == 0:
                out["alone"] = ops.conv_wgrad(xd, dyd, geom, like, prec)
            out[f"job{rep}"] = ops.conv_wgrad(xd, dyd, geom, like, prec, out_scale=0.5 if rep else 1.0, batch=batch)
        batch.flush()
        return out

    got = twice(body)
    assert torch.equal(got["alone"], refs[0][3]) and torch.equal(got["job0"], refs[0][3]) and torch.equal(got["job1"], refs[1][3] * 0.5)


@pytest.mark.parametrize("store,prec", STORE16, ids=[IDS[s] for s, _ in STORE16])
def test_weight_gradient_mixed_job_group(store, prec):
    """test_wgrad_jobs_share_one_partial_launch[mixed]: ten layers of three kernel families queued in one WgradBatch."""
    cases = WGRAD_JOB_CASES["mixed"]
    refs = [_wgrad_ref(c, 300 + i) for i, c in enumerate(cases)]

    def body(g):
        batch = ops.WgradBatch(torch.device(DEV), group_jobs=True)
        out = {}
        for i, (c, (xcl, dy, wp, _)) in enumerate(zip(cases, refs)):
            out[f"dw{i}"] = ops.conv_wgrad(g.put(xcl.to(store)), g.put(dy.to(store)), geom_of(c), g.put(wp), prec,
                                           out_scale=0.5 if i % 2 else 1.0, batch=batch)
        assert len(batch.jobs) + len(batch.descs) == len(cases)
        batch.flush()
        return out

    got = twice(body)
    for i, (_, _, _, ref) in enumerate(refs):
        assert torch.equal(got[f"dw{i}"], ref * (0.5 if i % 2 else 1.0)), f"job {i}"


@pytest.mark.parametrize("store", STORES, ids=[IDS[s] for s in STORES])
def test_weight_gradient_over_a_compact_row_list(store):
    """test_conv_wgrad_over_a_compact_row_list / test_wgrad_jobs_over_compact_row_lists at vox_l1: the contraction over the active sites
    only, alone and as a job; dOut holds 7.0 in the rows of inactive sites (never visited)."""
    case, prec = _BY["vox_l1"], PREC[store]
    x, w, wp, xcl, geom = make_case(case, integer=True, seed=81)
    M = geom.M
    act = torch.rand(M, generator=torch.Generator().manual_seed(1)) < 0.13
    mpad = torch.zeros((M + 31) // 32 * 32, dtype=torch.uint8)
    mpad[:M] = act.to(torch.uint8)
    dy = ints((M, geom.cout), -2, 2, 84) * act[:, None].float()
    wr = w.clone().requires_grad_()
    F.conv3d(x, wr, padding=1).backward(cf3(dy.view(geom.B, *geom.out_grid, geom.cout)))
    ref = wr.grad.permute(0, 2, 3, 4, 1).contiguous()
    junk = dy.clone()
    junk[~act] = 7.0

    def body(g):
        xd, dyd, like = g.put(xcl.to(store)), g.put(junk.view(geom.B, *geom.out_grid, geom.cout).to(store)), g.put(wp)
        rows = ops.mask_compact(g.put(mpad), M)
        batch = ops.WgradBatch(torch.device(DEV), group_jobs=True)
        out = dict(alone=ops.conv_wgrad(xd, dyd, geom, like, prec, rows=rows), job=ops.conv_wgrad(xd, dyd, geom, like, prec, rows=rows, batch=batch))
        batch.flush()
        return out

    got = twice(body)
    assert torch.equal(got["alone"], ref) and torch.equal(got["job"], ref)


@pytest.mark.parametrize("store,prec", STORE16, ids=[IDS[s] for s, _ in STORE16])
def test_weight_gradient_level0_brick_form(store, prec):
    """test_voxel_level0_weight_gradient_brick_kernel at (3, 32): sign data, exact, alone and through a WgradBatch."""
    B, V = 3, 32
    case = _vox("vox0", B, V, 3, 32)
    x, w, wp, xcl, geom = make_case(case, integer=True, seed=171)
    assert geom.wgrad_brick
    m = _blob_mask(B, V, seed=173)
    mf = m.float()
    x, xcl = (x * mf[:, None]).sign(), (xcl * mf[..., None]).sign()
    M = B * V ** 3
    mask = torch.zeros((M + 31) // 32 * 32, dtype=torch.uint8)
    mask[:M] = m.reshape(M).to(torch.uint8)
    dy = ints((B, V, V, V, 32), -1, 1, 175) * mf[..., None]
    wr = w.clone().requires_grad_()
    F.conv3d(x, wr, padding=1).backward(cf3(dy))
    ref = wr.grad.permute(0, 2, 3, 4, 1).contiguous()
    junk = dy.clone().view(M, 32)
    junk[~m.reshape(M)] = 9.0                                       # rows of inactive sites are never read

    def body(g):
        xd, dyd, like, mk = g.put(xcl.to(store)), g.put(junk.view(B, V, V, V, 32).to(store)), g.put(wp), g.put(mask)
        batch = ops.WgradBatch(torch.device(DEV))
        out = dict(alone=ops.conv_wgrad(xd, dyd, geom, like, prec, row_mask=mk, out_scale=0.5),
                   job=ops.conv_wgrad(xd, dyd, geom, like, prec, row_mask=mk, batch=batch))
        batch.flush()
        return out

    got = twice(body)
    assert torch.equal(got["alone"], ref * 0.5) and torch.equal(got["job"], ref)


@pytest.mark.parametrize("store,prec", STORE16, ids=[IDS[s] for s, _ in STORE16])
@pytest.mark.parametrize("N,HW,k", STEM_WGRAD)
def test_stem_weight_gradient_with_the_bn_apply_folded_in(N, HW, k, store, prec):
    """test_stem_weight_gradient_with_the_bn_apply_pass_folded_in: ops.maxpool_bn_bwd_wgrad bit-identical to ops.maxpool_bn_bwd +
    ops.conv_wgrad (both inside the bands), alone and through a batch, and within 2e-2 of torch's conv2d_weight."""
    case = ("stem", N, (1, HW, HW), 3, 64, (1, k, k), 2, (0, k // 2, k // 2), "torch")
    x, w, wp, xcl, geom = make_case(case, integer=False, seed=41)
    gen = torch.Generator().manual_seed(43)
    C, H, W = 64, HW // 2, HW // 2
    y = (torch.randn(N, 1, H, W, C, generator=gen) * 1.5 + 0.2).to(store)
    gamma, beta = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.3
    M = N * H * W
    yf = y.float().view(M, C)
    stats = torch.stack([yf.double().sum(0).float(), (yf.double() ** 2).sum(0).float()]).view(1, 2, C)
    dpool = torch.randn(N, 1, H // 2, W // 2, C, generator=gen).to(store)

    def body(g):
        yd, gm, bt, xd, like = g.put(y), g.put(gamma), g.put(beta), g.put(xcl.to(store)), g.put(wp)
        co = ops.bn_finalize(g.put(stats), C, gm, bt, None, None, None, count_host=M)
        pooled, arg = ops.maxpool2d_fwd(yd, want_arg=True, bn=co)
        dp = g.put(dpool)
        dy, dg_a, db_a = ops.maxpool_bn_bwd(yd, arg, dp, co, gm, out_scale=0.5)
        dw_a = ops.conv_wgrad(xd, dy, geom, like, prec, out_scale=0.5)
        dw_b, dg_b, db_b = ops.maxpool_bn_bwd_wgrad(xd, yd, arg, dp, co, gm, geom, like, prec, out_scale=0.5)
        batch = ops.WgradBatch(torch.device(DEV))
        dw_c, _, _ = ops.maxpool_bn_bwd_wgrad(xd, yd, arg, dp, co, gm, geom, like, prec, out_scale=0.5, batch=batch)
        batch.flush()
        return dict(dy=dy, dg_a=dg_a, db_a=db_a, dw_a=dw_a, dw_b=dw_b, dg_b=dg_b, db_b=db_b, dw_c=dw_c)

    got = twice(body)
    assert torch.equal(got["dg_a"], got["dg_b"]) and torch.equal(got["db_a"], got["db_b"])
    assert torch.equal(got["dw_a"], got["dw_b"]) and torch.equal(got["dw_a"], got["dw_c"])
    ref = torch.nn.grad.conv2d_weight(x[:, :, 0].float(), w[:, :, 0].shape, cf3(got["dy"].float())[:, :, 0], stride=2, padding=k // 2) * 0.5
    np.testing.assert_allclose(got["dw_b"][:, :, 0].numpy(), ref.numpy(), rtol=2e-2, atol=2e-2 * float(ref.abs().max()))


# ================================================================================================ BatchNorm and pooling passes
# references and bounds: tests/bn_reference.py, used as tests/test_gpu_bn_family.py uses them (test_image_tower_layer,
# test_bn_bwd_regime_edges, test_stem_bn_relu_maxpool_forward_and_backward, test_voxel_level_forward_and_backward,
# test_avgpool_viewmax_against_float64); row counts that do not fill the last block
OUT_SCALE = 1.0 / 4096


def _records(y, rows=None, tile=128):
    from tests.test_gpu_bn_family import records
    return records(y, rows, tile)


def _co(d, prefix):
    return R.SimpleNamespace(mean=d[prefix + "mean"].to(DEV), invstd=d[prefix + "invstd"].to(DEV), scale=d[prefix + "scale"].to(DEV),
                             shift=d[prefix + "shift"].to(DEV))


def _co_out(out, prefix, co):
    out.update({prefix + "mean": co.mean, prefix + "invstd": co.invstd, prefix + "scale": co.scale, prefix + "shift": co.shift})


@pytest.mark.parametrize("store", STORES, ids=[IDS[s] for s in STORES])
@pytest.mark.parametrize("M,C", [(4111, 64), (1037, 128), (300, 512), (777, 512)])
def test_batchnorm_passes(M, C, store):
    """bn_finalize (with running statistics), bn_act plain / identity residual / down-sample residual, bn_bwd final / relu / relu_out (three
    passes, or tri_bn_bwd_small at M <= 512), bn_bwd with a row mask and a device count, bn_bwd_pair."""
    rp = R.Report()
    case = f"guard {M}x{C} {IDS[store]}"
    inp = R.make_inputs(M, C, store, seed=M + C, device=DEV, grad_scale=64.0 if store != F32 else 1.0)
    msk = R.make_inputs(M, C, store, seed=M + C + 1, device=DEV, row_p=0.4)
    gen = torch.Generator().manual_seed(C)
    gamma_b, beta_b = (torch.rand(C, generator=gen) + 0.5).to(DEV), (torch.randn(C, generator=gen) * 0.3).to(DEV)
    rm0, rv0 = (torch.randn(C, generator=gen) * 0.1).to(DEV), (torch.rand(C, generator=gen) + 0.5).to(DEV)
    rec, rec_b, rec_m = _records(inp.y), _records(inp.res), _records(msk.y, msk.rows)

    def body(g):
        out = {}
        y, gr, res, gamma, beta = g.put(inp.y), g.put(inp.g), g.put(inp.res), g.put(inp.gamma), g.put(inp.beta)
        rm, rv, nbt = g.put(rm0), g.put(rv0), g.put(torch.zeros((), dtype=torch.long))
        co = ops.bn_finalize(g.put(rec), C, gamma, beta, rm, rv, nbt, count_host=M)
        gb_, bb_ = g.put(gamma_b), g.put(beta_b)
        cob = ops.bn_finalize(g.put(rec_b), C, gb_, bb_, None, None, None, count_host=M)
        _co_out(out, "co_", co)
        _co_out(out, "cob_", cob)
        out.update(rm=rm, rv=rv, nbt=nbt)
        out["act_plain"] = ops.bn_act(y, co, relu=True)
        out["act_identity"] = ops.bn_act(y, co, relu=True, res=res)
        out["act_downsample"] = ops.bn_act(y, co, relu=True, res=res, res_co=cob)
        for mode, kw in (("final", {}), ("relu", dict(relu=True)), ("relu_out", dict(relu_out=out["act_identity"]))):
            gm = g.put(torch.zeros_like(inp.g)) if mode == "relu_out" else None
            dy, dgam, dbet = ops.bn_bwd(y, gr, co, gamma, count_host=M, inplace=False, out_scale=OUT_SCALE, g_masked=gm, **kw)
            out.update({f"{mode}_dy": dy, f"{mode}_dgamma": dgam, f"{mode}_dbeta": dbet, f"{mode}_gm": gm})
        gm = g.put(torch.zeros_like(inp.g))
        pair = ops.bn_bwd_pair(y, co, gamma, res, cob, gb_, gr, out["act_downsample"], M, g_masked=gm, out_scale=OUT_SCALE)
        out.update({f"pair{i}": t for i, t in enumerate(pair)})
        out["pair_gm"] = gm
        # row mask + device-side count; the gradient holds 123.0 in the inactive rows
        ym, rows, gam_m, bet_m = g.put(msk.y), g.put(msk.rows), g.put(msk.gamma), g.put(msk.beta)
        cnt = ops.mask_count(rows, M)
        com = ops.bn_finalize(g.put(rec_m), C, gam_m, bet_m, None, None, None, count_dev=cnt)
        _co_out(out, "com_", com)
        g2 = msk.g.clone()
        g2[~msk.rows[:M].bool()] = 123.0
        dy, dgam, dbet = ops.bn_bwd(ym, g.put(g2), com, gam_m, count_dev=cnt, row_mask=rows, inplace=False, out_scale=0.5)
        out.update(mask_dy=dy, mask_dgamma=dgam, mask_dbeta=dbet, count=cnt)
        return out

    got = {k: v.to(DEV) for k, v in twice(body).items()}
    st = R.bn_stats(inp.y, inp.gamma, inp.beta, running_mean=rm0, running_var=rv0)
    stb = R.bn_stats(inp.res, gamma_b, beta_b)
    R.check_stats(rp, case, _co(got, "co_"), st, running=(got["rm"], got["rv"]))
    R.check_stats(rp, case + " shortcut", _co(got, "cob_"), stb)
    assert int(got["nbt"]) == 1 and int(got["count"]) == int(msk.rows.sum())
    for name, rkw in (("plain", {}), ("identity", dict(res=inp.res)), ("downsample", dict(res=inp.res, res_st=stb))):
        ref, bound, _, _ = R.bn_act(inp.y, st, relu=True, store=store, **rkw)
        R.check(rp, "elementwise", case, f"bn_act {name}", got[f"act_{name}"], ref, bound)
    for mode in ("final", "relu", "relu_out"):
        b = R.bn_bwd(inp.y, inp.g, st, inp.gamma, mode=mode, relu_out=got["act_identity"], out_scale=OUT_SCALE, store=store)
        R.check_bwd(rp, f"{case} bn_bwd {mode}", b, got[f"{mode}_dy"], got[f"{mode}_dgamma"], got[f"{mode}_dbeta"], g_masked=got.get(f"{mode}_gm"))
    a = R.bn_bwd(inp.y, inp.g, st, inp.gamma, mode="relu_out", relu_out=got["act_downsample"], out_scale=OUT_SCALE, store=store)
    R.check_bwd(rp, f"{case} bn_bwd_pair a", a, got["pair0"], got["pair1"], got["pair2"], g_masked=got["pair_gm"])
    bb = R.bn_bwd(inp.res, a.g_masked, stb, gamma_b, mode="final", out_scale=OUT_SCALE, store=store)
    R.check_bwd(rp, f"{case} bn_bwd_pair b", bb, got["pair3"], got["pair4"], got["pair5"])
    stm = R.bn_stats(msk.y, msk.gamma, msk.beta, rows=msk.rows)
    R.check_stats(rp, case + " rowmask", _co(got, "com_"), stm)
    bm = R.bn_bwd(msk.y, msk.g, stm, msk.gamma, mode="final", rows=msk.rows, out_scale=0.5, store=store)
    R.check_bwd(rp, case + " rowmask", bm, got["mask_dy"], got["mask_dgamma"], got["mask_dbeta"], rows=msk.rows, inactive=0.0)


@pytest.mark.parametrize("store", STORES, ids=[IDS[s] for s in STORES])
def test_stem_pool_passes(store):
    """maxpool2d_fwd with BatchNorm + ReLU folded in, maxpool2d_bwd, maxpool_bn_bwd from the full-resolution tensors (tri_maxpool_bn_bwd_reduce)
    and from the pooled ones (tri_maxpool_bn_bwd_reduce_pooled, 16-bit storage) with tri_maxpool_bn_bwd_apply: 24 images of 62 x 62.
    The sums bound of bn_reference (1e-4 of the absolute terms) is a bound of fp32 SUMMATION; the full-resolution form rounds the routed
    gradient to the storage type per position (bn_pool.hip says so where it introduces the pooled form), half an ulp of bf16 = 2^-9 per
    term, independent: ~2^-9 / sqrt(n) of the absolute terms over n routed positions per channel.  That is inside 1e-4 from n ~ 400 with
    no margin (measured at 3 images of 20 x 20, n = 300: 3.6 x the bound, bf16 only), so the shape gives n = 23,064 (an eighth of it).
    FOLLOW-UP: bn_reference's sums bound has no term for that per-position storage rounding (eps_s / 2 per routed term of the
    full-resolution form in 16-bit storage); with it the bound would hold at any n and this case could shrink to a few hundred rows."""
    N, H, W, C = 24, 62, 62, 64
    M = N * H * W
    rp = R.Report()
    case = f"guard stem {N}x{H}x{W}x{C} {IDS[store]}"
    inp = R.make_inputs(M, C, store, seed=11, device=DEV, grad_scale=64.0 if store != F32 else 1.0)
    rec = _records(inp.y)
    Mo = N * (H // 2) * (W // 2)
    dpool = torch.randn(Mo, C, generator=torch.Generator().manual_seed(12)) * (64.0 if store != F32 else 1.0)
    dpool[:, 2:4] = torch.randn(Mo, 2, generator=torch.Generator().manual_seed(13))
    dpool = dpool.to(store).reshape(N, 1, H // 2, W // 2, C)

    def body(g):
        y, gamma, beta = g.put(inp.y.reshape(N, 1, H, W, C)), g.put(inp.gamma), g.put(inp.beta)
        co = ops.bn_finalize(g.put(rec), C, gamma, beta, None, None, None, count_host=M)
        pooled, arg = ops.maxpool2d_fwd(y, bn=co)
        dp = g.put(dpool)
        out = dict(pooled=pooled, arg=arg, dx=ops.maxpool2d_bwd(arg, dp, y.shape))
        _co_out(out, "co_", co)
        for with_pooled in (False, True):
            dy, dgam, dbet = ops.maxpool_bn_bwd(y, arg, dp, co, gamma, out_scale=OUT_SCALE, pooled=pooled if with_pooled else None)
            out.update({f"dy{int(with_pooled)}": dy, f"dgamma{int(with_pooled)}": dgam, f"dbeta{int(with_pooled)}": dbet})
        return out

    got = {k: v.to(DEV) for k, v in twice(body).items()}
    y = inp.y.reshape(N, 1, H, W, C)
    st = R.bn_stats(inp.y, inp.gamma, inp.beta)
    R.check_stats(rp, case, _co(got, "co_"), st)
    ref = R.stem_pool(y, st, store=store)
    R.check(rp, "elementwise", case, "pooled", got["pooled"].reshape(-1, C), ref.pooled.reshape(-1, C), ref.b_pooled.reshape(-1, C))
    tap = got["arg"].reshape(ref.tap.shape).long()
    differs = tap != ref.tap
    chosen = torch.gather(ref.z, 3, tap.unsqueeze(3)).squeeze(3)
    assert int(tap.max()) <= 8 and not bool((differs & ~(chosen >= ref.pooled - 2 * ref.b_z.max(3).values)).any()), (case, "tap map")
    dp = dpool.to(DEV)
    rb = R.stem_pool(y, st, store=store, dpool=dp, tap=got["arg"])
    b = R.bn_bwd(y, rb.g, st, inp.gamma, mode="final", out_scale=OUT_SCALE, store=store, undecided=rb.undecided, g_unmasked=rb.g_unmasked)
    mass = R.stem_pool(y, st, store=store, dpool=dp.abs(), tap=got["arg"]).g_unmasked.reshape(-1, C)
    R.check(rp, "elementwise", case, "maxpool2d_bwd", got["dx"].reshape(-1, C), rb.g_unmasked.reshape(-1, C),
            R.eps_of(store) * rb.g_unmasked.abs().reshape(-1, C) + R.tiny_of(store) + 8 * R.U32 * mass)
    for wp_ in (0, 1):
        R.check_bwd(rp, f"{case} maxpool_bn_bwd pooled={wp_}", b, got[f"dy{wp_}"], got[f"dgamma{wp_}"], got[f"dbeta{wp_}"])


VOXEL_LEVELS = [(5, 16, 32, True), (5, 16, 64, False), (3, 8, 128, False), (3, 4, 512, False)]      # B, D, C, level-0 form (keep_inactive + rows)


@pytest.mark.parametrize("store", STORES, ids=[IDS[s] for s in STORES])
@pytest.mark.parametrize("B,D,C,keep", VOXEL_LEVELS, ids=[f"{b}x{d}^3x{c}{'-keep' if k else ''}" for b, d, c, k in VOXEL_LEVELS])
def test_voxel_level_passes(B, D, C, keep, store):
    """bn_relu_pool3d_fwd and ops.pool3d_bn_bwd fused and unfused: above 16,384 rows tri_pool3d_bwd_route_rows_reduce + tri_bn_bwd_apply(_rows)
    and tri_pool3d_bwd_route_rows + tri_bn_bwd_rows / the three bn_bwd passes; below, tri_pool3d_bwd_route_reduce and tri_pool3d_bwd_route +
    bn_bwd (tri_bn_bwd_small at 192 rows).  Inactive rows of y and of the pooled gradient hold NaN; sample 1 is empty."""
    M, Mo = B * D ** 3, B * (D // 2) ** 3
    rp = R.Report()
    case = f"guard voxel {B}x{D}^3x{C} {IDS[store]}"
    gen = torch.Generator().manual_seed(D + C)
    live = torch.rand(B, D, D, D, generator=gen) < 0.2
    live[1] = False
    live[0, :2, :2, :2] = True
    gs = 64.0 if store != F32 else 1.0
    inp = R.make_inputs(M, C, store, seed=D + C, device=DEV, grad_scale=gs, live=live)
    rec = _records(inp.y, inp.rows)
    live_out = R._windows3d(live.reshape(B, D, D, D, 1), B, D).any(4).reshape(-1).to(DEV)
    dp = torch.randn(Mo, C, generator=gen) * gs
    dp[:, 2:4] = torch.randn(Mo, 2, generator=gen)
    dp = dp.to(DEV)
    dp[~live_out] = float("nan")
    dp = dp.to(store).reshape(B, D // 2, D // 2, D // 2, C)

    def body(g):
        y, rows_m, gamma, beta = g.put(inp.y.reshape(B, D, D, D, C)), g.put(inp.rows), g.put(inp.gamma), g.put(inp.beta)
        rows = ops.mask_compact(rows_m, M)
        cnt = rows[1]
        co = ops.bn_finalize(g.put(rec), C, gamma, beta, None, None, None, count_dev=cnt)
        pooled, mask_out = ops.bn_relu_pool3d_fwd(y, co, rows_m, B, D, C)
        rows_out = ops.mask_compact(mask_out, Mo)
        out = dict(pooled=pooled, mask_out=mask_out, count=cnt)
        _co_out(out, "co_", co)
        dpd = g.put(dp)
        for fused in (True, False):
            dy, dgam, dbet = ops.pool3d_bn_bwd(y, co, rows_m, pooled, dpd, B, D, C, gamma, cnt, out_scale=OUT_SCALE, fused=fused,
                                               keep_inactive=keep, rows=rows if keep else None, rows_out=rows_out)
            if keep:                                          # level 0 leaves the inactive rows of dy unwritten: compare the active ones
                dy = dy.reshape(M, C)[inp.rows[:M].bool()]
            out.update({f"dy{int(fused)}": dy, f"dgamma{int(fused)}": dgam, f"dbeta{int(fused)}": dbet})
        return out

    got = {k: v.to(DEV) for k, v in twice(body).items()}
    y = inp.y.reshape(B, D, D, D, C)
    st = R.bn_stats(inp.y, inp.gamma, inp.beta, rows=inp.rows)
    R.check_stats(rp, case, _co(got, "co_"), st)
    ref = R.pool3d(y, st, inp.rows, B, D, store=store)
    R.check(rp, "elementwise", case, "pooled", got["pooled"].reshape(-1, C), ref.pooled.reshape(-1, C), ref.b_pooled.reshape(-1, C))
    assert torch.equal(got["mask_out"][:Mo].bool(), ref.mask_out) and not bool(got["mask_out"][Mo:].any()) and torch.equal(ref.mask_out, live_out)
    rb = R.pool3d(y, st, inp.rows, B, D, store=store, pooled=got["pooled"], dpooled=dp)
    b = R.bn_bwd(y, rb.g, st, inp.gamma, mode="final", rows=inp.rows, out_scale=OUT_SCALE, store=store, undecided=rb.undecided, g_unmasked=rb.g_abs)
    for fused in (1, 0):
        dy = got[f"dy{fused}"]
        if keep:
            full = torch.zeros(M, C, dtype=store, device=DEV)
            full[inp.rows[:M].bool()] = dy
            dy = full
        R.check_bwd(rp, f"{case} pool3d_bn_bwd fused={fused}", b, dy, got[f"dgamma{fused}"], got[f"dbeta{fused}"], rows=inp.rows,
                    inactive=None if keep else 0.0)


@pytest.mark.parametrize("store", STORES, ids=[IDS[s] for s in STORES])
def test_avgpool_viewmax_passes(store):
    B, V, H, C = 3, 6, 3, 512
    gen = torch.Generator().manual_seed(B + H)
    x = torch.randint(-128, 129, (B, V, H, H, C), generator=gen).float() / 64
    x[:, 1], x[:, 4], x[:, V - 1] = x[:, 0], x[:, 0], x[:, 0]
    x = x.reshape(B * V, 1, H, H, C).to(store)
    dout = torch.randn(B, C, generator=gen)

    def body(g):
        xd = g.put(x)
        out, arg = ops.avgpool_viewmax_fwd(xd, B, V)
        return dict(out=out, arg=arg, dx=ops.avgpool_viewmax_bwd(g.put(dout), arg, xd.shape, B, V, dtype=store, scale=64.0))

    got = {k: v.to(DEV) for k, v in twice(body).items()}
    rp = R.Report()
    ref, rarg, bound, means, rdx = R.avgpool_viewmax(x.to(DEV), B, V, dout=dout.to(DEV), scale=64.0)
    assert torch.equal(got["arg"].long(), rarg)
    R.check(rp, "elementwise", "guard viewmax", "out", got["out"], ref, bound)
    R.check(rp, "elementwise", "guard viewmax", "dx", got["dx"].reshape(-1, C), rdx.reshape(-1, C),
            R.eps_of(store) * rdx.abs().reshape(-1, C) + R.tiny_of(store) + 8 * R.U32 * rdx.abs().reshape(-1, C))


# ================================================================================================ heads, text tower, loss, optimizer, staging
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("M,K,N", [(19, 768, 512), (1, 128, 128)])
def test_linear_small(M, K, N, act):
    """test_linear_small_matches_torch: float64 reference, 2e-5 (bf16x3) / 3e-2 (bf16); the one-launch backward equals the weight-gradient
    entry point alone."""
    f = {0: lambda v: v, 1: torch.relu, 2: torch.tanh}[act]
    gen = torch.Generator().manual_seed(5)
    x, w, b = torch.randn(M, K, generator=gen), torch.randn(N, K, generator=gen) / np.sqrt(K), torch.randn(N, generator=gen)
    dout = torch.randn(M, N, generator=gen)
    ref = f(x.double() @ w.double().t() + b.double())
    for precision, tol in (("bf16x3", 2e-5), ("bf16", 3e-2)):
        def body(g):
            xd, wd, bd, dd = g.put(x), g.put(w), g.put(b), g.put(dout)
            out = ops.linear_small_fwd(xd, wd, bd, act, precision)
            dx, dw, db = ops.linear_small_bwd(xd, wd, out, dd, act, precision)
            _, dw1, db1 = ops.linear_small_bwd(xd, wd, out, dd, act, precision, need_dx=False)
            return dict(out=out, dx=dx, dw=dw, db=db, dw1=dw1, db1=db1)

        got = twice(body)
        np.testing.assert_allclose(got["out"].numpy(), ref.numpy(), atol=tol, rtol=tol)
        o = got["out"].double()
        dpre = dout.double() * {0: torch.ones_like(o), 1: (o > 0).double(), 2: 1 - o * o}[act]
        np.testing.assert_allclose(got["dx"].numpy(), (dpre @ w.double()).numpy(), atol=tol, rtol=tol)
        np.testing.assert_allclose(got["dw"].numpy(), (dpre.t() @ x.double()).numpy(), atol=tol * 20, rtol=tol)
        np.testing.assert_allclose(got["db"].numpy(), dpre.sum(0).numpy(), atol=tol * 4, rtol=tol)
        assert torch.equal(got["dw1"], got["dw"]) and torch.equal(got["db1"], got["db"])


@pytest.mark.parametrize("precision,tol", [("bf16x3", 2e-5), ("bf16", 2e-2), ("f16", 2e-3)])
@pytest.mark.parametrize("B,L", [(19, 7), (1, 1)])
def test_gru_recurrence(precision, tol, B, L):
    """test_gru_recurrence_matches_explicit_equations, plus tri_gru_bias_grads = the column sums of gru_bwd's per-chunk bias gradients."""
    gen = torch.Generator().manual_seed(3)
    xproj = torch.randn(L, B, 768, generator=gen)
    w_hh = torch.randn(2, 384, 128, generator=gen) / np.sqrt(128)
    b_hh = torch.randn(2, 384, generator=gen) * 0.1
    xr, wr, br = xproj.clone().requires_grad_(), w_hh.clone().requires_grad_(), b_hh.clone().requires_grad_()
    finals = []
    for d in range(2):
        gi = xr[:, :, d * 384:(d + 1) * 384]
        h = torch.zeros(B, 128)
        for t in (range(L - 1, -1, -1) if d == 1 else range(L)):
            gh = h @ wr[d].t() + br[d]
            r = torch.sigmoid(gi[t, :, :128] + gh[:, :128])
            z = torch.sigmoid(gi[t, :, 128:256] + gh[:, 128:256])
            n = torch.tanh(gi[t, :, 256:] + r * gh[:, 256:])
            h = (1 - z) * n + z * h
        finals.append(h)
    ref = torch.cat(finals, dim=1)
    up = torch.randn(B, 256, generator=gen)
    (ref * up).sum().backward()

    def body(g):
        wd = g.put(w_hh)
        hfinal, hs, gates = ops.gru_fwd(g.put(xproj), wd, g.put(b_hh), B, L, precision)
        dgi, dgh, hprev, dbias = ops.gru_bwd(g.put(up), wd, hs, gates, B, L, precision)
        bias = ops.gru_bias_grads(dbias)
        return dict(hfinal=hfinal, dgi=dgi, dgh=dgh, hprev=hprev, dbias=dbias, **{f"bias{i}": t for i, t in enumerate(bias)})

    got = twice(body)
    np.testing.assert_allclose(got["hfinal"].numpy(), ref.detach().numpy(), atol=tol)
    db = got["dbias"].sum(0)
    np.testing.assert_allclose(db[:, 3].numpy(), br.grad[:, 256:].numpy(), atol=tol * 50)
    np.testing.assert_allclose(db[:, :2].reshape(2, 256).numpy(), br.grad[:, :256].numpy(), atol=tol * 50)
    np.testing.assert_allclose(db[:, :3].reshape(2, 384).numpy(), xr.grad.sum((0, 1)).view(2, 384).numpy(), atol=tol * 50)
    np.testing.assert_allclose(got["dgi"].view(L, B, 768).numpy(), xr.grad.numpy(), atol=tol * 5)
    for d in range(2):
        dw = got["dgh"][d].double().t() @ got["hprev"][d].double()
        np.testing.assert_allclose(dw.numpy(), wr.grad[d].double().numpy(), atol=tol * 50)
        np.testing.assert_allclose(got["dgh"][d].double().sum(0).numpy(), br.grad[d].double().numpy(), atol=tol * 50)
        # (db_ih, db_hh) of direction d: the input-side gradient of the three gates, and the hidden side's (r, z, hn)
        np.testing.assert_allclose(got[f"bias{2 * d}"].numpy(), xr.grad.sum((0, 1)).view(2, 384)[d].numpy(), atol=tol * 50)
        np.testing.assert_allclose(got[f"bias{2 * d + 1}"].numpy(), br.grad[d].numpy(), atol=tol * 50)


def test_embedding_rows_and_elementwise_kernels():
    """test_embedding_kernels_match_torch (exact), test_layout_kernels_and_row_ops (l2norm 1e-7 / 1e-4, colsum 1e-5); act_bwd, relu_bwd, axpy,
    the casts and copy_segments are exact by construction (one rounding, or none)."""
    gen = torch.Generator().manual_seed(23)
    B, L, V, D = 7, 13, 50, 256
    tok = torch.randint(0, V, (B, L), generator=gen, dtype=torch.int32)
    w = torch.randn(V, D, generator=gen)
    w[0] = 0
    wr = w.clone().requires_grad_()
    eref = F.embedding(tok.t().contiguous().long(), wr, padding_idx=0)
    dout = ints((L, B, D), -3, 3, 29)
    eref.backward(dout)
    x = torch.randn(9, 512, generator=gen)
    x[4] = 0
    xr = x.clone().requires_grad_()
    nref = F.normalize(xr, dim=1)
    dz = torch.randn(9, 512, generator=gen)
    nref.backward(dz)
    m = torch.randn(37, 96, generator=gen)
    a_out, a_dout = torch.tanh(torch.randn(19, 512, generator=gen)), torch.randn(19, 512, generator=gen)
    big = torch.randn(10008, generator=gen)                        # (the casts take multiples of 4 elements)
    segs = [torch.randn(n, generator=gen) for n in (1, 4099, 384)]

    def body(g):
        out = dict(emb=ops.embedding_fwd(g.put(tok), g.put(w)), demb=ops.embedding_bwd(g.put(tok), g.put(dout), V))
        z, norm = ops.l2norm_fwd(g.put(x))
        out.update(z=z, norm=norm, dx=ops.l2norm_bwd(z, norm, g.put(dz)), colsum=ops.colsum(g.put(m)))
        for act in (1, 2):
            out[f"act_bwd{act}"] = ops.act_bwd(g.put(a_dout), g.put(a_out), act, inplace=False)
        for store in (F32, F16, BF16):
            out[f"relu_bwd_{IDS[store]}"] = ops.relu_bwd(g.put(a_dout.to(store)), g.put(a_out.to(store)), inplace=False)
        for store in (F16, BF16):
            h = ops.cast_from_f32(g.put(big), store, scale=0.5)
            out[f"cast_{IDS[store]}"], out[f"back_{IDS[store]}"] = h, ops.cast_to_f32(h)
        acc = g.put(big.clone())
        ops.check(ops.lib().tri_axpy(ops.ptr(g.put(big.flip(0))), 0.25, ops.ptr(acc), big.numel(), ops.stream()), "tri_axpy")       # y += a * x
        out["axpy"] = acc
        dst = [g.put(torch.zeros_like(s)) for s in segs]
        ops.copy_segments([(g.put(s), d) for s, d in zip(segs, dst)])
        out.update({f"seg{i}": d for i, d in enumerate(dst)})
        return out

    got = twice(body)
    assert torch.equal(got["emb"], eref.detach()) and torch.equal(got["demb"], wr.grad)
    np.testing.assert_allclose(got["z"].numpy(), nref.detach().numpy(), atol=1e-7)
    keep = [0, 1, 2, 3, 5, 6, 7, 8]
    np.testing.assert_allclose(got["dx"][keep].numpy(), xr.grad[keep].numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(got["colsum"].numpy(), m.sum(0).numpy(), atol=1e-5)
    assert torch.equal(got["act_bwd1"], a_dout * (a_out > 0))
    np.testing.assert_allclose(got["act_bwd2"].numpy(), (a_dout.double() * (1 - a_out.double() ** 2)).numpy(), rtol=4e-7, atol=1e-7)   # (three fp32 roundings)
    for store in (F32, F16, BF16):
        assert torch.equal(got[f"relu_bwd_{IDS[store]}"], torch.where(a_out.to(store) > 0, a_dout.to(store), torch.zeros((), dtype=store)))
    for store in (F16, BF16):
        assert torch.equal(got[f"cast_{IDS[store]}"], (big * 0.5).to(store)) and torch.equal(got[f"back_{IDS[store]}"], (big * 0.5).to(store).float())
    np.testing.assert_allclose(got["axpy"].numpy(), (big.double() + 0.25 * big.flip(0).double()).numpy(), rtol=2e-7, atol=1e-7)
    for i, s in enumerate(segs):
        assert torch.equal(got[f"seg{i}"], s)


@pytest.mark.parametrize("B", [5, 65])
def test_ntxent_pair(B):
    """test_ntxent_large_batch_against_float64: oracle.modules.nt_xent_numpy, 2e-5 on the loss, 1e-6 on the gradients."""
    from oracle.modules import nt_xent_numpy
    gen = torch.Generator().manual_seed(8)
    za, zb = torch.randn(B, 512, generator=gen), torch.randn(B, 512, generator=gen)
    zb[:B // 2] += za[:B // 2] * 2

    def body(g):
        loss, dza, dzb = ops.ntxent_fwd_bwd(g.put(za), g.put(zb), 0.1, 0.25)
        return dict(loss=loss, dza=dza, dzb=dzb)

    got = twice(body)
    l64, da, db = nt_xent_numpy(za.numpy(), zb.numpy(), 0.1, 0.25)
    assert abs(got["loss"].item() - l64) < 2e-5
    np.testing.assert_allclose(got["dza"].numpy(), da, atol=1e-6)
    np.testing.assert_allclose(got["dzb"].numpy(), db, atol=1e-6)


def test_ntxent_all_pairs():
    """test_ntxent_all_pairs_equals_the_pair_by_pair_loop at M = 3, B = 5, against the float64 pair loss (2e-5 / 1e-6 as above) with
    upstream gradients 1 per pair."""
    from oracle.modules import nt_xent_numpy
    gen = torch.Generator().manual_seed(11)
    zs = [torch.randn(5, 512, generator=gen) for _ in range(3)]

    def body(g):
        zd = [g.put(z) for z in zs]
        losses, ws = ops.ntxent_multi_fwd(zd, 0.1, 0.25)
        dzs = ops.ntxent_multi_bwd(zd, ws, 0.1, 0.25, dtotal=g.put(torch.ones(())))
        return dict(losses=losses, **{f"dz{i}": d for i, d in enumerate(dzs)})

    got = twice(body)
    want = [np.zeros((5, 512)) for _ in range(3)]
    total = 0.0
    for p, (i, j) in enumerate(combinations(range(3), 2)):
        l64, da, db = nt_xent_numpy(zs[i].numpy(), zs[j].numpy(), 0.1, 0.25)
        assert abs(got["losses"][p].item() - l64) < 2e-5
        total += l64
        want[i] += da
        want[j] += db
    assert abs(got["losses"][3].item() - total) < 3 * 2e-5
    for i in range(3):
        np.testing.assert_allclose(got[f"dz{i}"].numpy(), want[i], atol=2e-6)


def test_triplet_pair_and_all_pairs(golden):
    """tests/test_gpu_triplet.py: test_every_fixture_case_against_the_reference_float64 (fixture case dense_b48, 4 x the reference's own fp32
    noise) and test_all_pairs_is_bit_equal_to_the_pair_by_pair_loop (M = 3)."""
    from tests import triplet_reference as tr
    from tests.test_triplet_golden import case_inputs, check_against_fixture
    gd = golden("triplet")
    tag = "dense_b48"
    a, b = case_inputs(gd, tag)
    c, _ = tr.make_inputs("clustered", 48, 512, 2, 0.2, int(gd[f"{tag}/seed"]) + 100)
    c = 0.7 * a + 0.3 * c
    margin, up = float(gd[f"{tag}/margin"]), 0.75
    host = [a, b, c]

    def body(g):
        zs = [g.put(z) for z in host]
        upd = g.put(torch.tensor(up))
        loss, counts, ws = ops.triplet_fwd(zs[0], zs[1], margin)
        dza, dzb = ops.triplet_bwd(zs[0], zs[1], ws, margin, upd)
        out = dict(loss=loss, counts=counts, dza=dza, dzb=dzb)
        losses, mcounts, mws = ops.triplet_multi_fwd(zs, margin)
        dzs = ops.triplet_multi_bwd(zs, mws, margin, dtotal=upd)
        out.update(losses=losses, mcounts=mcounts, **{f"dz{i}": d for i, d in enumerate(dzs)})
        for p, (i, j) in enumerate(combinations(range(3), 2)):
            l, cn, w2 = ops.triplet_fwd(zs[i], zs[j], margin)
            di, dj = ops.triplet_bwd(zs[i], zs[j], w2, margin, upd)
            out.update({f"pl{p}": l, f"pc{p}": cn, f"pdi{p}": di, f"pdj{p}": dj})
        return out

    got = twice(body)
    assert got["counts"].tolist() == [int(gd[f"{tag}/n_semi"]), int(gd[f"{tag}/n_hard"])]
    check_against_fixture(gd, tag, got["loss"].item(), got["dza"].numpy(), got["dzb"].numpy(), 4.0 * float(gd["max_err_loss32"]),
                          4.0 * float(gd["max_err_grad32"]), scale=up, report="guarded kernel")
    sums = [torch.zeros(48, 512) for _ in range(3)]
    for p, (i, j) in enumerate(combinations(range(3), 2)):
        assert same_bytes(got["losses"][p], got[f"pl{p}"]) and got["mcounts"][p].tolist() == got[f"pc{p}"].tolist()
        sums[i] = sums[i] + got[f"pdi{p}"]
        sums[j] = sums[j] + got[f"pdj{p}"]
    for i in range(3):
        assert same_bytes(got[f"dz{i}"], sums[i])                  # (each embedding takes part in two pairs: one fp32 addition, commutative)


def test_adam_kernels():
    """test_adam_matches_torch_optim at n = 10007 (oracle.modules.adam_step_explicit, 2e-7); the segment reader (include/tricolo_hip.h:
    segment sizes multiples of 4) over three segments with one absent - a null gradient pointer: skipped like a parameter whose .grad is
    None -, its guard over the two present ones; the flat guard on a view that starts 4 bytes past a 16-byte boundary (scalar head and tail)."""
    from oracle.modules import adam_step_explicit
    gen = torch.Generator().manual_seed(2)
    n = 10007
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) for _ in range(3)]
    ns = 10008
    starts = [0, 4100, 4100 + 1536]                                   # segment 1 is absent
    ps0, gs = torch.randn(ns, generator=gen), torch.randn(ns, generator=gen)
    hp = (3.5e-4, 0.9, 0.999, 1e-8, 1e-6)
    bad = torch.randn(1031, generator=gen)
    bad_tail, bad_head = bad.clone(), bad.clone()
    bad_tail[-1], bad_head[0] = float("inf"), float("nan")

    def body(g):
        out = {}
        pd, m, v = g.put(p0), g.put(torch.zeros(n)), g.put(torch.zeros(n))
        step = g.put(torch.zeros(4, dtype=torch.int32))
        for gr in grads:
            ops.adam_tick(step)
            ops.adam_step(pd, g.put(gr), m, v, step, *hp)
        out.update(p=pd, m=m, v=v, step=step)
        ps, ms, vs = g.put(ps0), g.put(torch.zeros(ns)), g.put(torch.zeros(ns))
        step2 = g.put(torch.zeros(4, dtype=torch.int32))
        g0, g2 = g.put(gs[:starts[1]]), g.put(gs[starts[2]:])
        ptrs = g.put(torch.tensor([g0.data_ptr(), 0, g2.data_ptr()], dtype=torch.int64))
        st = g.put(torch.tensor(starts, dtype=torch.int64))
        scan_ptrs = g.put(torch.tensor([g0.data_ptr(), g2.data_ptr()], dtype=torch.int64))
        scan_st = g.put(torch.tensor([0, g0.numel()], dtype=torch.int64))
        ops.adam_guard_segments(scan_ptrs, scan_st, g0.numel() + g2.numel(), step2)
        ops.adam_tick(step2)
        ops.adam_step_segments(ps, ptrs, st, ms, vs, step2, *hp)
        out.update(ps=ps, ms=ms, vs=vs, step2=step2)
        # the segment guard must see the LAST element of a segment (and nothing past it: the band behind g0 is NaN in the 0xFF run)
        g0_inf = gs[:starts[1]].clone()
        g0_inf[-1] = float("inf")
        g0i = g.put(g0_inf)
        step3 = g.put(torch.zeros(4, dtype=torch.int32))
        ops.adam_guard_segments(g.put(torch.tensor([g0i.data_ptr(), g2.data_ptr()], dtype=torch.int64)), scan_st, g0.numel() + g2.numel(), step3)
        out["step3"] = step3
        for name, t in (("clean", bad), ("tail", bad_tail), ("head", bad_head)):
            buf = g.put(torch.cat([torch.zeros(1), t]))
            s3 = g.put(torch.zeros(4, dtype=torch.int32))
            view = buf[1:]
            assert view.data_ptr() % 16 == 4
            ops.adam_guard(view, s3)
            out[f"guard_{name}"] = s3
        return out

    got = twice(body)
    pr, mr, vr = p0.clone(), torch.zeros(n), torch.zeros(n)
    for s_, gr in enumerate(grads, 1):
        adam_step_explicit(pr, gr, mr, vr, s_)
    # the moments' reference gets the hyper-parameters the kernel gets: the C ABI takes them as fp32, and 1 - fp32(0.999) is 1.3e-5 (relative)
    # below 1 - 0.999 - every v would sit that far from a reference fed with the doubles
    hp32 = [float(np.float32(h)) for h in hp]
    pq, mr, vr = p0.clone(), torch.zeros(n), torch.zeros(n)
    for s_, gr in enumerate(grads, 1):
        adam_step_explicit(pq, gr, mr, vr, s_, *hp32)
    np.testing.assert_allclose(got["p"].numpy(), pr.numpy(), atol=2e-7)
    assert got["step"].tolist() == [3, 0, 0, 0]
    # moments: g' = g + wd p, m = b1 m + (1 - b1) g', v = b2 v + (1 - b2) g'^2 in fp32 on both sides, FMA contraction or not: <= 5 roundings
    # per step over 3 steps of the absolute terms - m's sum to <= 3 * 0.1 * max|g| ~ 1.5 (16 * 2^-24 * 1.5 = 1.5e-6), v's are all positive
    # (relative: 1e-6)
    np.testing.assert_allclose(got["m"].numpy(), mr.numpy(), rtol=0, atol=1.5e-6)
    np.testing.assert_allclose(got["v"].numpy(), vr.numpy(), rtol=1e-6, atol=1e-12)
    p1, m1, v1 = ps0.clone(), torch.zeros(ns), torch.zeros(ns)
    adam_step_explicit(p1, gs, m1, v1, 1, *hp32)
    present = torch.ones(ns, dtype=torch.bool)
    present[starts[1]:starts[2]] = False
    np.testing.assert_allclose(got["ps"][present].numpy(), p1[present].numpy(), atol=2e-7)
    assert torch.equal(got["ps"][~present], ps0[~present]) and not bool(got["ms"][~present].any()) and not bool(got["vs"][~present].any())
    np.testing.assert_allclose(got["ms"][present].numpy(), m1[present].numpy(), rtol=0, atol=1.5e-6)
    np.testing.assert_allclose(got["vs"][present].numpy(), v1[present].numpy(), rtol=1e-6, atol=1e-12)
    assert got["step2"].tolist() == [1, 0, 0, 0]                        # (the clean gradient left the guard's flag alone: the step applied)
    assert got["step3"][2].item() != 0 and got["step3"][0].item() == 0
    assert got["guard_clean"][2].item() == 0 and got["guard_tail"][2].item() != 0 and got["guard_head"][2].item() != 0


@pytest.mark.parametrize("n", [1, 2047, 5 * 2048 + 3])
def test_mask_count_and_compact(n):
    """test_mask_compact_matches_nonzero."""
    m = (torch.rand(n, generator=torch.Generator().manual_seed(n % 1000)) < 0.4).to(torch.uint8)
    m[n - 1] = 1
    mpad = torch.zeros((n + 31) // 32 * 32, dtype=torch.uint8)
    mpad[:n] = m

    def body(g):
        md = g.put(mpad)
        rows, count = ops.mask_compact(md, n)
        return dict(rows=rows[:int(m.sum())], count=count, count2=ops.mask_count(md, n))

    got = twice(body)
    ref = torch.nonzero(m).flatten().int()
    assert int(got["count"]) == ref.numel() == int(got["count2"]) and torch.equal(got["rows"], ref)


def test_mask_pyramid_and_multi_compaction():
    """test_mask_pyramid_and_multi_list_compaction at (3, 16)."""
    B, V = 3, 16
    m = (torch.rand(B, 1, V, V, V, generator=torch.Generator().manual_seed(B * 100 + V)) < 0.02).float()
    m[0, 0, V - 1, V - 1, V - 1] = 1
    n0 = B * V ** 3
    m0 = torch.zeros((n0 + 31) // 32 * 32, dtype=torch.uint8)
    m0[:n0] = m.reshape(-1).to(torch.uint8)
    ns = [B * (V >> l) ** 3 for l in range(5)]
    refs = [m]
    for l in range(1, 5):
        refs.append(F.max_pool3d(refs[-1], 2))
    refrows = [torch.nonzero(r.reshape(-1)).flatten().int() for r in refs]

    def body(g):
        md = g.put(m0)
        outs = ops.mask_pyramid(md, B, V)
        lists = ops.mask_compact_multi([md] + outs, ns)
        out = {f"mask{l}": o for l, o in enumerate(outs, 1)}
        out.update({f"rows{l}": r[:refrows[l].numel()] for l, (r, c) in enumerate(lists)})
        out.update({f"count{l}": c for l, (r, c) in enumerate(lists)})
        return out

    got = twice(body)
    for l in range(5):
        if l:
            assert torch.equal(got[f"mask{l}"][:ns[l]], refs[l].reshape(-1).to(torch.uint8)) and not bool(got[f"mask{l}"][ns[l]:].any()), f"level {l}"
        assert int(got[f"count{l}"]) == refrows[l].numel() and torch.equal(got[f"rows{l}"], refrows[l]), f"level {l}"


def test_staging_kernels():
    """test_layout_kernels_and_row_ops (voxel_scatter, nchw3_to_nhwc4: exact) and test_u8_input_staging_is_bit_identical_to_the_host_prepared_inputs
    (tests/test_gpu_modules.py: voxel_from_rgba == voxel_scatter of the same grids, nchw3_u8_to_nhwc4 == nchw3_to_nhwc4 of the host-normalised
    images), in the three storage types."""
    from tricolo_amd.data import synthetic as syn
    from tricolo_amd.data.synthetic import make_images_u8, normalise_images
    batch = syn.make_batch(3, voxel_size=32, num_views=None, seed=syn.BASE_SEED + 41, keep_grids=True)
    locs, feats, grids = batch["voxels"]["locs"], batch["voxels"]["feats"], batch["voxel_grids_u8"]
    rng = np.random.default_rng(5)
    u8 = torch.from_numpy(np.stack([make_images_u8(rng, 2, 64) for _ in range(2)])).view(4, 3, 64, 64)
    f32 = normalise_images(u8.numpy())

    def body(g):
        out = {}
        for store in STORES:
            t = IDS[store]
            out[f"dense_{t}"], out[f"mask_{t}"] = ops.voxel_scatter(g.put(locs.to(torch.int32)), g.put(feats), 3, 32, dtype=store)
            out[f"rgba_{t}"], out[f"rgba_mask_{t}"] = ops.voxel_from_rgba(g.put(grids), dtype=store)
            out[f"f32_{t}"], out[f"u8_{t}"] = ops.nchw3_to_nhwc4(g.put(f32), dtype=store), ops.nchw3_u8_to_nhwc4(g.put(u8), dtype=store)
        return out

    got = twice(body)
    ref = torch.zeros(3, 32, 32, 32, 4)
    ref[locs[:, 0].long(), locs[:, 1].long(), locs[:, 2].long(), locs[:, 3].long(), :3] = feats
    for store in STORES:
        t = IDS[store]
        assert torch.equal(got[f"dense_{t}"], ref.to(store)) and int(got[f"mask_{t}"].sum()) == locs.shape[0]
        assert torch.equal(got[f"rgba_{t}"], got[f"dense_{t}"]) and torch.equal(got[f"rgba_mask_{t}"], got[f"mask_{t}"])
        assert torch.equal(got[f"f32_{t}"][:, 0, :, :, :3], f32.permute(0, 2, 3, 1).to(store)) and float(got[f"f32_{t}"][..., 3].float().abs().sum()) == 0.0
        assert torch.equal(got[f"u8_{t}"], got[f"f32_{t}"])


def test_retrieval_topk():
    """test_retrieval_metrics_on_device_match_reference (tests/test_gpu_modules.py) at Nq = 3, Ns = 37, k = 5: numpy's float64 ranking -
    descending, equal similarities higher index first -, the 0-based rank of the query's own label, similarities to 1e-13."""
    rng = np.random.default_rng(3)
    shp = rng.standard_normal((37, 64)).astype(np.float32)
    shp[20] = shp[7]                                                 # an exact tie
    txt = shp[[7, 36, 0]] + 0.01 * rng.standard_normal((3, 64)).astype(np.float32)
    lab = np.array([7, 36, 5], dtype=np.int32)

    def body(g):
        idx, sim, hit = ops.retrieval_topk(g.put(torch.from_numpy(txt)), g.put(torch.from_numpy(shp)), g.put(torch.from_numpy(lab)), k=5)
        return dict(idx=idx, sim=sim, hit=hit)

    got = twice(body)
    sims = txt.astype(np.float64) @ shp.astype(np.float64).T
    order = np.flip(np.argsort(sims, axis=1, kind="stable"), 1)
    np.testing.assert_array_equal(got["idx"].numpy(), order[:, :5])
    np.testing.assert_array_equal(got["hit"].numpy(), np.argmax(order == lab[:, None], axis=1))
    np.testing.assert_allclose(got["sim"].numpy(), np.take_along_axis(sims, order[:, :5], 1), rtol=1e-13, atol=1e-13)


def test_batched_weight_packing():
    """test_batched_weight_packing_equals_per_layer_packing: tri_weight_prep_multi equals tri_weight_prep layer by layer, every packed
    operand and the descriptor table inside bands."""
    cases = [_BY["vox_l1"], _BY["stem7x7"], _BY["c3x3s2"], _BY["clip768"], _vox("vox_odd", 1, 4, 40, 72)]
    made = [make_case(c, integer=False, seed=7) for c in cases]

    def body(g):
        out = {}
        for precision in ("bf16", "bf16x3", "f16"):
            packer = ops.WeightPacker()
            for c, (_, _, wp, _, geom) in zip(cases, made):
                wd = g.put(wp)
                for tr in (False, True):
                    if tr and (geom.cin != geom.cin_stored or geom.cin % 4):
                        continue
                    packer.add((c[0], tr), wd, geom, transposed=tr)
                    hi, lo = ops.pack_weight(wd, geom, precision, transposed=tr)
                    out[f"{precision}/{c[0]}/{tr}/hi"], out[f"{precision}/{c[0]}/{tr}/lo"] = hi, lo
            for key, (hi, lo) in packer.run(precision, torch.device(DEV)).items():
                out[f"{precision}/{key[0]}/{key[1]}/hi_multi"], out[f"{precision}/{key[0]}/{key[1]}/lo_multi"] = hi, lo
        return out

    got = twice(body)
    for k, v in got.items():
        if k.endswith("_multi"):
            assert torch.equal(v, got[k[:-6]]), k


# ================================================================================================ completeness
# entry points a training step launches that no guarded case above needs to launch
EXEMPT = {
    "tri_debug_stamp": "diagnostics: only launched while a timeline is being recorded (tools/step_timeline.py); writes its own 8-byte stamp, no tensor of the step",
}


# what the groups above set out to launch: a routing branch that silently stopped being reached shows here, not as a quietly thinner file
REQUIRED = {
    "tri_weight_prep", "tri_weight_prep_multi", "tri_conv_fwd", "tri_conv_dgrad", "tri_conv_dgrad_bn", "tri_conv_plan_build", "tri_conv_wgrad",
    "tri_conv_wgrad_partial", "tri_conv_wgrad_partial_group", "tri_wgrad_reduce_grouped", "tri_wgrad_reduce_grouped_noted", "tri_conv_stem_wgrad_bn",
    "tri_bn_finalize", "tri_bn_act", "tri_bn_bwd_reduce", "tri_bn_bwd_finalize", "tri_bn_bwd_apply", "tri_bn_bwd_small", "tri_bn_bwd_pair_reduce",
    "tri_bn_bwd_pair_finalize", "tri_bn_bwd_pair_apply", "tri_bn_bwd_rows", "tri_bn_bwd_apply_rows", "tri_bn_relu_pool3d_fwd", "tri_pool3d_bwd_route",
    "tri_pool3d_bwd_route_rows", "tri_pool3d_bwd_route_rows_reduce", "tri_pool3d_bwd_route_reduce", "tri_maxpool2d_fwd", "tri_maxpool2d_bwd",
    "tri_maxpool_bn_bwd_reduce", "tri_maxpool_bn_bwd_reduce_pooled", "tri_maxpool_bn_bwd_apply", "tri_avgpool_viewmax_fwd", "tri_avgpool_viewmax_bwd",
    "tri_linear_small_fwd", "tri_linear_small_bwd", "tri_linear_small_wgrad", "tri_gru_fwd", "tri_gru_bwd", "tri_gru_bias_grads", "tri_embedding_fwd",
    "tri_embedding_bwd", "tri_l2norm_fwd", "tri_l2norm_bwd", "tri_colsum", "tri_act_bwd", "tri_relu_bwd", "tri_axpy", "tri_cast_from_f32",
    "tri_cast_to_f32", "tri_copy_segments", "tri_ntxent_fwd_bwd", "tri_ntxent_multi_fwd", "tri_ntxent_multi_bwd", "tri_triplet_fwd", "tri_triplet_bwd",
    "tri_triplet_multi_fwd", "tri_triplet_multi_bwd", "tri_adam_tick", "tri_adam_step", "tri_adam_step_segments", "tri_adam_guard",
    "tri_adam_guard_segments", "tri_mask_count", "tri_mask_compact", "tri_mask_pyramid", "tri_mask_compact_multi", "tri_voxel_scatter",
    "tri_voxel_from_rgba_u8", "tri_nchw3_to_nhwc4", "tri_nchw3_u8_to_nhwc4", "tri_retrieval_topk",
}


def _run_guarded_cases(golden):
    """Every guarded test of this file with every parameter set of its parametrize marks (their side effect is LAUNCHED)."""
    import inspect
    import itertools
    me = test_every_entry_point_of_a_training_step_has_a_guarded_case
    tests = [f for n, f in sorted(globals().items()) if n.startswith("test_") and inspect.isfunction(f) and f is not me]
    for fn in tests:
        marks = [m for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"]
        names = [[a.strip() for a in m.args[0].split(",")] for m in marks]
        for combo in itertools.product(*[m.args[1] for m in marks]):
            kw = {}
            for ns, val in zip(names, combo):
                kw.update(zip(ns, val if len(ns) > 1 else (val,)))
            if "golden" in inspect.signature(fn).parameters:
                kw["golden"] = golden
            fn(**kw)


def test_every_entry_point_of_a_training_step_has_a_guarded_case(golden):
    """One eager training step of TriCoLoNet per case of STEP_CASES (tests/test_gpu_modules.py) in f16 and bf16x3 under the recording
    wrapper: every tri_* entry point those steps LAUNCH was launched by a guarded case of this file in this process (when the test is
    selected alone it runs those cases itself), or is named in EXEMPT.  Size and plan queries take no stream and no device memory and
    are not launches (guard_bands.stream_entry_points)."""
    from tests.test_gpu_modules import STEP_CASES, _build_net
    from tricolo_amd.data import synthetic as syn
    if not REQUIRED <= LAUNCHED:                              # selected alone (-k, another worker): run the guarded cases here
        _run_guarded_cases(golden)
    assert REQUIRED <= LAUNCHED, f"no guarded case launched {sorted(REQUIRED - LAUNCHED)}"
    before = ops.default_precision()
    stepped = set()
    try:
        for precision in ("f16", "bf16x3"):
            ops.set_default_precision(precision)
            for tag, text, image, voxel, V, nv, S, B, seed_off, clip_text in STEP_CASES:
                net, cfg = _build_net(text, image, voxel, V, nv or 6, S)
                batch = syn.batch_to_device(syn.make_batch(B, voxel_size=V if voxel else None, num_views=nv if image else None, image_size=S,
                                                           clip_text=clip_text, seed=syn.BASE_SEED + seed_off), DEV)
                opt = net.configure_optimizers()
                with recording() as rec:
                    opt.zero_grad(set_to_none=True)
                    loss = net.training_step(batch, 0)
                    loss.backward()
                    opt.step()
                    torch.cuda.synchronize()
                assert np.isfinite(loss.item())
                stepped.update(rec.launches())
                del net, opt, batch
    finally:
        ops.set_default_precision(before)
    assert len(stepped) > 30, stepped
    missing = sorted(stepped - LAUNCHED - set(EXEMPT))
    assert not missing, f"launched by a training step, by no guarded case: {missing}"
    assert set(EXEMPT) <= stream_entry_points() and not set(EXEMPT) & LAUNCHED, "EXEMPT names an unknown entry point, or one a guarded case launches"
