"""Float64 reference of the BatchNorm / pooling passes (tricolo_amd/csrc/bn_pool.hip) and the tolerances the kernels are held to.

Plain torch; everything runs in float64 on whatever device its inputs are on, from the STORED values of the tensors (a 16-bit tensor
is converted to float64, never re-derived).  Importable without a GPU: tests/test_bn_reference_cpu.py proves on an fp32 emulation of the
three-pass scheme that the bounds are neither wrong (the faithful emulation passes) nor vacuous (eight mutations of it fail).

Where the numbers come from (none is tuned on the kernels):

u32 = 2^-24 (fp32 unit roundoff), eps_s = machine epsilon of the storage type, r_c^2 = mean_c^2 / (var_c + 1e-5).

* Statistics.  Each conv-epilogue record is one fp32 rounding of a sum of size n * (var + mean^2); the records are summed in double and
  var = q / n - mean^2 exposes that rounding by 1 + r^2:  invstd and scale within 4 u32 (1 + r^2) relative, mean within
  4 u32 (|mean| + std).  shift = beta - mean * scale is formed in double from the same mean and invstd and stored once in fp32: its bound
  is the two above pushed through the product plus u32 |shift| for that store (without the store term a channel with mean 0 and
  beta = 1.5 would be asked for an fp32 number more exact than fp32 holds).  Running statistics: momentum times the same bounds, plus
  u32 |value| for the fp32 store of every update (the kept 0.9 share is rounded too).
* Sums.  dgamma / dbeta per channel within 1e-4 * (sum of the ABSOLUTE terms) * out_scale: a forward-error bound of any fp32 summation
  with chains below ~1,600 terms, and one that a wrong small channel cannot hide behind a right big one.  Elements whose ReLU mask is
  undecidable (see below) add their own absolute terms: a flipped mask element moves a sum by exactly that much.
* Elementwise outputs.  eps_s |ref| (half an ulp of the store, half for an fp32 value on the other side of a rounding tie) + the smallest
  subnormal of the store + 8 u32 * (sum of the absolute terms of the expression) + the first-order effect of the statistics and sums
  bounds through the closed form.  The closed forms are perturbed as the passes compute them: y * scale + shift = scale (y - mean) + beta
  (scale and shift come from ONE invstd and mean in double) and dy = c1 (g - sum_g / n) + c3 (y - mean) (c2 is formed in double from c3
  and mean); the separate fp32 stores of shift / c2 are inside the 8 u32 term, which counts |shift| and |c2| among its terms.
* Masks and argmax maps are exact.  A ReLU mask element recomputed from y may differ from the float64 one only where the float64
  pre-activation is closer to zero than the arithmetic part of the elementwise bound (no store terms: nothing is stored; strictly closer,
  so an exactly-zero pre-activation of a channel whose bound is zero is never excused).  A winning tap / child / view may differ only
  where the float64 value of the kernel's choice is within the elementwise bound of the float64 maximum.  Both exemptions are counted and
  capped: MASK_CAP_TENSOR of a tensor's elements, MASK_CAP_CHANNEL of one channel's.
"""
import math
from types import SimpleNamespace

import torch

U32 = 2.0 ** -24
MOMENTUM, EPS = 0.1, 1e-5
SUM_TOL = 1e-4
MASK_CAP_TENSOR, MASK_CAP_CHANNEL = 1e-4, 1e-2


def eps_of(dtype):
    return float(torch.finfo(dtype).eps)


def tiny_of(dtype):
    return {torch.float32: 2.0 ** -149, torch.float16: 2.0 ** -24, torch.bfloat16: 2.0 ** -133}[dtype]


def f64(t):
    return t.detach().to(torch.float64)


def _active(t, rows):
    """[M, C] view of t, restricted to the rows with a non-zero mask byte (rows may be padded past M)."""
    t2 = t.reshape(-1, t.shape[-1])
    if rows is None:
        return t2
    return t2[rows.reshape(-1)[:t2.shape[0]].bool()]


# ------------------------------------------------------------------------------------------------ statistics
def bn_stats(y, gamma, beta, rows=None, running_mean=None, running_var=None, momentum=MOMENTUM, eps=EPS, updates=1):
    """Train-mode BatchNorm statistics of the stored y over the active rows, with the bound of every field (b_*).
    running_mean / running_var: the values BEFORE the call; the fields hold them after `updates` identical updates."""
    y64 = f64(_active(y, rows))
    n, C = y64.shape
    ga, be = f64(gamma), f64(beta)
    s = SimpleNamespace(n=n, C=C)
    if n == 0:                                        # no active site: BatchNorm is skipped, coefficients zero, running statistics kept
        z = torch.zeros(C, dtype=torch.float64, device=y.device)
        s.mean = s.var = s.invstd = s.scale = s.shift = s.r2 = s.rel = s.b_mean = s.b_invstd = s.b_scale = s.b_shift = s.b_shift_own = z
        s.running_mean, s.running_var = (None if running_mean is None else f64(running_mean)), (None if running_var is None else f64(running_var))
        s.b_running_mean = s.b_running_var = z
        return s
    s.mean = y64.mean(0)
    s.var = ((y64 - s.mean) ** 2).mean(0)
    s.invstd = 1.0 / torch.sqrt(s.var + eps)
    s.scale = ga * s.invstd
    s.shift = be - s.mean * s.scale
    s.r2 = s.mean ** 2 / (s.var + eps)
    s.rel = 4 * U32 * (1 + s.r2)
    s.b_mean = 4 * U32 * (s.mean.abs() + torch.sqrt(s.var))
    s.b_invstd = s.rel * s.invstd
    s.b_scale = s.rel * s.scale.abs()
    s.b_shift = s.scale.abs() * s.b_mean + s.mean.abs() * s.b_scale + U32 * s.shift.abs()
    s.b_shift_own = torch.zeros_like(s.mean)         # error of shift that is NOT shared with scale and mean (eval mode only)
    s.running_mean = s.running_var = None
    if running_mean is not None:
        unb = s.var * n / (n - 1) if n > 1 else s.var
        b_unb = 2 * s.rel * (s.var + eps) * (n / (n - 1) if n > 1 else 1.0)
        rm, rv = f64(running_mean), f64(running_var)
        brm, brv = torch.zeros_like(rm), torch.zeros_like(rv)
        for _ in range(updates):
            rm = (1 - momentum) * rm + momentum * s.mean
            rv = (1 - momentum) * rv + momentum * unb
            brm = (1 - momentum) * brm + momentum * s.b_mean + U32 * rm.abs()
            brv = (1 - momentum) * brv + momentum * b_unb + U32 * rv.abs()
        s.running_mean, s.running_var, s.b_running_mean, s.b_running_var = rm, rv, brm, brv
    return s


def eval_stats(gamma, beta, running_mean, running_var, eps=EPS):
    """Eval-mode coefficients.  The pass works in fp32 throughout (rv + eps, sqrt, divide, two products, one subtraction): four
    roundings on invstd and scale, and a shift whose error is its own, not shared with scale."""
    s = SimpleNamespace(n=1, C=gamma.numel())
    ga, be, rm, rv = f64(gamma), f64(beta), f64(running_mean), f64(running_var)
    s.mean, s.var = rm, rv
    s.invstd = 1.0 / torch.sqrt(rv + eps)
    s.scale = ga * s.invstd
    s.shift = be - rm * s.scale
    s.rel = torch.full_like(rm, 4 * U32)
    s.b_mean = torch.zeros_like(rm)
    s.b_invstd, s.b_scale = s.rel * s.invstd, s.rel * s.scale.abs()
    s.b_shift_own = 4 * U32 * (rm * s.scale).abs() + U32 * s.shift.abs()
    s.b_shift = s.b_shift_own + rm.abs() * s.b_scale
    return s


# ------------------------------------------------------------------------------------------------ forward apply
def _affine(y64, st):
    """(value, arithmetic bound) of y * scale + shift per element: 8 u32 of the absolute terms + the statistics' first-order effect."""
    v = y64 * st.scale + st.shift
    mag = (y64 * st.scale).abs() + st.shift.abs()
    b = 8 * U32 * mag + (y64 - st.mean).abs() * st.b_scale + st.scale.abs() * st.b_mean + st.b_shift_own
    return v, b


def bn_act(y, st, relu=True, res=None, res_st=None, store=None):
    """relu(y * scale + shift + res), res = identity or res * rscale + rshift.  -> (ref, bound, pre, band): pre = the float64
    pre-activation, band = its arithmetic bound (the ReLU-mask exemption band)."""
    store = store or y.dtype
    pre, band = _affine(f64(y), st)
    if res is not None:
        if res_st is not None:
            r, rb = _affine(f64(res), res_st)
        else:
            r = f64(res)
            rb = 8 * U32 * r.abs()
        pre, band = pre + r, band + rb
    ref = torch.relu(pre) if relu else pre
    bound = eps_of(store) * ref.abs() + tiny_of(store) + band
    return ref, bound, pre, band


# ------------------------------------------------------------------------------------------------ backward
def bn_bwd(y, g, st, gamma, mode="final", relu_out=None, rows=None, out_scale=1.0, store=None, undecided=None, g_unmasked=None):
    """BatchNorm backward in closed form over the active rows.  mode: "final" (g is the gradient of the BatchNorm output), "relu" (of
    relu(bn(y)): mask recomputed from y), "relu_out" (of relu(bn(y) + residual) with its saved output relu_out; g_masked returned).
    -> namespace on the ACTIVE rows: dy, b_dy, g_masked, dgamma, dbeta, b_dgamma, b_dbeta, undecided (mask exemption, bool [n, C]).
    Inactive rows are the caller's to check: exactly zero, or untouched with keep_inactive."""
    store = store or y.dtype
    y64, g64 = f64(_active(y, rows)), f64(_active(g, rows))
    n, C = y64.shape
    ga = f64(gamma)
    o = SimpleNamespace(n=n)
    zero = torch.zeros(C, dtype=torch.float64, device=y.device)
    if n == 0:
        o.dy = o.b_dy = o.g_masked = y64
        o.undecided = torch.zeros_like(y64, dtype=torch.bool)
        o.dgamma = o.dbeta = o.b_dgamma = o.b_dbeta = zero
        return o
    o.undecided = torch.zeros_like(y64, dtype=torch.bool)
    if mode == "relu":
        pre, band = _affine(y64, st)
        g64 = g64 * (pre > 0)
        o.undecided = pre.abs() < band
    elif mode == "relu_out":
        g64 = g64 * (f64(_active(relu_out, rows)) > 0)      # the saved output is an input of the pass: its mask is exact
    else:
        assert mode == "final"
    if undecided is not None:                               # the caller masked g itself and says where its mask is undecidable
        o.undecided = _active(undecided, rows)
    o.g_masked = g64
    und = o.undecided.to(torch.float64) * f64(_active(g if g_unmasked is None else g_unmasked, rows)).abs()
    sg, sgy = g64.sum(0), (g64 * (y64 - st.mean)).sum(0)
    mass_b = g64.abs().sum(0)
    mass_g = st.invstd * ((g64 * y64).abs().sum(0) + st.mean.abs() * mass_b)
    o.dbeta, o.dgamma = sg * out_scale, st.invstd * sgy * out_scale
    bb = SUM_TOL * mass_b + und.sum(0)                                                        # bounds of the unscaled sums
    bg = SUM_TOL * mass_g + st.invstd * (und * (y64 - st.mean).abs()).sum(0)
    o.b_dbeta, o.b_dgamma = bb * abs(out_scale), bg * abs(out_scale)
    # dy = c1 (g - sum_g / n) + c3 (y - mean),  c1 = gamma invstd,  c3 = -gamma invstd^2 dgamma / n,  c2 = -c1 sum_g / n - c3 mean
    dga = st.invstd * sgy
    c1, c3 = ga * st.invstd, -ga * st.invstd ** 2 * dga / n
    c2 = -c1 * sg / n - c3 * st.mean
    o.dy = c1 * g64 + c2 + c3 * y64
    mag = (c1 * g64).abs() + c2.abs() + (c3 * y64).abs()
    b_c1 = st.rel * c1.abs()
    b_dga = bg + st.rel * dga.abs() + st.invstd * sg.abs() * st.b_mean
    b_c3 = 2 * st.rel * c3.abs() + ga.abs() * st.invstd ** 2 * b_dga / n
    first = b_c1 * (g64 - sg / n).abs() + c1.abs() * bb / n + b_c3 * (y64 - st.mean).abs() + c3.abs() * st.b_mean
    o.b_dy = eps_of(store) * o.dy.abs() + tiny_of(store) + 8 * U32 * mag + first
    return o


# ------------------------------------------------------------------------------------------------ pooling
def _first_max(z, dim):
    """Index of the first maximum along dim (torch.max / argmax give no order guarantee among ties)."""
    m = z.max(dim, keepdim=True).values
    n = z.shape[dim]
    shape = [1] * z.dim()
    shape[dim] = n
    idx = torch.arange(n, device=z.device).reshape(shape).expand_as(z)
    return torch.where(z == m, idx, n).min(dim).values, m.squeeze(dim)


def round_store(x64, store):
    """x as it reads back after a store in `store` (through fp32, as the passes convert)."""
    return x64.to(torch.float32).to(store).to(torch.float64)


def _windows3d(t, B, D):
    """[B, D, D, D, K] -> [B, Do, Do, Do, 8, K], the children of a 2x2x2 window in d, h, w scan order."""
    Do, K = D // 2, t.shape[-1]
    return t.reshape(B, Do, 2, Do, 2, Do, 2, K).permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(B, Do, Do, Do, 8, K)


def _unwindows3d(t, B, D):
    Do, K = D // 2, t.shape[-1]
    return t.reshape(B, Do, Do, Do, 2, 2, 2, K).permute(0, 1, 4, 2, 5, 3, 6, 7).reshape(B, D, D, D, K)


def pool3d(y, st, mask, B, D, store=None, pooled=None, dpooled=None):
    """BatchNorm + ReLU + site mask + 2x2x2 max-pool of one voxel level, y [B,D,D,D,C] (inactive rows may hold anything, NaN included):
    pooled = max over the ACTIVE children of relu(bn(y)), 0 for an empty window; mask_out = any child active.
    Backward (pooled = the forward's STORED output, an input of the pass, and dpooled): g, the gradient of the BatchNorm output, is dpooled
    at the first active child in scan order whose value, rounded to the storage type, equals the stored maximum and is positive; zero at
    every other active child.  A child is a candidate when the stored maximum lies between its float64 value minus / plus its arithmetic
    bound, both rounded to the storage type; it is certain when the two roundings agree.  The pass takes the first child that hits, so the
    routing of a window is decided when it has one candidate, or no uncertain candidate stands before the first certain one, or all
    candidates are equal in any arithmetic (the first wins); otherwise its candidates up to the first certain one are returned in
    `undecided` (the counted exemption) with |dpooled| in g_abs.
    -> namespace pooled, b_pooled [B,Do,Do,Do,C], mask_out [Mo] and, for the backward, g, g_abs [B,D,D,D,C] float64, undecided (bool)."""
    store = store or y.dtype
    C = y.shape[-1]
    M, Do = B * D ** 3, D // 2
    dev = y.device
    zero, ninf = torch.zeros((), dtype=torch.float64, device=dev), torch.full((), -math.inf, dtype=torch.float64, device=dev)
    act = mask.reshape(-1)[:M].bool()
    y64 = torch.where(act[:, None], f64(y.reshape(M, C)), zero)
    pre, band = _affine(y64, st)
    aw = _windows3d(act.reshape(B, D, D, D, 1), B, D)
    zw = torch.where(aw, _windows3d(torch.relu(pre).reshape(B, D, D, D, C), B, D), ninf)
    bw = torch.where(aw, _windows3d(band.reshape(B, D, D, D, C), B, D), zero)
    o = SimpleNamespace()
    o.mask_out = aw.any(4).reshape(-1)
    o.pooled = torch.clamp(zw.max(4).values, min=0.0)
    o.b_pooled = eps_of(store) * o.pooled + tiny_of(store) + bw.max(4).values         # (the fp32 maximum may be another child's value)
    if dpooled is None:
        return o
    P = f64(pooled).reshape(B, Do, Do, Do, 1, C)
    lo, hi = round_store(torch.clamp(zw - bw, min=0.0), store), round_store(torch.clamp(zw + bw, min=0.0), store)
    cand = aw & (lo <= P) & (P <= hi) & (P > 0)
    idx = torch.arange(8, device=dev).reshape(1, 1, 1, 1, 8, 1)
    first = torch.where(cand, idx, 8).min(4, keepdim=True).values
    sure = cand & (lo == hi)
    first_sure = torch.where(sure, idx, 8).min(4, keepdim=True).values
    yw = _windows3d(y64.reshape(B, D, D, D, C), B, D)
    y_first = torch.gather(yw, 4, first.clamp(max=7))
    # equal in any arithmetic: the same y, or a scale of exactly zero (gamma = 0: fma(y, 0, shift) = shift for every y)
    same = (~cand | (yw == y_first)).all(4, keepdim=True) | (st.scale == 0)
    und = (cand & ~sure & (idx < first_sure)).any(4, keepdim=True) & (cand.sum(4, keepdim=True) > 1) & ~same
    flagged = cand & und & (idx <= first_sure)
    dp = torch.where(o.mask_out.reshape(B, Do, Do, Do, 1, 1), f64(dpooled).reshape(B, Do, Do, Do, 1, C), zero)
    o.g = _unwindows3d(torch.where(idx == first, dp, zero), B, D)
    o.g_abs = _unwindows3d(torch.where(flagged, dp.abs(), zero), B, D)
    o.undecided = _unwindows3d(flagged, B, D)
    return o


def stem_pool(y, st, store=None, dpool=None, tap=None):
    """relu(bn(y)) -> 3x3 / stride 2 / pad 1 max-pool of y [N,1,H,W,C]: pooled values, tap map (kh * 3 + kw of the first maximum in scan
    order over the in-bounds taps, compared unrounded) and, with dpool, g = the gradient of the BatchNorm output [N,1,H,W,C]."""
    store = store or y.dtype
    N, _, H, W, C = y.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    pre, band = _affine(f64(y).reshape(N, H, W, C), st)
    z = torch.relu(pre)
    pad = torch.full((N, H + 2, W + 2, C), -math.inf, dtype=torch.float64, device=y.device)
    pad[:, 1:H + 1, 1:W + 1] = z
    bp = torch.zeros_like(pad)
    bp[:, 1:H + 1, 1:W + 1] = band
    taps = torch.stack([pad[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2] for kh in range(3) for kw in range(3)], 3)     # [N,Ho,Wo,9,C]
    btaps = torch.stack([bp[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2] for kh in range(3) for kw in range(3)], 3)
    o = SimpleNamespace(z=taps, b_z=btaps)
    o.tap, o.pooled = _first_max(taps, 3)
    o.b_pooled = eps_of(store) * o.pooled.abs() + tiny_of(store) + btaps.max(3).values
    if dpool is not None:                                  # tap: the map to route by (the backward pass takes the forward's map as an input)
        d64 = f64(dpool).reshape(N, Ho, Wo, C)
        tp = o.tap if tap is None else tap.reshape(N, Ho, Wo, C).long()
        gp = torch.zeros((N, H + 2, W + 2, C), dtype=torch.float64, device=y.device)
        for kh in range(3):
            for kw in range(3):
                gp[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2] += d64 * (tp == kh * 3 + kw)
        o.g_unmasked = gp[:, 1:H + 1, 1:W + 1].reshape(N, 1, H, W, C)
        o.g = o.g_unmasked * (pre > 0).reshape(N, 1, H, W, C)
        o.undecided = ((pre.abs() < band).reshape(N, 1, H, W, C)) & (o.g_unmasked != 0)
    return o


def avgpool_viewmax(x, B, V, dout=None, scale=1.0):
    """Mean over the HW positions of x [B*V, 1, H, W, C], then the maximum over the V views of one shape, first maximal view wins.
    -> (out [B, C], arg [B, C], bound, means [B, V, C]) and, with dout, dx = scale * dout / HW at the winning view, zero elsewhere."""
    N, _, H, W, C = x.shape
    x64 = f64(x).reshape(B, V, H * W, C)
    means = x64.mean(2)
    arg, out = _first_max(means, 1)
    # a plain fp32 loop over HW terms is within (HW - 1) u32 sum|x|; the product with the rounded 1 / HW adds 2 u32 |mean| and the fp32
    # store one more; the kernel's winner may be another view inside that bound, so the largest view's mean |x| is taken: (HW + 4) u32
    bound = (H * W + 4) * U32 * x64.abs().mean(2).max(1).values
    dx = None
    if dout is not None:
        win = (torch.arange(V, device=x.device).reshape(1, V, 1) == arg.unsqueeze(1)).to(torch.float64)
        dx = (win * (f64(dout) * (scale / (H * W))).unsqueeze(1)).unsqueeze(2).expand(B, V, H * W, C).reshape(x.shape)
    return out, arg, bound, means, dx


# ------------------------------------------------------------------------------------------------ checks
class Report:
    """Largest fraction of each bound that was used, and the largest counted exemption, with the case that produced it."""

    def __init__(self):
        self.used = {}

    def note(self, kind, value, case):
        if kind not in self.used or value > self.used[kind][0]:
            self.used[kind] = (value, case)

    def lines(self):
        return [f"{k}: {v:.3g}  ({c})" for k, (v, c) in sorted(self.used.items())]


def fraction(out, ref, bound):
    """max |out - ref| / bound; an exact match uses nothing of a zero bound, any miss of a zero bound is infinite; NaN / inf fail."""
    err = (f64(out) - ref).abs()
    fr = torch.where(err == 0, torch.zeros_like(err), err / bound)
    fr = torch.where(torch.isnan(fr), torch.full_like(fr, math.inf), fr)
    return fr


def check(report, kind, case, name, out, ref, bound, exempt=None):
    """Assert |out - ref| <= bound elementwise (shapes [.., C]); elements under `exempt` are counted instead, against the two caps."""
    C = ref.shape[-1]
    fr = fraction(out.reshape(ref.shape), ref, bound).reshape(-1, C)
    bad = fr > 1.0
    if exempt is not None:
        ex = bad & exempt.reshape(-1, C)
        bad = bad & ~exempt.reshape(-1, C)
        n_ex = ex.sum(0).double()
        if ex.numel() == 0:
            return 0.0
        report.note("mask exemption, share of a tensor", float(n_ex.sum()) / ex.numel(), f"{case} {name}")
        report.note("mask exemption, share of a channel", float(n_ex.max()) / ex.shape[0], f"{case} {name}")
        assert float(n_ex.sum()) <= MASK_CAP_TENSOR * ex.numel(), (case, name, "exempted elements", float(n_ex.sum()), ex.numel())
        assert float(n_ex.max()) <= MASK_CAP_CHANNEL * ex.shape[0], (case, name, "exempted elements of one channel", float(n_ex.max()), ex.shape[0])
        fr = torch.where(ex, torch.zeros_like(fr), fr)
    worst = float(fr.max()) if fr.numel() else 0.0
    if bool(bad.any()):
        r, c = [int(v) for v in torch.nonzero(bad)[0]]
        o2, r2, b2 = out.reshape(-1, C), ref.reshape(-1, C), bound.reshape(-1, C) if bound.dim() > 1 else bound.reshape(1, C).expand(fr.shape)
        raise AssertionError(f"{case} {name}: {int(bad.sum())} of {bad.numel()} elements outside the bound, worst {worst:.3g} x bound; first at row {r} "
                             f"channel {c}: got {float(o2[r, c])!r}, float64 {float(r2[r, c])!r}, bound {float(b2[r, c]):.3g}; "
                             f"channels hit: {torch.nonzero(bad.any(0)).reshape(-1).tolist()[:16]}")
    report.note(kind, worst, f"{case} {name}")
    return worst


def check_stats(report, case, co, st, running=None):
    """co: the four fp32 coefficient vectors of the pass (mean, invstd, scale, shift); running = (running_mean, running_var) after it."""
    for name, out, ref, b in (("mean", co.mean, st.mean, st.b_mean), ("invstd", co.invstd, st.invstd, st.b_invstd),
                              ("scale", co.scale, st.scale, st.b_scale), ("shift", co.shift, st.shift, st.b_shift)):
        check(report, "statistics", case, name, out.reshape(1, -1), ref.reshape(1, -1), b.reshape(1, -1))
    if running is not None:
        check(report, "statistics", case, "running_mean", running[0].reshape(1, -1), st.running_mean.reshape(1, -1), st.b_running_mean.reshape(1, -1))
        check(report, "statistics", case, "running_var", running[1].reshape(1, -1), st.running_var.reshape(1, -1), st.b_running_var.reshape(1, -1))


def check_bwd(report, case, ref, dy, dgamma, dbeta, rows=None, g_masked=None, inactive=None):
    """dy / dgamma / dbeta (and g_masked) of a backward pass against bn_bwd's namespace.  inactive: None, or the exact value every
    element of an inactive dy row must hold (0.0 = zeroed, a sentinel = untouched)."""
    if ref.undecided.numel():                             # the input itself: at most half of each cap inside the band, from the reference alone
        share, worst = band_share(ref.undecided)
        assert share <= 0.5 * MASK_CAP_TENSOR and worst <= 0.5 * MASK_CAP_CHANNEL, (case, "share of the input inside the exemption band", share, worst)
    check(report, "sums", case, "dgamma", dgamma.reshape(1, -1), ref.dgamma.reshape(1, -1), ref.b_dgamma.reshape(1, -1))
    check(report, "sums", case, "dbeta", dbeta.reshape(1, -1), ref.dbeta.reshape(1, -1), ref.b_dbeta.reshape(1, -1))
    check(report, "elementwise", case, "dy", _active(dy, rows), ref.dy, ref.b_dy, exempt=ref.undecided)
    if g_masked is not None:
        assert torch.equal(f64(_active(g_masked, rows)), ref.g_masked), (case, "g_masked")
    if rows is not None and inactive is not None:
        dead = dy.reshape(-1, dy.shape[-1])[~rows.reshape(-1)[:dy.numel() // dy.shape[-1]].bool()]
        assert bool((dead == inactive).all()), (case, "inactive rows of dy", inactive)


def band_share(undecided):
    """(share of the tensor, largest share of one channel) of the elements inside the mask exemption band - from the reference alone."""
    u = undecided.reshape(-1, undecided.shape[-1]).double()
    return float(u.mean()), float(u.mean(0).max())


# ------------------------------------------------------------------------------------------------ inputs
STRESS = ("r3", "r30", "const", "zero", "masked", "gamma0", "gamma_neg", "gamma_tiny")


def make_inputs(M, C, store, seed, device="cpu", r100=False, grad_scale=1.0, row_p=None, live=None):
    """Gaussian y with a per-channel mean and spread and the stress channels (index = position in STRESS): |mean| / std = 3 and 30, a
    constant channel, an all-zero channel with beta = 0 (pre-activation exactly zero in any arithmetic), a channel whose pre-activation is
    negative everywhere (its gradient is masked away), gamma = 0, gamma < 0, gamma = 1e-3 with beta = 1.5; r100: channel 8 at
    |mean| / std = 100.  row_p: share of active rows; inactive rows of y and g hold NaN.
    -> namespace y, g, res (stored in `store`), gamma, beta (fp32), rows (uint8, padded to 32, or None)."""
    assert C >= 16
    gen = torch.Generator().manual_seed(seed)
    mean = torch.randn(C, generator=gen) * 0.5
    std = torch.rand(C, generator=gen) * 1.5 + 0.25
    gamma, beta = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.3
    mean[0], mean[1] = 3 * std[0], -30 * std[1]
    if r100:
        mean[8] = 100 * std[8]
    y = torch.randn(M, C, generator=gen) * std + mean
    y[:, 2], beta[2] = 0.75, 0.3
    y[:, 3], beta[3] = 0.0, 0.0
    beta[4] = -12.0
    gamma[5] = 0.0
    gamma[6] = -gamma[6]
    gamma[7], beta[7] = 1e-3, 1.5
    g = torch.randn(M, C, generator=gen) * grad_scale
    g[:, 2:4] /= grad_scale                          # (variance 0: dy = 316 gamma (g - mean g) would leave the f16 range at the f16 gradient scale)
    res = torch.randn(M, C, generator=gen)
    o = SimpleNamespace(M=M, C=C, store=store, rows=None, gamma=gamma.to(device), beta=beta.to(device))
    if row_p is not None or live is not None:              # live: the active rows themselves (bool [M]) instead of a share
        live = torch.rand(M, generator=gen) < row_p if live is None else live.reshape(-1).bool().cpu()
        rows = torch.zeros((M + 31) // 32 * 32, dtype=torch.uint8)
        rows[:M] = live.to(torch.uint8)
        y[~live], g[~live] = math.nan, math.nan
        o.rows = rows.to(device)
    o.y, o.g, o.res = y.to(device).to(store), g.to(device).to(store), res.to(device).to(store)
    return o
