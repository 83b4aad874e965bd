"""Tensor-level wrappers over the C ABI (one Python function per kernel family).

Precision modes: "bf16x3" fp32 activation storage, 3-product split bf16 operands (strict parity);
"f16" f16 activation storage and operands, fp32 accumulation, bf16x3 heads / GRU (inside the 1e-3 parity bound at the
speed of the bf16 mode); "bf16" bf16 storage and operands (throughput mode of BASELINE config 2).

All tensors are contiguous, channels-last ([B, D, H, W, C]; 2D tensors carry D = 1) and live on the GPU.
Nothing here falls back to torch arithmetic: every function launches a kernel of libtricolo_hip.so on the
current torch stream (so the calls can be captured into a HIP graph together with the rest of the step).
"""
from __future__ import annotations

import collections
import math
import os

import torch

from . import _C
from ._C import check, lib, make_desc, ptr, stream

_PRECISIONS = ("bf16", "bf16x3", "f16")
_FMT = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}        # act_fmt of include/tricolo_hip.h
# Gradients of the big activation tensors are stored in f16 in the f16 mode.  Their magnitude shrinks with the number of
# positions they spread over (1e-6 .. 1e-5 per element in layer1 at batch 32 x 6 views), below f16's normal range
# (6.1e-5): they are carried multiplied by 2^12 from the first 16-bit gradient tensor of a tower to the parameter-gradient
# kernels, which multiply by 2^-12 (exact).  f16 max is 65504.
F16_GRAD_SCALE = float(os.environ.get("TRICOLO_F16_GRAD_SCALE", "4096"))      # (a power of two: the un-scaling is exact)
if not (F16_GRAD_SCALE >= 1.0 and math.frexp(F16_GRAD_SCALE)[0] == 0.5):
    raise ValueError(f"TRICOLO_F16_GRAD_SCALE={F16_GRAD_SCALE!r}: must be a power of two >= 1 (the kernels divide it out exactly)")
_default_precision = os.environ.get("TRICOLO_PRECISION", "bf16x3")


def set_default_precision(p: str):
    global _default_precision
    if p not in _PRECISIONS:
        raise ValueError(f"precision must be one of {_PRECISIONS}")
    _default_precision = p


def default_precision() -> str:
    return _default_precision


class KernelTimer:
    """Optional per-launch timing with HIP events on the launch stream (bench.py's roofline leg).  Disabled by
    default; when enabled every conv launch is bracketed by two events and tallied per kernel symbol."""

    def __init__(self):
        self.records = []          # (symbol, algorithmic_flops, start_event, end_event)
        self.overhead_ms = 0.0     # fixed cost of one event pair around a launch (calibrate()), subtracted per record

    def calibrate(self, n=96):
        """Event-pair time of an (almost) empty kernel launched the same way: what a bracketed launch pays on top of its kernel's own
        duration (event processing + the dispatch gap; ~1.3 us of it is the stamp kernel itself and is left in).  Call behind a
        spin kernel so the launches are queued back to back like the step's."""
        buf = torch.zeros(1, dtype=torch.int64, device="cuda")
        pairs = []
        for _ in range(n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            check(lib().tri_debug_stamp(buf.data_ptr(), stream()), "tri_debug_stamp")
            b.record()
            pairs.append((a, b))
        torch.cuda.synchronize()
        ts = sorted(a.elapsed_time(b) for a, b in pairs)
        self.overhead_ms = max(ts[len(ts) // 2] - 1.3e-3, 0.0)
        return self.overhead_ms

    def run(self, symbol, flops, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        self.records.append((symbol, flops, a, b))
        return r

    def summary(self):
        """Per symbol: launches, summed event time (ms: the calibrated event-pair overhead subtracted per launch; ms_raw: as measured),
        flops = EXECUTED FLOPs (launches over a compact row list or a site mask count their active rows - resolved here from the
        device-side counts, after the synchronize), flops_dense = the dense-equivalent figure beside it."""
        torch.cuda.synchronize()
        agg = {}
        for sym, fl, a, b in self.records:
            d = agg.setdefault(sym, {"launches": 0, "ms": 0.0, "flops": 0, "flops_dense": 0})
            d["launches"] += 1
            e = a.elapsed_time(b)
            d["ms_raw"] = d.get("ms_raw", 0.0) + e
            d["ms"] += max(e - self.overhead_ms, 0.25 * e)
            ex, dense = fl() if callable(fl) else (fl, fl)
            d["flops"] += ex
            d["flops_dense"] += dense
        return agg


TIMER: KernelTimer | None = None


def _timed(symbol, flops, fn):
    return TIMER.run(symbol, flops, fn) if TIMER is not None else fn()


def _flops(g, rows=None, row_mask=None):
    """FLOPs of one launch of layer g for the KernelTimer: dense 2*M*taps*Cin*Cout, or - for launches that contract / compute over a
    compact row list or a site mask - a callable -> (executed, dense) with executed = 2 * active rows * taps * Cin * Cout, resolved at
    summary time from the device-side count (masked launches are priced on executed FLOPs)."""
    if TIMER is None or (rows is None and row_mask is None):
        return g.flops
    per_row = 2 * g.ntaps * g.cin * g.cout
    n = g.M
    if rows is not None:
        cnt = rows[1]
        return lambda: (per_row * min(int(cnt.item()), n), g.flops)
    return lambda: (per_row * int(row_mask[:n].sum().item()), g.flops)


def _flops_sum(items):
    """Sum of _flops() values (numbers or callables) as one value of the same kind."""
    if not any(callable(f) for f in items):
        return sum(items)

    def total():
        ex = dn = 0
        for f in items:
            e, d = f() if callable(f) else (f, f)
            ex, dn = ex + e, dn + d
        return ex, dn
    return total


_TNAME = {torch.float32: "float", torch.bfloat16: "bf16", torch.float16: "f16"}


# Kernel families of tri_conv_fwd / tri_conv_dgrad by code (TriConvFamily in include/tricolo_hip.h; the C side's table is conv_families[]
# in csrc/conv_igemm.hip): what rocprofv3 calls the kernel (variants of one family under one name), whether it reads the packed operand
# fragment-major (tri_weight_prep frag), and whether it walks the dense grid by the SITE MASK passed as row_mask.
ConvFamily = collections.namedtuple("ConvFamily", "symbol frag site_mask")
CONV_FAMILIES = {
    0: ConvFamily("conv_igemm_kernel<{tile}, {nsplit}, {t}>", False, False),
    2: ConvFamily("conv_dma_kernel<{tile}, {t}>", False, False),
    3: ConvFamily("conv_halo2d_kernel<{tile}, {t}>", False, False),
    4: ConvFamily("conv_stem_kernel<{kh}, {t}>", False, False),
    5: ConvFamily("conv_halo_rows_kernel<{t}>", False, False),
    6: ConvFamily("conv_vox0_kernel<{t}>", False, True),
    9: ConvFamily("conv_c64_kernel<{t}>", False, False),
    10: ConvFamily("conv_s2d_kernel<{t}>", False, False),
    12: ConvFamily("conv_pw_kernel<{tile}, {t}>", False, False),
    13: ConvFamily("conv_voxg_kernel<{tile}, {t}>", True, True),
    14: ConvFamily("conv_voxb_kernel<{t}>", True, True),
    15: ConvFamily("conv_s2g_kernel<{t}>", True, False),
}
# the word tri_conv_kernel_family returns (TRI_FAMILY_* in include/tricolo_hip.h)
FAMILY_CODE_MASK, FAMILY_TILE_SHIFT, FAMILY_SPLITK_SHIFT, FAMILY_SPU_SHIFT = 255, 8, 16, 24


# Kernel families of the weight gradient by code (TriWgradFamily; the C side's table is wgrad_families[] in csrc/conv_wgrad.hip): what
# rocprofv3 calls the kernel.  WGRAD_* are the feature bits and the word of tri_conv_wgrad_route (TRI_WGRAD_* in include/tricolo_hip.h).
WGRAD_FAMILIES = {
    0: "conv_wgrad_kernel<{bi}, {bj}, {nsplit}, {t}>",
    2: "conv_wgrad_dma_kernel<{bi}, {bj}, {t}>",
    4: "conv_stem_wgrad_kernel<{kh}, {t}>",
    6: "conv_vox0_wgrad_kernel<{t}>",
    7: "conv_wgrad_krow_kernel<{bi}, {t}>",
    9: "conv_wgrad_c64_kernel<{t}>",
}
WGRAD_MASK, WGRAD_ROWS, WGRAD_SPLIT3, WGRAD_BNF = 1, 2, 4, 8
WGRAD_ROUTE_GROUP_SHIFT, WGRAD_ROUTE_ROWS_SHIFT, WGRAD_ROUTE_COLS_SHIFT = 8, 12, 21


def _wgrad_symbol(g, route, dtype, split=False):
    """Name of the kernel a weight-gradient call with route word `route` (ConvGeom.wgrad_route) runs, for the KernelTimer."""
    return WGRAD_FAMILIES[route & FAMILY_CODE_MASK].format(bi=(route >> WGRAD_ROUTE_ROWS_SHIFT) & 511, bj=(route >> WGRAD_ROUTE_COLS_SHIFT) & 1023,
                                                           nsplit=2 if split else 1, t=_TNAME[dtype], kh=g.kernel[1])


def _igemm_symbol(g, transposed, split, t):
    """Name of the kernel the C dispatch picks for this layer (what rocprofv3 reports), for the KernelTimer."""
    code = g.kernel_family[(transposed, 1 if split else (2 if t.dtype != torch.float32 else 0))]
    return CONV_FAMILIES[code & FAMILY_CODE_MASK].symbol.format(tile=(code >> FAMILY_TILE_SHIFT) & 255, nsplit=2 if split else 1,
                                                                t=_TNAME[t.dtype], kh=g.kernel[1])


def _f32(t):
    assert t.dtype == torch.float32 and t.is_contiguous(), "expected contiguous fp32"
    return t


def _act(t):
    """Activation tensor: contiguous fp32 (bf16x3 mode), bf16 (bf16 mode) or f16 (f16 mode)."""
    assert t.dtype in _FMT and t.is_contiguous(), "expected contiguous fp32 / bf16 / f16 activations"
    return t


def _abf(t) -> int:
    """act_fmt of a tensor: 0 fp32, 1 bf16, 2 f16."""
    return _FMT[t.dtype]


def act_dtype(precision: str):
    """Storage type of the big activation tensors for a precision mode (TRICOLO_ACT_FP32=1 forces fp32 storage in bf16 mode)."""
    if precision == "f16":
        return torch.float16
    if precision == "bf16" and os.environ.get("TRICOLO_ACT_FP32", "0") != "1":
        return torch.bfloat16
    return torch.float32


def split3(precision: str) -> int:
    """3-product split bf16 operands in the fp32 kernels (heads, GRU): the strict mode and the f16 mode."""
    return 1 if precision in ("bf16x3", "f16") else 0


def head_precision(precision: str) -> str:
    """Precision of the dense fp32 layers (MLP heads, GRU input projection): the f16 mode runs them in bf16x3."""
    return "bf16x3" if precision == "f16" else precision


def grad_scale(precision: str) -> float:
    return F16_GRAD_SCALE if precision == "f16" else 1.0


def _conv_mode(x, lo) -> int:
    """Plan index of the conv entry points: 0 bf16 operands / fp32 storage, 1 bf16x3, 2 16-bit storage."""
    return 1 if lo is not None else (2 if x.dtype != torch.float32 else 0)


class ConvGeom:
    """Geometry + packed-weight buffers of one conv / linear layer.

    weight_strides = (s_co, s_tap, s_ci) element strides of the fp32 parameter in the reference's layout."""

    def __init__(self, B, in_grid, cin, cin_stored, cout, kernel, stride, pad, weight_strides):
        ID, IH, IW = in_grid
        KD, KH, KW = kernel
        pd, ph, pw = pad
        OD = (ID + 2 * pd - KD) // stride + 1
        OH = (IH + 2 * ph - KH) // stride + 1
        OW = (IW + 2 * pw - KW) // stride + 1
        self.B, self.in_grid, self.out_grid = B, (ID, IH, IW), (OD, OH, OW)
        self.cin, self.cin_stored, self.cout = cin, cin_stored, cout
        self.kernel, self.stride, self.pad = kernel, stride, pad
        self.ntaps = KD * KH * KW
        self.strides = weight_strides
        self.desc = make_desc(B, ID, IH, IW, cin_stored, OD, OH, OW, cout, KD, KH, KW, stride, pd, ph, pw)
        self.kpad = lib().tri_conv_kpad(self.ntaps, cin_stored)
        self.kpad_t = lib().tri_conv_kpad(self.ntaps, cout)
        self.M = B * OD * OH * OW
        self.M_in = B * ID * IH * IW
        self.num_mtiles = {m: lib().tri_conv_num_mtiles(_C.C.byref(self.desc), m) for m in (0, 1, 2)}     # by _conv_mode
        self.num_records_rows = {m: lib().tri_conv_num_records(_C.C.byref(self.desc), m, 1) for m in (0, 1, 2)}   # calls with a row list
        self.kernel_family = {(tr, m): lib().tri_conv_kernel_family(_C.C.byref(self.desc), 1 if tr else 0, m)
                              for tr in (False, True) for m in (0, 1, 2)}
        self.wgrad_ws = lib().tri_conv_wgrad_workspace(_C.C.byref(self.desc))
        routes = [lib().tri_conv_wgrad_route(_C.C.byref(self.desc), 1, feat) for feat in (0, WGRAD_MASK)]     # (negative: refused)
        self.wgrad_krow = routes[0] >= 0 and routes[0] & FAMILY_CODE_MASK == 7    # conv_wgrad_krow_kernel (resolution-keeping 3x3 layers, 16-bit storage, no row mask / list)
        self.wgrad_brick = routes[1] >= 0 and routes[1] & FAMILY_CODE_MASK == 6   # conv_vox0_wgrad_kernel: needs the dense site mask (row_mask), not a row list
        self._plans = {}
        self.fwd_ws = lib().tri_conv_workspace(_C.C.byref(self.desc), 0)
        self.dgrad_ws = lib().tri_conv_workspace(_C.C.byref(self.desc), 1) if cin == cin_stored and cin % 32 == 0 else 0

    def dgrad_row_order(self, device):
        """Stride-2 layers: the input positions sorted by the parity class of (coordinate + pad) per axis - the order in which
        tri_conv_dgrad should visit its rows so that a tile only runs the taps its rows can use.  None for stride 1."""
        if self.stride != 2 or self.ntaps == 1:                  # 1x1 / 2: one tap, nothing to skip (and scattered rows cost)
            return None
        t = self._plans.get(("rowpos", device))
        if t is None:
            ID, IH, IW = self.in_grid
            pd, ph, pw = self.pad
            pos = torch.arange(self.M_in, dtype=torch.int64)
            x, r = pos % IW, pos // IW
            y, r = r % IH, r // IH
            z = r % ID
            cls = (((z + pd) & 1) << 2) | (((y + ph) & 1) << 1) | ((x + pw) & 1)
            order = torch.sort(cls * self.M_in + pos).indices          # by class, ascending position inside a class
            t = order.to(torch.int32).to(device)
            self._plans[("rowpos", device)] = t
        return t

    def family(self, transposed: bool, mode: int) -> ConvFamily:
        """Row of CONV_FAMILIES for the kernel tri_conv_fwd / tri_conv_dgrad runs this layer on in plan `mode` (_conv_mode)."""
        return CONV_FAMILIES[self.kernel_family[(transposed, mode)] & FAMILY_CODE_MASK]

    def brick(self, transposed: bool, mode: int) -> bool:
        """True when tri_conv_fwd / tri_conv_dgrad runs this layer on a kernel that walks the dense grid by the SITE MASK (the brick kernels
        of conv_vox.hip, conv_voxg_kernel on the coarse grids): such launches take the mask as row_mask (rows of inactive sites are then
        neither computed nor written), not a compact row list."""
        return self.family(transposed, mode).site_mask

    def packed_frag(self, transposed: bool, precision: str, storage=None) -> int:
        """1 when the kernel that consumes this layer's packed operand (forward / data gradient) reads it in MFMA-fragment-major order
        (tri_weight_prep frag: conv_voxg_kernel loads its weight fragments straight into registers).  The plan mode follows the
        activation storage the operand will meet (default: the precision mode's own)."""
        storage = storage or act_dtype(precision)
        mode = 1 if precision == "bf16x3" else (2 if storage != torch.float32 else 0)
        return int(self.family(transposed, mode).frag)

    def check_packed(self, packed, transposed: bool, x):
        """The packed operand must be in the order this call's kernel reads (see pack_weight's `storage`)."""
        need = int(self.family(transposed, _conv_mode(x, packed[1])).frag)
        if getattr(packed[0], "tri_frag", 0) != need:
            raise RuntimeError("conv: the packed operand was ordered for another plan (row-major vs fragment-major): pack it with "
                               "pack_weight(..., storage=<dtype of the activations>)")

    def voxg_spu(self, transposed: bool, mode: int) -> int:
        """Samples per unit of conv_voxg_kernel for this layer (0: another kernel runs it)."""
        return (self.kernel_family[(transposed, mode)] >> FAMILY_SPU_SHIFT) & 127

    def splitk(self, transposed: bool, mode: int) -> bool:
        """True when tri_conv_fwd / tri_conv_dgrad runs this layer split-K in plan `mode` (_conv_mode): such launches take
        row_mask, not a compact row list."""
        return bool(self.kernel_family[(transposed, mode)] >> FAMILY_SPLITK_SHIFT & 1)

    def dgrad_bn_records(self, accumulate: bool, fmt: int) -> int:
        """Records tri_conv_dgrad_bn writes for this layer (0: its data-gradient kernel has no fused BatchNorm-backward sums), cached."""
        c = self.__dict__.setdefault("_dgrad_bn", {})
        k = (bool(accumulate), fmt)
        if k not in c:
            c[k] = int(lib().tri_conv_dgrad_bn_records(_C.C.byref(self.desc), 1 if accumulate else 0, fmt))
        return c[k]

    def wgrad_group(self, fmt: int):
        """(family, tiles, steps) of this layer's weight gradient for WgradBatch.add_job (tri_conv_wgrad_group_info), cached."""
        c = self.__dict__.setdefault("_wgrad_group", {})
        if fmt not in c:
            fam, tiles, steps = _C.C.c_int(), _C.C.c_int(), _C.C.c_int()
            check(lib().tri_conv_wgrad_group_info(_C.C.byref(self.desc), fmt, _C.C.byref(fam), _C.C.byref(tiles), _C.C.byref(steps)),
                  "tri_conv_wgrad_group_info")
            c[fmt] = (fam.value, tiles.value, steps.value)
        return c[fmt]

    def wgrad_route(self, fmt: int, features: int) -> int:
        """The word tri_conv_wgrad_route answers for a weight-gradient call with these WGRAD_* features in storage format fmt, cached;
        a call the library refuses raises as the call itself would."""
        c = self.__dict__.setdefault("_wgrad_route", {})
        if (fmt, features) not in c:
            word = lib().tri_conv_wgrad_route(_C.C.byref(self.desc), fmt, features)
            if word < 0:
                check(word, "tri_conv_wgrad_route")
            c[(fmt, features)] = word
        return c[(fmt, features)]

    def plan(self, device):
        """Gather plan (built once per geometry and device, reused by every step's wgrad)."""
        pl = self._plans.get(device)
        if pl is None:
            pl = torch.empty((lib().tri_conv_plan_bytes(_C.C.byref(self.desc)),), dtype=torch.uint8, device=device)
            check(lib().tri_conv_plan_build(_C.C.byref(self.desc), ptr(pl), stream()), "tri_conv_plan_build")
            self._plans[device] = pl
        return pl

    @property
    def flops(self):
        return 2 * self.M * self.ntaps * self.cin * self.cout


def pack_weight(w: torch.Tensor, g: ConvGeom, precision: str, transposed: bool = False, storage=None):
    """fp32 parameter -> (hi, lo|None) bf16 MFMA operand rows.  transposed=True packs the dgrad operand.  storage: dtype of the activation
    tensors the operand will meet (default act_dtype(precision)) - it selects the plan mode and with it the operand ORDER (row-major, or
    fragment-major for conv_voxg_kernel); conv_fwd / conv_dgrad refuse an operand packed for another plan."""
    s_co, s_tap, s_ci = g.strides
    if not transposed:
        rows, inner, inner_pad, kpad, s_row, s_inner = g.cout, g.cin, g.cin_stored, g.kpad, s_co, s_ci
    else:
        rows, inner, inner_pad, kpad, s_row, s_inner = g.cin_stored, g.cout, g.cout, g.kpad_t, s_ci, s_co
        if g.cin != g.cin_stored:
            raise RuntimeError("dgrad operand requested for a layer with padded input channels")
    hi = torch.empty((rows, kpad), dtype=torch.float16 if precision == "f16" else torch.bfloat16, device=w.device)
    lo = torch.empty_like(hi) if precision == "bf16x3" else None
    frag = g.packed_frag(transposed, precision, storage)
    check(lib().tri_weight_prep(ptr(_f32(w)), s_row, s_tap, s_inner, rows, g.ntaps, inner, inner_pad, ptr(hi), ptr(lo), _abf(hi),
                                frag, stream()), "tri_weight_prep")
    hi.tri_frag = frag
    return hi, lo


class WeightPacker:
    """Packs the MFMA operand rows of every layer of a tower in ONE launch per step (forward + data-gradient operands).

    Entries are registered once (parameter, geometry, direction); the packed buffers and the device-side descriptor
    table are persistent, so a step costs one kernel instead of one per layer.  The table is rebuilt if a parameter's
    storage moved (e.g. after FusedAdam re-bound the parameters to its flat buffer)."""

    def __init__(self):
        self.entries = {}            # key -> (param, geom, transposed)
        self._tables = {}            # precision -> (desc tensor, n, {key: (hi, lo)}, ptr snapshot)

    def add(self, key, param, g: "ConvGeom", transposed: bool = False):
        if key not in self.entries:
            self.entries[key] = (param, g, transposed)
            self._tables.clear()

    def _build(self, precision, device):
        descs = (_C.TriPrepDesc * len(self.entries))()
        bufs = {}
        for i, (key, (w, g, tr)) in enumerate(self.entries.items()):
            s_co, s_tap, s_ci = g.strides
            if not tr:
                rows, inner, inner_pad, kpad, s_row, s_inner = g.cout, g.cin, g.cin_stored, g.kpad, s_co, s_ci
            else:
                rows, inner, inner_pad, kpad, s_row, s_inner = g.cin_stored, g.cout, g.cout, g.kpad_t, s_ci, s_co
            hi = torch.empty((rows, kpad), dtype=torch.float16 if precision == "f16" else torch.bfloat16, device=device)
            lo = torch.empty_like(hi) if precision == "bf16x3" else None
            bufs[key] = (hi, lo)
            d = descs[i]
            d.fmt = _abf(hi)
            d.w, d.hi, d.lo = w.data_ptr(), hi.data_ptr(), (lo.data_ptr() if lo is not None else None)
            d.s_row, d.s_tap, d.s_inner = s_row, s_tap, s_inner
            d.rows, d.ntaps, d.inner, d.inner_pad, d.kpad = rows, g.ntaps, inner, inner_pad, kpad
            d.frag = hi.tri_frag = g.packed_frag(tr, precision)
        raw = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(device)
        snap = tuple(w.data_ptr() for (w, _, _) in self.entries.values())
        return raw, len(self.entries), bufs, snap

    def run(self, precision, device):
        """Launch the packing of all registered layers; returns {key: (hi, lo)}."""
        tab = self._tables.get(precision)
        if tab is None or tab[3] != tuple(w.data_ptr() for (w, _, _) in self.entries.values()):
            tab = self._build(precision, device)
            self._tables[precision] = tab
        raw, n, bufs, _ = tab
        check(lib().tri_weight_prep_multi(ptr(raw), n, stream()), "tri_weight_prep_multi")
        return bufs


def conv_fwd(x, g: ConvGeom, packed, row_mask=None, bias=None, act=0, want_stats=False, out=None, accumulate=False, rows=None):
    """rows = (row_pos, count) from mask_compact: only those rows are computed and WRITTEN (submanifold layers; pass no row_mask)."""
    hi, lo = packed
    g.check_packed(packed, False, x)
    OD, OH, OW = g.out_grid
    if out is None:
        out = torch.empty((g.B, OD, OH, OW, g.cout), dtype=x.dtype, device=x.device)
    assert out.dtype == x.dtype
    nrec = (g.num_records_rows if rows else g.num_mtiles)[_conv_mode(x, lo)]
    stats = torch.empty((nrec, 2, g.cout), dtype=torch.float32, device=x.device) if want_stats else None
    ws = _workspace(g.fwd_ws, x.device) if g.fwd_ws else None
    check(_timed(_igemm_symbol(g, False, lo is not None, x), _flops(g, rows, row_mask),
                 lambda: lib().tri_conv_fwd(_C.C.byref(g.desc), ptr(_act(x)), ptr(hi), ptr(lo), ptr(out), ptr(row_mask), ptr(bias),
                                            act, 1 if accumulate else 0, ptr(stats), _abf(x), ptr(ws),
                                            ws.numel() if ws is not None else 0, ptr(rows[0]) if rows else None,
                                            ptr(rows[1]) if rows else None, stream())), "tri_conv_fwd")
    return (out, stats) if want_stats else out


_ROW_ORDER = True                                                    # parity-class row order for stride-2 data gradients (A/B switch dropped in round 6)


# A/B switch: 0 = BatchNorm-backward sums as a pass of their own everywhere, 2 (default) = only the relu(bn1) form inside conv2's data
# gradient, 1 = also the relu(bn2 + x) form inside the accumulated conv1 gradient (reads y AND the saved output cold: 40.0 us against
# 38.3 us for data gradient + reduce pass, tools/dgrad_bn_bench.py; the relu(bn1) form 27.0 against 31.2)
_DGRAD_BN_MODE = os.environ.get("TRICOLO_DGRAD_BN", "2")
_DGRAD_BN = _DGRAD_BN_MODE != "0"


def conv_dgrad(dout, g: ConvGeom, packed_t, row_mask=None, out=None, accumulate=False, rows=None, bn_sums=None):
    """Data gradient.  bn_sums = (y, BNCoeffs | None, relu_out | None): the caller's next pass over the result is the BatchNorm-backward
    reduce of the BatchNorm that consumed y; where the layer's kernel can take those sums in its epilogue (tri_conv_dgrad_bn_records)
    the call returns (din, partial) and bn_bwd(..., partial=partial) skips its reduce launch, otherwise (din, None)."""
    hi, lo = packed_t
    g.check_packed(packed_t, True, dout)
    ID, IH, IW = g.in_grid
    if out is None:
        out = torch.empty((g.B, ID, IH, IW, g.cin_stored), dtype=dout.dtype, device=dout.device)
    assert out.dtype == dout.dtype
    ws = _workspace(g.dgrad_ws, dout.device) if g.dgrad_ws else None
    rowpos = g.dgrad_row_order(dout.device) if (row_mask is None and rows is None and _ROW_ORDER) else None
    if rows is not None:
        rowpos = rows[0]
    if bn_sums is not None:
        y, co, relu_out = bn_sums
        nrec = g.dgrad_bn_records(accumulate, _abf(dout)) if (_DGRAD_BN and not (accumulate and _DGRAD_BN_MODE == "2") and row_mask is None and rows is None and lo is None
                                                               and (relu_out is not None) == bool(accumulate)
                                                               and (co is not None) != (relu_out is not None)) else 0
        if nrec == 0:
            return conv_dgrad(dout, g, packed_t, row_mask=row_mask, out=out, accumulate=accumulate, rows=rows), None
        assert y.dtype == out.dtype and y.numel() == out.numel()
        partial = torch.empty((nrec, 2, g.cin_stored), dtype=torch.float32, device=dout.device)
        sums = _C.TriConvBnSums(ptr(y), ptr(co.scale) if co is not None else None, ptr(co.shift) if co is not None else None,
                                ptr(relu_out), ptr(partial))
        check(_timed(_igemm_symbol(g, True, False, dout), g.flops,
                     lambda: lib().tri_conv_dgrad_bn(_C.C.byref(g.desc), ptr(_act(dout)), ptr(hi), None, ptr(out), 1 if accumulate else 0,
                                                     _abf(dout), ptr(ws), ws.numel() if ws is not None else 0, ptr(rowpos),
                                                     _C.C.byref(sums), stream())), "tri_conv_dgrad_bn")
        return out, partial
    check(_timed(_igemm_symbol(g, True, lo is not None, dout), _flops(g, rows, row_mask),
                 lambda: lib().tri_conv_dgrad(_C.C.byref(g.desc), ptr(_act(dout)), ptr(hi), ptr(lo), ptr(out), ptr(row_mask),
                                              1 if accumulate else 0, _abf(dout), ptr(ws), ws.numel() if ws is not None else 0,
                                              ptr(rowpos), ptr(rows[1]) if rows else None, stream())), "tri_conv_dgrad")
    return out


_wgrad_ws = {}


def _workspace(nbytes: int, device) -> torch.Tensor:
    key = (device, torch.cuda.current_stream().cuda_stream)
    ws = _wgrad_ws.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _wgrad_ws[key] = ws
    return ws


_WGRAD_GROUPED = os.environ.get("TRICOLO_WGRAD_GROUPED", "1") != "0"     # A/B switch: one reduce launch per layer instead
_WGRAD_JOBS = os.environ.get("TRICOLO_WGRAD_JOBS", "1") != "0"           # A/B switch: one partial launch per layer instead
# output tiles (workgroups per split) this queue lets one grouped partial launch collect, per grouping family (1: 128-row, 2: 64-row,
# 3: 256-row DMA tiles; 4, 5, 7: conv_wgrad_krow_kernel<128> / <64> / <64> stride 2).  The queue's budget, not the resident-slot target the
# library plans a launch's splits for (wgrad_group_target: family 5 is 768 there); a krow launch may hold more workgroups than resident
# slots, the library deals them longest first
_WGRAD_JOB_TILES = {1: 512, 2: 448, 3: 256, 4: 512, 5: 512, 7: 512}


_WGRAD_REDUCE_OVERLAP = os.environ.get("TRICOLO_WGRAD_REDUCE_OVERLAP", "1") != "0"   # A/B switch (round 6): WgradBatch.flush(side=...)


# Overflow note (round 6): the optimizer whose zero_grad() ran last lends the grouped weight-gradient reduce its device record; the reduce flags
# a step that STORED an inf / NaN exactly as the optimizer's own scan would, and tags every gradient tensor it vouched for (`_tri_noted` =
# (address of the record, the tensor's version counter)) - FusedAdam leaves those out of its scan (64 of the default step's 74 MB of
# gradients).  The tag travels with the tensor OBJECT: a gradient that reaches the optimizer as another tensor (accumulated over several
# backward passes, cloned by AccumulateGrad, made contiguous) has no tag, one that was modified in place no longer matches its version -
# both are scanned as before.  (No table of addresses, and no reference to the tensors is kept here: a second owner makes autograd's
# AccumulateGrad CLONE every gradient it is handed - measured: +120 us per step.)
_GUARD_NOTE = None           # int32[4] device tensor (kept alive here) or None


def set_guard_note(note):
    global _GUARD_NOTE
    _GUARD_NOTE = note


def guard_noted(g, note) -> bool:
    """True when g's writer already noted its inf / NaN in `note` and nobody touched g since.  Consumes the tag: a second optimizer step on
    the same tensor scans it."""
    tag = g.__dict__.pop("_tri_noted", None)
    return tag is not None and tag == (note.data_ptr(), g._version)


class WgradBatch:
    """Deferred weight-gradient reduces of one tower backward (tri_conv_wgrad_partial / tri_wgrad_reduce_grouped).

    Every conv_wgrad(..., batch=b) launches only the position-split partial kernel, into a slab of its own carved from a
    per-stream arena that persists across steps (so a captured HIP graph replays on the same memory); b.flush() sums all of
    them in one launch.  The returned dw tensors hold garbage until then: flush before they leave the autograd Function.

    Layers of one kernel family (tri_conv_wgrad_group_info) are not even launched one by one: their jobs wait here until a launch's
    worth of output tiles (~448 workgroups) or TRI_WGRAD_JOBS_MAX of them are pending and then share ONE partial launch
    (tri_conv_wgrad_partial_group) - each layer is cut into fewer, longer splits, so the fp32 slabs the reduce has to re-read
    shrink by about the number of jobs.  The job keeps x / dout alive until that launch."""
    _arenas = {}

    def __init__(self, device, group_jobs: bool | None = None):
        self.device = device
        self.group_jobs = _WGRAD_JOBS if group_jobs is None else bool(group_jobs)
        # arenas of a HIP-graph capture are kept apart from the eager ones of the same stream id: a chunk allocated under capture lives
        # in the graph's private pool and must only ever be touched by replays (torch hands stream ids out of a small pool, so an
        # eager step could otherwise land on a capture's arena - ADVICE r2)
        self.chunks = WgradBatch._arenas.setdefault((device, torch.cuda.current_stream().cuda_stream, torch.cuda.is_current_stream_capturing()), [])
        self.ci, self.off, self.descs = 0, 0, []
        self.queues = {}                                          # kernel family -> [pending jobs, their output tiles]
        self._pre = None                                          # prelaunch() state: (descs to reduce early, event, family left for flush)
        self.dws = {}                                             # data_ptr -> gradient tensor of every layer queued here (overflow note)

    @property
    def jobs(self):
        return [j for q in self.queues.values() for j in q[0]]

    def add_job(self, family, tiles, job, keep, flops, sym):
        """Queue one layer's partial kernel in its family's queue (see the class docstring); that queue is launched first when this
        job does not fit beside what is pending."""
        q = self.queues.setdefault(family, [[], 0])
        if q[0] and (q[1] + tiles > _WGRAD_JOB_TILES[family] or len(q[0]) == _C.TRI_WGRAD_JOBS_MAX):
            self.launch_jobs(family)
            q = self.queues.setdefault(family, [[], 0])
        q[0].append((job, keep, flops, sym))
        q[1] += tiles

    def launch_jobs(self, family=None):
        for fam in ([family] if family is not None else sorted(self.queues)):
            pending = self.queues.pop(fam, [[], 0])[0]
            n = len(pending)
            if not n:
                continue
            arr = (_C.TriWgradJob * n)(*[j[0] for j in pending])
            pend = (_C.TriWgradReduce * n)()
            fmt = _abf(pending[0][1][0])
            check(_timed(pending[0][3], _flops_sum([j[2] for j in pending]),
                         lambda: lib().tri_conv_wgrad_partial_group(arr, n, fmt, pend, stream())), "tri_conv_wgrad_partial_group")
            for i in range(n):
                d = _C.TriWgradReduce()
                _C.C.memmove(_C.C.byref(d), _C.C.byref(pend[i]), _C.C.sizeof(d))
                self.descs.append(d)

    def slab(self, nbytes: int) -> torch.Tensor:
        nbytes = (nbytes + 255) // 256 * 256
        while True:
            if self.ci < len(self.chunks):
                if self.off + nbytes <= self.chunks[self.ci].numel():
                    t = self.chunks[self.ci][self.off:self.off + nbytes]
                    self.off += nbytes
                    return t
                self.ci, self.off = self.ci + 1, 0
            else:
                self.chunks.append(torch.empty(max(nbytes, 16 << 20), dtype=torch.uint8, device=self.device))

    @staticmethod
    def reserve(device, nbytes: int):
        """Make sure the current stream's arena holds at least nbytes (call eagerly, ahead of a capture)."""
        chunks = WgradBatch._arenas.setdefault((device, torch.cuda.current_stream().cuda_stream, torch.cuda.is_current_stream_capturing()), [])
        have = sum(c.numel() for c in chunks)
        if have < nbytes:
            chunks.append(torch.empty(max(nbytes - have, 16 << 20), dtype=torch.uint8, device=device))

    @staticmethod
    def release():
        """Drop every arena (between runs / modes: the chunks are plain torch allocations)."""
        WgradBatch._arenas.clear()

    def _reduce(self, descs):
        n = len(descs)
        if n:
            arr = (_C.TriWgradReduce * n)(*descs)
            note = _GUARD_NOTE
            if note is not None and self.device.index is not None and note.device.index != self.device.index:
                note = None
            check(lib().tri_wgrad_reduce_grouped_noted(arr, n, ptr(note), stream()), "tri_wgrad_reduce_grouped")
            if note is not None:
                for d in descs:
                    t = self.dws.pop(int(d.dw or 0), None)
                    if t is not None:
                        t._tri_noted = (note.data_ptr(), t._version)

    def prelaunch(self):
        """First half of flush(side=...): every pending family but the last is launched now (smallest first, the two largest swapped - see
        flush).  The caller may issue other work between this and flush(); -> True when something is left for flush() to overlap."""
        if self._pre is not None:
            return True
        fams = [f for f in sorted(self.queues) if self.queues[f][0]]
        if not _WGRAD_REDUCE_OVERLAP or len(fams) < 2:
            return False

        def work(f):                                              # dense layers carry their FLOPs as numbers (row-list layers: callables)
            fl = [j[2] for j in self.queues[f][0]]
            return sum(v for v in fl if not callable(v)) + 1e9 * self.queues[f][1] * any(callable(v) for v in fl)
        fams.sort(key=work)
        fams[-1], fams[-2] = fams[-2], fams[-1]
        for f in fams[:-1]:
            self.launch_jobs(f)
        early, self.descs = self.descs, []
        ev = torch.cuda.Event()
        ev.record()                                               # (the early reduce depends on the partial kernels issued so far ...)
        self._pre = (early, ev, fams[-1])
        return True

    def flush(self, side=None):
        """Launch what is pending and sum every slab into its parameter gradient.  side (a layers.SideStream forked from the CAPTURE'S ORIGIN
        stream - the image tower's; round 6): the pending families go smallest first with the two largest swapped, and the reduce of everything
        launched before the LAST partial kernel runs on the side stream beside that kernel (the image tower's tail: 80 % of the slab bytes
        belong to the 128-channel kernel-row launch, whose reduce - HBM-bound - then hides under the 64-channel launch - MFMA-bound)."""
        if side is None or not self.prelaunch():
            self.launch_jobs()
            self._reduce(self.descs)
            self.ci, self.off, self.descs = 0, 0, []
            self.dws.clear()
            return
        early, ev, last = self._pre
        self._pre = None
        late, self.descs = self.descs, []                         # (partial kernels issued between prelaunch() and here - the stem's)
        self.launch_jobs(last)                                    # (... and is issued behind the last one: released after it under graph replay)
        with torch.cuda.stream(side.fork(event=ev)):
            self._reduce(early)
        side.join()
        self._reduce(late + self.descs)
        self.ci, self.off, self.descs = 0, 0, []
        self.dws.clear()


def wgrad_batch(device):
    """A WgradBatch, or None when grouping is switched off (conv_wgrad then reduces per layer)."""
    return WgradBatch(device) if _WGRAD_GROUPED else None


def conv_wgrad(x, dout, g: ConvGeom, like: torch.Tensor, precision: str, row_mask=None, out_scale: float = 1.0, batch=None, rows=None):
    """Gradient of the layer's parameter, returned in the parameter's own layout (shape of ``like``), times out_scale.
    With ``batch`` (a WgradBatch of the CURRENT stream) only the partial sums are launched; batch.flush() completes dw.
    rows = (row_pos, count) from mask_compact: the contraction runs over those output positions only (pass no row_mask)."""
    assert rows is None or row_mask is None
    assert x.dtype == dout.dtype
    dw = torch.empty_like(like)
    ws = batch.slab(g.wgrad_ws) if batch is not None else _workspace(g.wgrad_ws, x.device)
    plan = g.plan(x.device)
    s_co, s_tap, s_ci = g.strides
    h16 = x.dtype != torch.float32
    s3 = 1 if (split3(precision) and not h16) else 0          # fp32 tensors (heads, GRU) take the 3-product split in the f16 mode too
    feat = (WGRAD_MASK if row_mask is not None else 0) | (WGRAD_ROWS if rows is not None else 0) | (WGRAD_SPLIT3 if s3 else 0)
    sym = _wgrad_symbol(g, g.wgrad_route(_abf(x), feat), x.dtype, s3)
    if batch is not None and batch.group_jobs and h16 and row_mask is None:
        fam, tiles, _ = g.wgrad_group(_abf(x))
        if fam:
            xa, da = _act(x), _act(dout)
            job = _C.TriWgradJob(_C.C.pointer(g.desc), ptr(xa), ptr(da), ptr(plan), ptr(ws), ws.numel(), ptr(dw), s_co, s_tap, s_ci, g.cin,
                                 float(out_scale), ptr(rows[0]) if rows else None, ptr(rows[1]) if rows else None)
            batch.add_job(fam, tiles, job, (xa, da, ws, dw, plan, rows), _flops(g, rows), sym)
            batch.dws[dw.data_ptr()] = dw
            return dw
    if batch is not None:
        batch.dws[dw.data_ptr()] = dw
        desc = _C.TriWgradReduce()
        check(_timed(sym, _flops(g, rows, row_mask),
                     lambda: lib().tri_conv_wgrad_partial(_C.C.byref(g.desc), ptr(_act(x)), ptr(_act(dout)), ptr(row_mask), ptr(plan),
                                                          ptr(ws), ws.numel(), ptr(dw), s_co, s_tap, s_ci, g.cin, s3, _abf(x),
                                                          float(out_scale), ptr(rows[0]) if rows else None,
                                                          ptr(rows[1]) if rows else None, _C.C.byref(desc), stream())),
              "tri_conv_wgrad_partial")
        batch.descs.append(desc)
        return dw
    check(_timed(sym, _flops(g, rows, row_mask),
                 lambda: lib().tri_conv_wgrad(_C.C.byref(g.desc), ptr(_act(x)), ptr(_act(dout)), ptr(row_mask), ptr(plan), ptr(ws),
                                              ws.numel(), ptr(dw), s_co, s_tap, s_ci, g.cin, s3, _abf(x), float(out_scale),
                                              ptr(rows[0]) if rows else None, ptr(rows[1]) if rows else None, stream())),
          "tri_conv_wgrad")
    return dw


# ------------------------------------------------------------------------------------------------ BatchNorm
class BNCoeffs:
    __slots__ = ("mean", "invstd", "scale", "shift")

    def __init__(self, C, device):
        buf = torch.empty((4, C), dtype=torch.float32, device=device)
        self.mean, self.invstd, self.scale, self.shift = buf[0], buf[1], buf[2], buf[3]


# ---- optional synchronised BatchNorm (SURVEY 8e "BatchNorm caveat") ---------------------------------------------------------------
# Default (like the reference under Lightning DDP without sync_batchnorm): per-rank statistics.  set_sync_bn(True) makes every
# BatchNorm of the towers use GLOBAL-batch statistics - one SUM all-reduce of the per-channel (sum, sum of squares) record and of the
# row count in the forward, one of the (sum g, sum g*y) record in the backward (the parameter gradients dgamma / dbeta stay the LOCAL
# sums: the gradient all-reduce of the step adds the ranks up) - so N ranks reproduce the single-process run on the global batch
# (tests/test_gpu_dp.py::test_sync_bn_two_ranks_reproduce_the_single_process_global_batch).  25 + 25 small collectives per step: a
# parity mode, eager only (the collectives cannot sit inside a captured tower), never the benchmarked configuration.
_SYNC_BN = False


def set_sync_bn(flag: bool):
    global _SYNC_BN
    _SYNC_BN = bool(flag)


def _sync_world() -> int:
    if not _SYNC_BN:
        return 1
    import torch.distributed as dist
    return dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1


def _sync_sum(t: torch.Tensor) -> torch.Tensor:
    from .parallel import all_reduce_sum                  # (host-staged under gloo, RCCL under nccl)
    if t.dtype == torch.int32:                             # gloo has no int32 SUM on every build: go through int64
        u = t.to(torch.int64)
        all_reduce_sum(u)
        return u.to(torch.int32)
    all_reduce_sum(t)
    return t


def bn_finalize(stats, C, gamma, beta, running_mean, running_var, nbt, count_dev=None, count_host=0, momentum=0.1, eps=1e-5):
    world = _sync_world()
    if world > 1:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("sync_bn: the BatchNorm collectives cannot be captured into a HIP graph - run the step eagerly")
        stats = _sync_sum(stats.sum(0, keepdim=True).contiguous())
        if count_dev is not None:
            count_dev = _sync_sum(count_dev.clone())
        else:
            count_host = int(count_host) * world
    co = BNCoeffs(C, stats.device)
    check(lib().tri_bn_finalize(ptr(stats), stats.shape[0], C, ptr(count_dev), int(count_host), ptr(gamma), ptr(beta),
                                ptr(running_mean), ptr(running_var), ptr(nbt), momentum, eps, ptr(co.mean), ptr(co.invstd),
                                ptr(co.scale), ptr(co.shift), stream()), "tri_bn_finalize")
    return co


def bn_eval_coeffs(C, gamma, beta, running_mean, running_var, eps=1e-5):
    co = BNCoeffs(C, gamma.device)
    check(lib().tri_bn_eval_coeffs(C, ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var), eps, ptr(co.mean),
                                   ptr(co.invstd), ptr(co.scale), ptr(co.shift), stream()), "tri_bn_eval_coeffs")
    return co


def bn_act(y, co: BNCoeffs, relu=True, res=None, res_co: BNCoeffs | None = None):
    C = y.shape[-1]
    out = torch.empty_like(y)
    check(lib().tri_bn_act(ptr(_act(y)), ptr(co.scale), ptr(co.shift), ptr(res), ptr(res_co.scale) if res_co else None,
                           ptr(res_co.shift) if res_co else None, ptr(out), y.numel() // C, C, 1 if relu else 0, _abf(y), stream()),
          "tri_bn_act")
    return out


def relu_bwd(dout, out, inplace=True):
    g = dout if inplace else torch.empty_like(dout)
    check(lib().tri_relu_bwd(ptr(_act(dout)), ptr(out), ptr(g), dout.numel(), _abf(dout), stream()), "tri_relu_bwd")
    return g


def _bn_bwd_finalize(partial, nblk, C, count_dev, count_host, gamma, co: "BNCoeffs", out_scale):
    """tri_bn_bwd_finalize -> buf [5, C] = (dgamma, dbeta, c1, c2, c3).  Under sync_bn the apply coefficients come from the GLOBAL
    (all-reduced) sums and row count, dgamma / dbeta from this rank's own sums."""
    buf = torch.empty((5, C), dtype=torch.float32, device=partial.device)
    check(lib().tri_bn_bwd_finalize(ptr(partial), nblk, C, ptr(count_dev), int(count_host), ptr(gamma), ptr(co.mean),
                                    ptr(co.invstd), ptr(buf[0]), ptr(buf[1]), ptr(buf[2]), ptr(buf[3]), ptr(buf[4]), float(out_scale), stream()),
          "tri_bn_bwd_finalize")
    world = _sync_world()
    if world > 1:
        tot = _sync_sum(partial.sum(0, keepdim=True).contiguous())
        if count_dev is not None:
            count_dev = _sync_sum(count_dev.clone())
        else:
            count_host = int(count_host) * world
        gbuf = torch.empty((5, C), dtype=torch.float32, device=partial.device)
        check(lib().tri_bn_bwd_finalize(ptr(tot), 1, C, ptr(count_dev), int(count_host), ptr(gamma), ptr(co.mean), ptr(co.invstd), ptr(gbuf[0]),
                                        ptr(gbuf[1]), ptr(gbuf[2]), ptr(gbuf[3]), ptr(gbuf[4]), float(out_scale), stream()), "tri_bn_bwd_finalize")
        buf = torch.stack([buf[0], buf[1], gbuf[2], gbuf[3], gbuf[4]])
    return buf


_BN_SMALL = True                                                    # one-launch BatchNorm backward of tiny tensors (A/B switch dropped in round 6)


def _bn_bwd_finish(y, g, partial, co: BNCoeffs, gamma, count_dev, count_host, out_scale, dy, row_mask=None, keep_inactive=False, rows=None,
                   rs=None, rb=None, relu_out=None, g_masked=None):
    """The last two stages of every BatchNorm backward that has its sums ("BatchNorm backward by caller"):
    tri_bn_bwd_finalize over partial [nblk, 2, C], then ONE apply pass into dy (may be g) -> (dy, dgamma, dbeta).  The apply is dense, or
    walks the dense grid by row_mask (keep_inactive: rows with 0 stay unwritten instead of zeroed), or walks the row list rows =
    (row_pos, count) and touches no other row.  rs / rb (ReLU scale / shift), relu_out, g_masked: the mask operands of bn_bwd."""
    C = y.shape[-1]
    buf = _bn_bwd_finalize(partial, partial.shape[0], C, count_dev, count_host, gamma, co, out_scale)
    if rows is not None:
        check(lib().tri_bn_bwd_apply_rows(ptr(y), ptr(g), ptr(buf[2]), ptr(buf[3]), ptr(buf[4]), ptr(dy), C, ptr(rows[0]), ptr(rows[1]),
                                          rows[0].numel(), _abf(y), stream()), "tri_bn_bwd_apply_rows")
    else:
        check(lib().tri_bn_bwd_apply(ptr(y), ptr(g), ptr(buf[2]), ptr(buf[3]), ptr(buf[4]), ptr(row_mask), ptr(dy), y.numel() // C, C, ptr(rs), ptr(rb),
                                     ptr(relu_out), ptr(g_masked), 1 if keep_inactive else 0, _abf(y), stream()), "tri_bn_bwd_apply")
    return dy, buf[0], buf[1]


def bn_bwd(y, g, co: BNCoeffs, gamma, count_dev=None, count_host=0, row_mask=None, inplace=True, relu=False, relu_out=None,
           g_masked=None, out_scale: float = 1.0, keep_inactive: bool = False, partial=None):
    # row_mask: rows with 0 are never read by either pass (their y / g may be unwritten) and come out as zeros in dy
    """Returns (dy, dgamma, dbeta).  g = gradient w.r.t. the BN output (already activation-masked), or - with relu=True -
    w.r.t. relu(bn(y)): the ReLU mask is then recomputed from y inside the two passes (no separate relu_bwd pass), or -
    with relu_out - w.r.t. relu(bn(y) + residual) whose saved output is relu_out; g_masked (may alias g) then receives
    g * (relu_out > 0), the gradient of the pre-activation sum that the residual branch needs too.
    out_scale multiplies dgamma / dbeta only (f16 mode: g and dy carry F16_GRAD_SCALE, parameter gradients do not).
    partial: sums [nblk, 2, C] that the pass which produced g left behind (conv_dgrad(bn_sums=...)), in place of this function's own."""
    rs, rb = (co.scale, co.shift) if relu else (None, None)
    C = y.shape[-1]
    M = y.numel() // C
    assert y.dtype == g.dtype
    dy = g if inplace else torch.empty_like(g)
    if partial is None and _BN_SMALL and M <= 512 and C % 8 == 0 and C >= 64 and _sync_world() == 1:
        # tiny tensors (deepest voxel level): sums, coefficients and the apply pass in ONE launch (tri_bn_bwd_small; slower than the
        # three passes from ~1 k rows on - its loads are 16 bytes per cache line)
        buf = torch.empty((2, C), dtype=torch.float32, device=y.device)
        check(lib().tri_bn_bwd_small(ptr(_act(y)), ptr(_act(g)), M, C, ptr(count_dev), int(count_host), ptr(gamma), ptr(co.mean), ptr(co.invstd),
                                     ptr(rs), ptr(rb), ptr(relu_out), ptr(g_masked), ptr(row_mask), 1 if keep_inactive else 0, ptr(dy), ptr(buf[0]),
                                     ptr(buf[1]), float(out_scale), _abf(y), stream()), "tri_bn_bwd_small")
        return dy, buf[0], buf[1]
    if partial is None:
        partial = torch.empty((lib().tri_bn_bwd_num_blocks(M), 2, C), dtype=torch.float32, device=y.device)
        check(lib().tri_bn_bwd_reduce(ptr(_act(y)), ptr(_act(g)), M, C, ptr(partial), ptr(rs), ptr(rb), ptr(relu_out), ptr(row_mask), _abf(y), stream()),
              "tri_bn_bwd_reduce")
    assert partial.shape[1:] == (2, C)
    return _bn_bwd_finish(y, g, partial, co, gamma, count_dev, count_host, out_scale, dy, row_mask=row_mask, keep_inactive=keep_inactive,
                          rs=rs, rb=rb, relu_out=relu_out, g_masked=g_masked)


def bn_bwd_pair(ya, coa: BNCoeffs, gamma_a, yb, cob: BNCoeffs, gamma_b, g, relu_out, count_host, g_masked=None, out_scale: float = 1.0):
    """BatchNorm backward of bn_a(ya) and bn_b(yb) under out = relu(bn_a(ya) + bn_b(yb)) (bn2 and the shortcut's BatchNorm of a
    down-sampling BasicBlock): -> (dya, dgamma_a, dbeta_a, dyb, dgamma_b, dbeta_b); g_masked (may alias g) receives g * (out > 0).
    Three launches for both tensors; the values of bn_bwd(ya, g, ..., relu_out=out, g_masked=...) followed by bn_bwd(yb, g_masked, ...)."""
    C = ya.shape[-1]
    M = ya.numel() // C
    assert ya.dtype == g.dtype == yb.dtype == relu_out.dtype and ya.shape == yb.shape and _sync_world() == 1
    nblk = lib().tri_bn_bwd_num_blocks(M)
    partial = torch.empty((2, nblk, 2, C), dtype=torch.float32, device=ya.device)
    check(lib().tri_bn_bwd_pair_reduce(ptr(_act(ya)), ptr(_act(yb)), ptr(_act(g)), ptr(relu_out), M, C, ptr(partial[0]), ptr(partial[1]), _abf(ya),
                                       stream()), "tri_bn_bwd_pair_reduce")
    buf = torch.empty((2, 5, C), dtype=torch.float32, device=ya.device)
    check(lib().tri_bn_bwd_pair_finalize(ptr(partial[0]), ptr(partial[1]), nblk, C, int(count_host), ptr(gamma_a), ptr(coa.mean), ptr(coa.invstd),
                                         ptr(buf[0]), ptr(gamma_b), ptr(cob.mean), ptr(cob.invstd), ptr(buf[1]), float(out_scale), stream()),
          "tri_bn_bwd_pair_finalize")
    dya, dyb = torch.empty_like(ya), torch.empty_like(yb)
    check(lib().tri_bn_bwd_pair_apply(ptr(ya), ptr(yb), ptr(g), ptr(relu_out), ptr(buf[0]), ptr(buf[1]), ptr(dya), ptr(dyb), ptr(g_masked), M, C,
                                      _abf(ya), stream()), "tri_bn_bwd_pair_apply")
    return dya, buf[0, 0], buf[0, 1], dyb, buf[1, 0], buf[1, 1]


# ------------------------------------------------------------------------------------------------ pooling
def bn_relu_pool3d_fwd(y, co: BNCoeffs, mask, B, D, C, want_mask: bool = True):
    """want_mask=False: the pooled level's site mask is not written (the caller has it from mask_pyramid); returns (pooled, None)."""
    Do = D // 2
    pooled = torch.empty((B, Do, Do, Do, C), dtype=y.dtype, device=y.device)
    mask_out = torch.empty(((B * Do ** 3 + 31) // 32 * 32,), dtype=torch.uint8, device=y.device) if want_mask else None   # every byte written by the kernel
    check(lib().tri_bn_relu_pool3d_fwd(ptr(_act(y)), ptr(co.scale), ptr(co.shift), ptr(mask), B, D, C, ptr(pooled), ptr(mask_out),
                                       _abf(y), stream()), "tri_bn_relu_pool3d_fwd")
    return pooled, mask_out


_VOX_ROWS = True                                                    # row-list passes on the fine voxel levels (A/B switch dropped in round 6)
_ROUTE_RED = True                                                     # BatchNorm-backward sums inside the row-list routing walk (A/B switch dropped in round 6)
_POOL3D_ROUTES = {(False, False): "tri_pool3d_bwd_route", (True, False): "tri_pool3d_bwd_route_rows",       # by (row list, sums)
                  (False, True): "tri_pool3d_bwd_route_reduce", (True, True): "tri_pool3d_bwd_route_rows_reduce"}


def _pool3d_bwd_route(y, co: BNCoeffs, mask, pooled, dpooled, B, D, C, rows_out=None, sums=False):
    """The routing launch of one voxel level -> (g, partial).  rows_out (the pooled level's (row_pos, count)): over the ACTIVE pooled sites
    only.  sums: the walk also leaves the BatchNorm-backward sums, partial [nblk, 2, C] (C / 4 must divide 256); otherwise partial is None."""
    assert dpooled.dtype == y.dtype and pooled.dtype == y.dtype
    g, partial = torch.empty_like(y), None
    args = (ptr(_act(y)), ptr(co.scale), ptr(co.shift), ptr(mask), ptr(pooled), ptr(_act(dpooled)), B, D, C, ptr(g))
    args += (ptr(rows_out[0]), ptr(rows_out[1])) if rows_out is not None else ()
    if sums:
        nblk = (lib().tri_pool3d_bwd_route_reduce_num_blocks if rows_out is None else lib().tri_pool3d_bwd_route_rows_num_blocks)(B, D, C)
        partial = torch.empty((nblk, 2, C), dtype=torch.float32, device=y.device)
        args += (ptr(partial),)
    name = _POOL3D_ROUTES[(rows_out is not None, sums)]
    check(getattr(lib(), name)(*args, _abf(y), stream()), name)
    return g, partial


def pool3d_bwd_route(y, co: BNCoeffs, mask, pooled, dpooled, B, D, C):
    return _pool3d_bwd_route(y, co, mask, pooled, dpooled, B, D, C)[0]


def pool3d_bwd_route_rows(y, co: BNCoeffs, mask, pooled, dpooled, B, D, C, rows_out):
    """pool3d_bwd_route over the ACTIVE pooled sites only (rows_out = the next level's (row_pos, count))."""
    return _pool3d_bwd_route(y, co, mask, pooled, dpooled, B, D, C, rows_out)[0]


def bn_bwd_rows(y, g, co: BNCoeffs, gamma, rows, out_scale: float = 1.0):
    """BatchNorm backward over a compact row list, in place on g: rows outside the list are neither read nor written."""
    C = y.shape[-1]
    scratch = torch.empty((lib().tri_bn_bwd_rows_scratch(C),), dtype=torch.uint8, device=y.device)
    buf = torch.empty((2, C), dtype=torch.float32, device=y.device)
    check(lib().tri_bn_bwd_rows(ptr(_act(y)), ptr(_act(g)), C, ptr(rows[0]), ptr(rows[1]), rows[0].numel(), ptr(gamma), ptr(co.mean),
                                ptr(co.invstd), ptr(g), ptr(buf[0]), ptr(buf[1]), float(out_scale), ptr(scratch), _abf(y), stream()),
          "tri_bn_bwd_rows")
    return g, buf[0], buf[1]


def pool3d_bn_bwd(y, co: BNCoeffs, mask, pooled, dpooled, B, D, C, gamma, count_dev, out_scale: float = 1.0, fused: bool = True,
                  keep_inactive: bool = False, rows=None, rows_out=None):
    """Backward of BatchNorm1d -> ReLU -> SparseMaxPool3d of one voxel level: (dy, dgamma, dbeta).  fused: the routing pass also leaves the
    BatchNorm-backward sums where a kernel for it exists (fused=False / TRICOLO_POOL_REDUCE=0: separate route and reduce passes).
    keep_inactive: dy rows of inactive sites stay unwritten instead of zeroed (level 0: its dy only feeds the weight gradient over the same
    mask).  rows / rows_out: (row_pos, count) of THIS level / of the pooled level.  DESIGN.md section 5, "BatchNorm backward by caller"."""
    c4 = C % 4 == 0
    sums = fused and c4 and 256 % (C // 4) == 0            # the *_reduce routing kernels: C / 4 divides 256
    lists = _VOX_ROWS and c4 and y.numel() // C > 16384    # the fine levels (13-16 % occupied) walk row lists, not the dense grid
    own = rows is not None and keep_inactive               # ... this level's own list for the whole BatchNorm backward: dy may stay unwritten
    # step one: the routing launch -> g and, from the two *_reduce forms, the sums
    if lists and sums and _ROUTE_RED and rows_out is not None:
        g, partial = _pool3d_bwd_route(y, co, mask, pooled, dpooled, B, D, C, rows_out, sums=True)
    elif lists and (rows_out is not None or own) and _sync_world() == 1:
        g, partial = _pool3d_bwd_route(y, co, mask, pooled, dpooled, B, D, C, rows_out)
    else:                                                  # coarse levels, and sync-BN without sums: the dense grid by the site mask
        own = False
        g, partial = _pool3d_bwd_route(y, co, mask, pooled, dpooled, B, D, C, sums=sums)
    # step two: the BatchNorm backward over g, in place
    if partial is not None:
        return _bn_bwd_finish(y, g, partial, co, gamma, count_dev, 0, out_scale, g, row_mask=None if own else mask, keep_inactive=keep_inactive,
                              rows=rows if own else None)
    if own:
        return bn_bwd_rows(y, g, co, gamma, rows, out_scale=out_scale)
    return bn_bwd(y, g, co, gamma, count_dev=count_dev, row_mask=mask, out_scale=out_scale, keep_inactive=keep_inactive)


def maxpool2d_fwd(x, want_arg=True, bn: BNCoeffs = None):
    """3x3/2/pad-1 max-pool; also returns the winning-tap byte map used by maxpool2d_bwd.
    With ``bn`` the pooled tensor is relu(x * scale + shift): BatchNorm + ReLU + MaxPool2d in one pass."""
    N, _, H, W, C = x.shape
    out = torch.empty((N, 1, (H + 1) // 2, (W + 1) // 2, C), dtype=x.dtype, device=x.device)
    arg = torch.empty(out.shape, dtype=torch.uint8, device=x.device) if want_arg else None
    check(lib().tri_maxpool2d_fwd(ptr(_act(x)), N, H, W, C, ptr(out), ptr(arg), ptr(bn.scale if bn else None), ptr(bn.shift if bn else None),
                                  _abf(x), stream()), "tri_maxpool2d_fwd")
    return out, arg


_STEM_POOLED = True                                                    # stem BatchNorm-backward sums from the pooled tensors (A/B switch dropped in round 6)


def _maxpool_bn_bwd_sums(y, arg, dpool, co: "BNCoeffs", gamma, pooled):
    """-> (partial [blocks, 2, C], blocks): sums of g and g * y over the stem's conv output, g = gradient of relu(bn(y)) in front of
    the max-pool.  With the forward's pooled output at hand (16-bit storage) the sums are taken over the pooled-resolution tensors."""
    N, _, H, W, C = y.shape
    if pooled is not None and _STEM_POOLED and y.dtype != torch.float32 and C % 8 == 0 and 256 % (C // 8) == 0:
        assert pooled.dtype == y.dtype and pooled.numel() == dpool.numel()
        nblk = lib().tri_maxpool_bn_bwd_pooled_num_blocks(N, H, W)
        partial = torch.empty((nblk, 2, C), dtype=torch.float32, device=y.device)
        check(lib().tri_maxpool_bn_bwd_reduce_pooled(ptr(_act(pooled)), ptr(_act(dpool)), ptr(_act(y)), ptr(arg), N, H, W, C, ptr(partial),
                                                     ptr(co.scale), ptr(co.shift), ptr(_f32(gamma.detach())), _abf(y), stream()),
              "tri_maxpool_bn_bwd_reduce_pooled")
        return partial, nblk
    nblk = lib().tri_maxpool_bn_bwd_num_blocks(N, H, W)
    partial = torch.empty((nblk, 2, C), dtype=torch.float32, device=y.device)
    check(lib().tri_maxpool_bn_bwd_reduce(ptr(_act(y)), ptr(arg), ptr(_act(dpool)), N, H, W, C, ptr(partial), ptr(co.scale), ptr(co.shift),
                                          _abf(y), stream()), "tri_maxpool_bn_bwd_reduce")
    return partial, nblk


def _maxpool_bn_bwd_coeffs(y, arg, dpool, co: "BNCoeffs", gamma, out_scale, pooled):
    """Sums and coefficients of the stem's BatchNorm backward -> buf [5, C] = (dgamma, dbeta, c1, c2, c3)."""
    partial, nblk = _maxpool_bn_bwd_sums(y, arg, dpool, co, gamma, pooled)
    return _bn_bwd_finalize(partial, nblk, y.shape[-1], None, y.numel() // y.shape[-1], gamma, co, out_scale)      # (count = N * H * W)


def _maxpool_bn_bwd_apply(y, arg, dpool, co: "BNCoeffs", buf):
    """The stem's apply pass: dy from the pooled gradient, the winning-tap map and the coefficients buf[2:5]."""
    N, _, H, W, C = y.shape
    dy = torch.empty_like(y)
    check(lib().tri_maxpool_bn_bwd_apply(ptr(y), ptr(arg), ptr(dpool), N, H, W, C, ptr(buf[2]), ptr(buf[3]), ptr(buf[4]), ptr(co.scale),
                                         ptr(co.shift), ptr(dy), _abf(y), stream()), "tri_maxpool_bn_bwd_apply")
    return dy


def maxpool_bn_bwd(y, arg, dpool, co: "BNCoeffs", gamma, out_scale: float = 1.0, pooled=None):
    """Backward of relu(bn(y)) -> MaxPool2d(3, 2, 1) in the two BatchNorm passes (no max-pool backward pass, no 4x-sized gradient
    tensor): (dy, dgamma, dbeta).  y [N,1,H,W,C], arg / dpool [N,1,H/2,W/2,C]; H, W even.  pooled: the forward's max-pool output."""
    assert dpool.dtype == y.dtype and y.shape[2] % 2 == 0 and y.shape[3] % 2 == 0
    buf = _maxpool_bn_bwd_coeffs(y, arg, dpool, co, gamma, out_scale, pooled)
    return _maxpool_bn_bwd_apply(y, arg, dpool, co, buf), buf[0], buf[1]


def _stem_wgrad_bn(x0, y, arg, dpool, co: "BNCoeffs", buf, g: "ConvGeom", like, out_scale, batch):
    """tri_conv_stem_wgrad_bn: the stem's weight gradient with the apply pass of _maxpool_bn_bwd_apply folded into its operand staging
    -> dw, or None where the library has no stem kernel for the geometry (nothing was launched; the batch gets its slab back)."""
    dw = torch.empty_like(like)
    mark = (batch.ci, batch.off) if batch is not None else None   # the arena cursor
    ws = batch.slab(g.wgrad_ws) if batch is not None else _workspace(g.wgrad_ws, y.device)
    s_co, s_tap, s_ci = g.strides
    desc = _C.TriWgradReduce()
    rc = _timed(WGRAD_FAMILIES[4].format(kh=g.kernel[1], t=_TNAME[y.dtype]), g.flops,
                lambda: lib().tri_conv_stem_wgrad_bn(_C.C.byref(g.desc), ptr(_act(x0)), ptr(_act(y)), ptr(arg), ptr(_act(dpool)), ptr(buf[2]),
                                                     ptr(buf[3]), ptr(buf[4]), ptr(co.scale), ptr(co.shift), ptr(ws), ws.numel(), ptr(dw), s_co,
                                                     s_tap, s_ci, g.cin, _abf(y), float(out_scale), _C.C.byref(desc), stream()))
    if rc == _C.TRI_ERR_UNSUPPORTED:
        if batch is not None:
            batch.ci, batch.off = mark
        return None
    check(rc, "tri_conv_stem_wgrad_bn")
    if batch is not None:
        batch.descs.append(desc)
        batch.dws[dw.data_ptr()] = dw
    else:
        check(lib().tri_wgrad_reduce_grouped(_C.C.byref(desc), 1, stream()), "tri_wgrad_reduce_grouped")
    return dw


def maxpool_bn_bwd_wgrad(x0, y, arg, dpool, co: "BNCoeffs", gamma, g: "ConvGeom", like, precision: str, out_scale: float = 1.0, batch=None,
                         pooled=None):
    """Stem backward: (dw, dgamma, dbeta) of conv -> BN -> ReLU -> MaxPool2d(3, 2, 1) (mv_cnn.py:44).  The stem has no data gradient: where
    the stem kernel runs the layer, the gradient w.r.t. the conv output - 100 MB written and re-read at the bench shape - is never stored
    (three launches).  Elsewhere the apply pass is a launch of its own in front of conv_wgrad, and a map with an odd side takes
    maxpool2d_bwd and bn_bwd ("BatchNorm backward by caller")."""
    N, _, H, W, C = y.shape
    if H % 2 == 0 and W % 2 == 0:
        assert dpool.dtype == y.dtype
        buf = _maxpool_bn_bwd_coeffs(y, arg, dpool, co, gamma, out_scale, pooled)
        dw = _stem_wgrad_bn(x0, y, arg, dpool, co, buf, g, like, out_scale, batch) if y.dtype != torch.float32 and C == 64 and _sync_world() == 1 else None
        if dw is None:
            dw = conv_wgrad(x0, _maxpool_bn_bwd_apply(y, arg, dpool, co, buf), g, like, precision, out_scale=out_scale, batch=batch)
        return dw, buf[0], buf[1]
    dy, dgamma, dbeta = bn_bwd(y, maxpool2d_bwd(arg, dpool, tuple(y.shape)), co, gamma, count_host=g.M, relu=True, out_scale=out_scale)
    return conv_wgrad(x0, dy, g, like, precision, out_scale=out_scale, batch=batch), dgamma, dbeta


def maxpool2d_bwd(arg, dout, in_shape):
    N, _, H, W, C = in_shape
    dx = torch.empty(in_shape, dtype=dout.dtype, device=dout.device)
    check(lib().tri_maxpool2d_bwd(ptr(arg), ptr(_act(dout)), N, H, W, C, ptr(dx), _abf(dout), stream()), "tri_maxpool2d_bwd")
    return dx


def avgpool_viewmax_fwd(x, B, V):
    N, _, H, W, C = x.shape
    out = torch.empty((B, C), dtype=torch.float32, device=x.device)
    arg = torch.empty((B, C), dtype=torch.int32, device=x.device)
    check(lib().tri_avgpool_viewmax_fwd(ptr(_act(x)), B, V, H * W, C, ptr(out), ptr(arg), _abf(x), stream()), "tri_avgpool_viewmax_fwd")
    return out, arg


def avgpool_viewmax_bwd(dout, arg, shape, B, V, dtype=torch.float32, scale: float = 1.0):
    N, _, H, W, C = shape
    dx = torch.empty(shape, dtype=dtype, device=dout.device)
    check(lib().tri_avgpool_viewmax_bwd(ptr(_f32(dout)), ptr(arg), B, V, H * W, C, ptr(dx), _abf(dx), float(scale), stream()),
          "tri_avgpool_viewmax_bwd")
    return dx


def cast_from_f32(x, dtype, scale: float = 1.0):
    """scale * x (fp32) stored as `dtype` - the fp32 head -> 16-bit tower boundary (one launch, no ATen copy)."""
    if dtype == torch.float32 and scale == 1.0:
        return x
    out = torch.empty(x.shape, dtype=dtype, device=x.device)
    check(lib().tri_cast_from_f32(ptr(_f32(x)), ptr(out), x.numel(), float(scale), _abf(out), stream()), "tri_cast_from_f32")
    return out


def cast_to_f32(x):
    if x.dtype == torch.float32:
        return x
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    check(lib().tri_cast_to_f32(ptr(_act(x)), ptr(out), x.numel(), _abf(x), stream()), "tri_cast_to_f32")
    return out


# ------------------------------------------------------------------------------------------------ layouts
def voxel_scatter(locs, feats, B, V, dtype=torch.float32):
    n = locs.shape[0]
    sites = B * V ** 3
    esz = torch.empty((), dtype=dtype).element_size()
    buf = torch.empty((sites * 4 * esz + (sites + 31) // 32 * 32,), dtype=torch.uint8, device=feats.device)   # grid + mask: one zero-fill
    dense = buf[:sites * 4 * esz].view(dtype).view(B, V, V, V, 4)
    mask = buf[sites * 4 * esz:]
    locs = locs.to(torch.int32).contiguous()
    check(lib().tri_voxel_scatter(ptr(locs), ptr(_f32(feats.contiguous())), n, B, V, ptr(dense), ptr(mask), _abf(dense), stream()),
          "tri_voxel_scatter")
    return dense, mask


def voxel_from_rgba(rgba_u8, dtype=torch.float32):
    """Dense RGBA u8 grids [B,4,V,V,V] (the dataset's storage format) -> (channels-last grid [B,V,V,V,4], site mask)."""
    B, C, V = rgba_u8.shape[0], rgba_u8.shape[1], rgba_u8.shape[2]
    assert C == 4 and rgba_u8.dtype == torch.uint8 and rgba_u8.shape[2:] == (V, V, V)
    dense = torch.empty((B, V, V, V, 4), dtype=dtype, device=rgba_u8.device)
    sites = B * V ** 3
    mask = torch.empty(((sites + 31) // 32 * 32,), dtype=torch.uint8, device=rgba_u8.device)      # fully written by the call
    check(lib().tri_voxel_from_rgba_u8(ptr(rgba_u8.contiguous()), B, V, ptr(dense), ptr(mask), _abf(dense), stream()), "tri_voxel_from_rgba_u8")
    return dense, mask


def mask_compact(mask, n):
    """(row_pos [n] int32 - the first `count` entries are the active positions in ascending order, count [1] int32 on the device)."""
    row_pos = torch.empty((n,), dtype=torch.int32, device=mask.device)
    count = torch.empty((1,), dtype=torch.int32, device=mask.device)
    scratch = torch.empty((lib().tri_mask_compact_scratch(n),), dtype=torch.uint8, device=mask.device)
    check(lib().tri_mask_compact(ptr(mask), n, ptr(row_pos), ptr(count), ptr(scratch), stream()), "tri_mask_compact")
    return row_pos, count


def mask_pyramid(mask0, B, V):
    """Site masks of voxel levels 1-4 (2x2x2 OR-pool of the level below) from the level-0 mask, one launch; V % 16 == 0."""
    import ctypes
    outs = [torch.empty(((B * (V >> l) ** 3 + 31) // 32 * 32,), dtype=torch.uint8, device=mask0.device) for l in range(1, 5)]
    arr = (ctypes.c_void_p * 4)(*[o.data_ptr() for o in outs])
    check(lib().tri_mask_pyramid(ptr(mask0), B, V, arr, stream()), "tri_mask_pyramid")
    return outs


MASK_MULTI_MAX = 1024 * 2048          # sites per list tri_mask_compact_multi takes (1,024 blocks: the scan is folded into the write pass)


def mask_compact_multi(masks, ns):
    """mask_compact of several masks in two launches: [(row_pos, count), ...].  Lists beyond MASK_MULTI_MAX sites go through mask_compact."""
    import ctypes
    out = [None] * len(masks)
    small = [i for i, n in enumerate(ns) if n <= MASK_MULTI_MAX]
    for i, n in enumerate(ns):
        if n > MASK_MULTI_MAX:
            out[i] = mask_compact(masks[i], n)
    for s0 in range(0, len(small), 8):
        grp = small[s0:s0 + 8]
        dev = masks[grp[0]].device
        rows = [torch.empty((ns[i],), dtype=torch.int32, device=dev) for i in grp]
        counts = torch.empty((len(grp),), dtype=torch.int32, device=dev)
        n_arr = (ctypes.c_long * len(grp))(*[ns[i] for i in grp])
        scratch = torch.empty((lib().tri_mask_compact_multi_scratch(n_arr, len(grp)),), dtype=torch.uint8, device=dev)
        m_arr = (ctypes.c_void_p * len(grp))(*[masks[i].data_ptr() for i in grp])
        r_arr = (ctypes.c_void_p * len(grp))(*[r.data_ptr() for r in rows])
        c_arr = (ctypes.c_void_p * len(grp))(*[counts[k:k + 1].data_ptr() for k in range(len(grp))])
        check(lib().tri_mask_compact_multi(m_arr, n_arr, len(grp), r_arr, c_arr, ptr(scratch), stream()), "tri_mask_compact_multi")
        for k, i in enumerate(grp):
            out[i] = (rows[k], counts[k:k + 1])
    return out


def mask_count(mask, n):
    cnt = torch.empty((1,), dtype=torch.int32, device=mask.device)
    check(lib().tri_mask_count(ptr(mask), n, ptr(cnt), stream()), "tri_mask_count")
    return cnt


def nchw3_to_nhwc4(x, dtype=torch.float32):
    N, C, H, W = x.shape
    assert C == 3
    out = torch.empty((N, 1, H, W, 4), dtype=dtype, device=x.device)
    check(lib().tri_nchw3_to_nhwc4(ptr(_f32(x.contiguous())), N, H, W, ptr(out), _abf(out), stream()), "tri_nchw3_to_nhwc4")
    return out


_CLIP_MEAN = (C_F3 := _C.C.c_float * 3)(0.48145466, 0.4578275, 0.40821073)      # general_dataset.py:88
_CLIP_STD = C_F3(0.26862954, 0.26130258, 0.27577711)


def nchw3_u8_to_nhwc4(x_u8, dtype=torch.float32, mean=None, std=None):
    """u8 images [N,3,H,W] -> channels-last [N,1,H,W,4], ToTensor + CLIP Normalize done on the device."""
    N, C, H, W = x_u8.shape
    assert C == 3 and x_u8.dtype == torch.uint8
    out = torch.empty((N, 1, H, W, 4), dtype=dtype, device=x_u8.device)
    m = C_F3(*mean) if mean is not None else _CLIP_MEAN
    sd = C_F3(*std) if std is not None else _CLIP_STD
    check(lib().tri_nchw3_u8_to_nhwc4(ptr(x_u8.contiguous()), N, H, W, _C.C.cast(m, _C.C.c_void_p), _C.C.cast(sd, _C.C.c_void_p), ptr(out),
                                      _abf(out), stream()), "tri_nchw3_u8_to_nhwc4")
    return out


def resize_output_size(H: int, W: int, size):
    """torchvision Resize's size rule: (h, w) as given, an int = the short edge becomes `size`, the long edge int(size * long / short)."""
    if isinstance(size, (tuple, list)):
        if len(size) == 1:
            return resize_output_size(H, W, int(size[0]))
        if len(size) != 2:
            raise ValueError(f"size must be an int or (H, W), got {size!r}")
        return int(size[0]), int(size[1])
    short, long = (W, H) if W <= H else (H, W)
    new_short, new_long = int(size), int(int(size) * long / short)
    return (new_long, new_short) if W <= H else (new_short, new_long)


def resize_bicubic_aa_u8(x_u8, size):
    """u8 [..., H, W] -> u8 [..., Hout, Wout]: torchvision's Resize(size, BICUBIC, antialias=True) on a uint8 tensor
    (general_dataset.py:63-65) = float32, F.interpolate(mode="bicubic", align_corners=False, antialias=True), clamp(0, 255), round
    half to even, uint8.  GPU tensors run csrc/resize.hip; host tensors take that torch expression (the loader stays usable and
    testable without a GPU), as the mesh-sampling and chamfer ops split."""
    if x_u8.dtype != torch.uint8:
        raise ValueError(f"resize_bicubic_aa_u8 takes a uint8 tensor, got {x_u8.dtype}")
    if x_u8.dim() < 2:
        raise ValueError(f"resize_bicubic_aa_u8 takes [..., H, W], got {tuple(x_u8.shape)}")
    H, W = int(x_u8.shape[-2]), int(x_u8.shape[-1])
    Ho, Wo = resize_output_size(H, W, size)
    if min(H, W, Ho, Wo) <= 0:
        raise ValueError(f"resize_bicubic_aa_u8: empty image {H}x{W} -> {Ho}x{Wo}")
    lead = tuple(x_u8.shape[:-2])
    if not x_u8.is_cuda:
        x4 = x_u8 if x_u8.dim() == 4 else x_u8.reshape(1, -1, H, W)
        y = torch.nn.functional.interpolate(x4.to(torch.float32), size=(Ho, Wo), mode="bicubic", align_corners=False, antialias=True)
        return y.clamp(0, 255).round().to(torch.uint8).reshape(lead + (Ho, Wo))
    x = x_u8.contiguous()
    out = torch.empty(lead + (Ho, Wo), dtype=torch.uint8, device=x.device)
    planes = x.numel() // (H * W)
    if planes >= 1 << 31:
        raise ValueError("resize_bicubic_aa_u8: 2^31 or more planes")
    ws = torch.empty((max(16, lib().tri_resize_bicubic_aa_workspace(H, W, Ho, Wo)),), dtype=torch.uint8, device=x.device)
    check(lib().tri_resize_bicubic_aa_u8(ptr(x), planes, H, W, ptr(out), Ho, Wo, ptr(ws), stream()), "tri_resize_bicubic_aa_u8")
    return out


# ------------------------------------------------------------------------------------------------ row ops
def l2norm_fwd(x, eps=1e-12):
    rows, D = x.shape
    z = torch.empty_like(x)
    norm = torch.empty((rows,), dtype=torch.float32, device=x.device)
    check(lib().tri_l2norm_fwd(ptr(_f32(x)), rows, D, eps, ptr(z), ptr(norm), stream()), "tri_l2norm_fwd")
    return z, norm


def l2norm_bwd(z, norm, dz, eps=1e-12):
    rows, D = z.shape
    dx = torch.empty_like(z)
    check(lib().tri_l2norm_bwd(ptr(z), ptr(norm), ptr(_f32(dz.contiguous())), rows, D, eps, ptr(dx), stream()), "tri_l2norm_bwd")
    return dx


# ------------------------------------------------------------------------------------------------ token embedding
def embedding_fwd(tokens, weight):
    """tokens [B,L] int32, weight [V,D] -> [L,B,D] (time-major, what the GRU consumes)."""
    B, L = tokens.shape
    D = weight.shape[1]
    out = torch.empty((L, B, D), dtype=torch.float32, device=weight.device)
    check(lib().tri_embedding_fwd(ptr(tokens), ptr(_f32(weight)), B, L, D, ptr(out), stream()), "tri_embedding_fwd")
    return out


def embedding_bwd(tokens, dout, V, padding_idx=0):
    B, L = tokens.shape
    D = dout.shape[-1]
    dw = torch.empty((V, D), dtype=torch.float32, device=dout.device)
    check(lib().tri_embedding_bwd(ptr(tokens), ptr(_f32(dout.contiguous())), B, L, V, D, padding_idx, ptr(dw), stream()), "tri_embedding_bwd")
    return dw


# ------------------------------------------------------------------------------------------------ retrieval
def retrieval_topk(text, shape, labels, k=5):
    """text [Nq,D], shape [Ns,D] fp32 on the GPU, labels [Nq] int32 -> (indices [Nq,k] i32, sims [Nq,k] f64, first_hit [Nq] i32)."""
    Nq, D = text.shape
    Ns = shape.shape[0]
    idx = torch.empty((Nq, k), dtype=torch.int32, device=text.device)
    sim = torch.empty((Nq, k), dtype=torch.float64, device=text.device)
    hit = torch.empty((Nq,), dtype=torch.int32, device=text.device)
    check(lib().tri_retrieval_topk(ptr(_f32(text)), ptr(_f32(shape)), ptr(labels), Nq, Ns, D, k, ptr(idx), ptr(sim), ptr(hit), stream()),
          "tri_retrieval_topk")
    return idx, sim, hit


GALLERY_MAX_K, GALLERY_MAX_D = 64, 4096                 # TRI_GALLERY_MAX_K and the D bound of csrc/gallery.hip


def retrieval_gallery(text, shape, labels=None, k=5):
    """retrieval_topk for a gallery of any size (csrc/gallery.hip; k <= 64, D <= 4096), the same bits wherever both accept the call.
    text [Nq,D], shape [Ns,D] fp32 on the GPU, labels [Nq] int32 or None -> (indices [Nq,k] i32, sims [Nq,k] f64, first_hit [Nq] i32 | None)."""
    Nq, D = text.shape
    Ns = shape.shape[0]
    idx = torch.empty((Nq, k), dtype=torch.int32, device=text.device)
    sim = torch.empty((Nq, k), dtype=torch.float64, device=text.device)
    hit = None if labels is None else torch.empty((Nq,), dtype=torch.int32, device=text.device)
    check(lib().tri_retrieval_gallery(ptr(_f32(text)), ptr(_f32(shape)), ptr(labels), Nq, Ns, D, k, ptr(idx), ptr(sim), ptr(hit), stream()),
          "tri_retrieval_gallery")
    return idx, sim, hit


def class_csr(cand_class, ncls=None):
    """Candidate classes [Nc] (any integer dtype, on the device) -> (class_off [ncls + 1] i32, class_rows [Nc] i32, ncls): the rows of
    class g are class_rows[class_off[g] : class_off[g + 1]], ascending within a class (a stable sort).  A candidate whose class is
    negative - or not below an explicit ncls - belongs to no class: it sorts behind the last class, past class_off[ncls].  Without
    ncls, ncls = max class + 1 (one host read)."""
    cc = cand_class.to(torch.int64)
    if ncls is None:
        ncls = max(int(cc.max()) + 1, 0) if cc.numel() else 0
    ncls = int(ncls)
    key = torch.where((cc >= 0) & (cc < ncls), cc, torch.full_like(cc, ncls))
    rows = torch.argsort(key, stable=True).to(torch.int32)
    counts = torch.bincount(key, minlength=ncls + 1)[:ncls]
    off = torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)]).to(torch.int32)
    return off, rows, ncls


def retrieval_classes_csr(query, cand, query_class, class_off, class_rows, ncls, k=5):
    """tri_retrieval_classes on a CSR that is already built (class_csr): query [Nq,D], cand [Nc,D] fp32 on the GPU, query_class [Nq] i32,
    class_off [ncls + 1] i32, class_rows i32; the three may be None together -> (indices [Nq,k] i32, sims [Nq,k] f64, first_hit [Nq] i32
    | None)."""
    Nq, D = query.shape
    Nc = cand.shape[0]
    idx = torch.empty((Nq, k), dtype=torch.int32, device=query.device)
    sim = torch.empty((Nq, k), dtype=torch.float64, device=query.device)
    hit = None if query_class is None else torch.empty((Nq,), dtype=torch.int32, device=query.device)
    check(lib().tri_retrieval_classes(ptr(_f32(query)), ptr(_f32(cand)), ptr(query_class), ptr(class_off), ptr(class_rows), Nq, Nc, D,
                                      int(ncls), k, ptr(idx), ptr(sim), ptr(hit), stream()), "tri_retrieval_classes")
    return idx, sim, hit


def retrieval_classes(query, cand, query_class=None, cand_class=None, k=5, ncls=None):
    """Shape -> text ranking (csrc/gallery.hip, the kernel of retrieval_gallery; k <= 64, D <= 4096): several candidates are correct for
    a query.  query [Nq,D], cand [Nc,D] fp32 on the GPU; query_class [Nq] and cand_class [Nc] integer classes (a negative cand_class:
    no class), both or neither; ncls = max cand_class + 1 unless given -> (indices [Nq,k] i32, sims [Nq,k] f64, first_hit [Nq] i32 |
    None).  first_hit[q]: the candidates ranking before the best candidate of class query_class[q]; -1 when the class is outside
    [0, ncls) or empty."""
    if (query_class is None) != (cand_class is None):
        raise ValueError("retrieval_classes: query_class and cand_class go together")
    if query_class is None:
        return retrieval_classes_csr(query, cand, None, None, None, 0, k)
    if cand_class.shape != (cand.shape[0],) or query_class.shape != (query.shape[0],):
        raise ValueError("retrieval_classes: one class per query row and one per candidate row")
    off, rows, ncls = class_csr(cand_class.to(cand.device), ncls)
    return retrieval_classes_csr(query, cand, query_class.to(query.device, torch.int32).contiguous(), off, rows, ncls, k)


# ------------------------------------------------------------------------------------------------ small dense layers
def linear_small_supported(rows, K, N):
    return bool(lib().tri_linear_small_supported(int(rows), int(K), int(N)))


def linear_small_fwd(x, w, b, act, precision):
    M, K = x.shape
    N = w.shape[0]
    y = torch.empty((M, N), dtype=torch.float32, device=x.device)
    check(_timed("linear_small_fwd_kernel", 2.0 * M * K * N,
                 lambda: lib().tri_linear_small_fwd(ptr(_f32(x)), ptr(_f32(w)), ptr(b), ptr(y), M, K, N, act, split3(precision),
                                                    stream())), "tri_linear_small_fwd")
    return y


def linear_small_bwd(x, w, out, dout, act, precision, need_dx=True, need_db=True):
    M, K = x.shape
    N = w.shape[0]
    s3 = split3(precision)
    dout = _f32(dout.contiguous())
    dw = torch.empty_like(w)
    db = torch.empty((N,), dtype=torch.float32, device=x.device) if need_db else None
    if need_dx:                                              # weight- and data-gradient tiles in one launch
        dx = torch.empty((M, K), dtype=torch.float32, device=x.device)
        check(lib().tri_linear_small_bwd(ptr(_f32(x)), ptr(dout), ptr(out), ptr(_f32(w)), ptr(dx), ptr(dw), ptr(db), M, K, N, act, s3,
                                         stream()), "tri_linear_small_bwd")
        return dx, dw, db
    check(lib().tri_linear_small_wgrad(ptr(_f32(x)), ptr(dout), ptr(out), ptr(dw), ptr(db), M, K, N, act, s3, stream()), "tri_linear_small_wgrad")
    return None, dw, db


def colsum(g):
    C = g.shape[-1]
    out = torch.empty((C,), dtype=torch.float32, device=g.device)
    check(lib().tri_colsum(ptr(_f32(g)), g.numel() // C, C, ptr(out), stream()), "tri_colsum")
    return out


def act_bwd(dout, out, act, inplace=True):
    g = dout if inplace else torch.empty_like(dout)
    check(lib().tri_act_bwd(ptr(dout), ptr(out), ptr(g), dout.numel(), act, stream()), "tri_act_bwd")
    return g


# ------------------------------------------------------------------------------------------------ GRU recurrence
def gru_mode(precision: str) -> int:
    """Operand mode of the GRU recurrence (tri_gru_fwd / tri_gru_bwd `split3`): 1 = 3-product bf16 split (bf16x3), 0 = single bf16
    products (bf16), 2 = single f16 products (f16 mode: z within 4e-5 of float64 over the 96 steps, a third of the split's MFMAs;
    TRICOLO_GRU_F16=0 keeps the split there - the A/B partner)."""
    if precision == "f16" and os.environ.get("TRICOLO_GRU_F16", "1") != "0":
        return 2
    return split3(precision)


def gru_fwd(xproj, w_hh, b_hh, B, L, precision):
    dev = xproj.device
    hs = torch.empty((2, L, B, 128), dtype=torch.float32, device=dev)
    gates = torch.empty((2, L, B, 128, 4), dtype=torch.float32, device=dev)        # (r, z, n, hn) per unit: one 16-byte access
    hfinal = torch.empty((B, 256), dtype=torch.float32, device=dev)
    check(lib().tri_gru_fwd(ptr(_f32(xproj)), ptr(_f32(w_hh)), ptr(_f32(b_hh)), B, L, ptr(hs), ptr(gates), ptr(hfinal),
                            gru_mode(precision), stream()), "tri_gru_fwd")
    return hfinal, hs, gates


def gru_bwd(dhfinal, w_hh, hs, gates, B, L, precision):
    dev = hs.device
    dgi = torch.empty((L * B, 768), dtype=torch.float32, device=dev)
    dgh = torch.empty((2, L * B, 384), dtype=torch.float32, device=dev)
    hprev = torch.empty((2, L * B, 128), dtype=torch.float32, device=dev)
    dbias = torch.empty(((B + 15) // 16, 2, 4, 128), dtype=torch.float32, device=dev)
    check(lib().tri_gru_bwd(ptr(_f32(dhfinal.contiguous())), ptr(_f32(w_hh)), ptr(hs), ptr(gates), B, L, ptr(dgi), ptr(dgh), ptr(hprev),
                            ptr(dbias), gru_mode(precision), stream()), "tri_gru_bwd")
    return dgi, dgh, hprev, dbias


# ------------------------------------------------------------------------------------------------ NT-Xent
def copy_segments(pairs):
    """[(src, dst), ...] (<= 8 contiguous fp32 tensors each way, equal sizes per pair) copied in ONE launch."""
    n = len(pairs)
    PA, LA = _C.C.c_void_p * n, _C.C.c_long * n
    for s, d in pairs:
        assert s.numel() == d.numel() and s.is_contiguous() and d.is_contiguous() and s.dtype == d.dtype == torch.float32
    check(lib().tri_copy_segments(PA(*[ptr(s) for s, _ in pairs]), PA(*[ptr(d) for _, d in pairs]), LA(*[s.numel() for s, _ in pairs]), n,
                                  stream()), "tri_copy_segments")


def gru_bias_grads(dbias):
    """dbias [nchunk, 2, 4, 128] from gru_bwd -> (db_ih_f, db_hh_f, db_ih_r, db_hh_r), [384] each, one launch."""
    out = torch.empty((4, 384), dtype=torch.float32, device=dbias.device)
    check(lib().tri_gru_bias_grads(ptr(_f32(dbias)), dbias.shape[0], ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]), stream()),
          "tri_gru_bias_grads")
    return out[0], out[1], out[2], out[3]


MAX_LOGIT_SCALE = math.log(100.0)                 # CLIP's clamp on its learned logit scale


def _logit_scale(logit_scale, like):
    """The learnable temperature of the NT-Xent calls: a 0-d / one-element fp32 tensor on the embeddings' device, read BY THE KERNELS
    (1 / T = exp(clamp(logit_scale, 0, max_logit_scale))) - never copied, so a captured graph follows in-place updates."""
    if not (isinstance(logit_scale, torch.Tensor) and logit_scale.numel() == 1 and logit_scale.dtype == torch.float32
            and logit_scale.device == like.device):
        raise RuntimeError("ntxent: logit_scale must be a one-element fp32 tensor on the embeddings' device")
    return logit_scale.detach()


def ntxent_fwd(za, zb, temperature, alpha, norm=True, *, logit_scale=None, max_logit_scale=MAX_LOGIT_SCALE):
    """Loss only; returns (loss, workspace) - hand the workspace to ntxent_bwd.  With `logit_scale` (device scalar) the temperature is
    learnable: exp(-clamp(logit_scale, 0, max_logit_scale)), read on the device; `temperature` is ignored and may be None."""
    B, D = za.shape
    loss = torch.empty((), dtype=torch.float32, device=za.device)
    if logit_scale is not None:
        nbytes = lib().tri_ntxent_ls_workspace(2, B, D)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=za.device)
        check(lib().tri_ntxent_ls_fwd_bwd(ptr(_f32(za)), ptr(_f32(zb)), B, D, ptr(_logit_scale(logit_scale, za)), float(max_logit_scale),
                                          float(alpha), 1 if norm else 0, ptr(loss), None, None, None, ptr(ws), nbytes, stream()),
              "tri_ntxent_ls_fwd_bwd")
        return loss, ws
    nbytes = lib().tri_ntxent_workspace(B, D)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=za.device)
    check(lib().tri_ntxent_fwd_bwd(ptr(_f32(za)), ptr(_f32(zb)), B, D, float(temperature), float(alpha), 1 if norm else 0, ptr(loss), None,
                                   None, ptr(ws), nbytes, stream()), "tri_ntxent_fwd_bwd")
    return loss, ws


def ntxent_bwd(za, zb, ws, temperature, alpha, norm=True, dloss=None, *, logit_scale=None, max_logit_scale=MAX_LOGIT_SCALE):
    """(dza, dzb) times the upstream scalar dloss (device tensor) in one launch; with `logit_scale` (dza, dzb, dlogit_scale) in two."""
    B, D = za.shape
    dza, dzb = torch.empty_like(za), torch.empty_like(zb)
    if logit_scale is not None:
        dls = torch.empty((), dtype=torch.float32, device=za.device)
        check(lib().tri_ntxent_ls_bwd(ptr(_f32(za)), ptr(_f32(zb)), B, D, ptr(_logit_scale(logit_scale, za)), float(max_logit_scale), float(alpha),
                                      1 if norm else 0, ptr(dloss), ptr(dza), ptr(dzb), ptr(dls), ptr(ws), ws.numel(), stream()), "tri_ntxent_ls_bwd")
        return dza, dzb, dls
    check(lib().tri_ntxent_bwd(ptr(_f32(za)), ptr(_f32(zb)), B, D, float(temperature), float(alpha), 1 if norm else 0, ptr(dloss), ptr(dza),
                               ptr(dzb), ptr(ws), ws.numel(), stream()), "tri_ntxent_bwd")
    return dza, dzb


TIMELINE = None      # tools/step_timeline.py sets {"buf": int64 device tensor, "names": []}: stamp() then timestamps the stream


def stamp(name: str):
    """Device-side timestamp of this point of the current stream (no-op unless a timeline is being recorded)."""
    tl = TIMELINE
    if tl is None:
        return
    idx = len(tl["names"])
    if idx >= tl["buf"].numel():
        return
    tl["names"].append(name)
    check(lib().tri_debug_stamp(tl["buf"].data_ptr() + 8 * idx, stream()), "tri_debug_stamp")


DEBUG_KEEP = None            # dict: debugging tools park intermediate tensors here (tools/r6/determinism.py)
_ONES = {}


def one(device) -> torch.Tensor:
    """A cached 0-d fp32 one on `device`: `loss.backward(gradient=ops.one(loss.device))` spares autograd's fill launch per step."""
    device = torch.device(device)
    t = _ONES.get(device)
    if t is None:
        if torch.cuda.is_current_stream_capturing():
            # created inside a capture its fill kernel would only be RECORDED: an eager use before the first replay would read
            # uninitialised memory.  FusedAdam.prepare() creates it ahead of any capture; anything else must call ops.one() eagerly first.
            raise RuntimeError("ops.one(): first use inside a HIP-graph capture - call ops.one(device) (or FusedAdam.prepare()) before capturing")
        t = torch.ones((), dtype=torch.float32, device=device)
        _ONES[device] = t
    return t


def ntxent_multi_supported(B: int, D: int, M: int) -> bool:
    return M in (2, 3) and 1 <= B <= 512 and 4 <= D <= 2048 and D % 4 == 0


def _multi_args(zs, workspace=None, dpairs=None):
    """The pair plumbing of the all-pairs calls over the M = 2 / 3 embeddings `zs`.  head = (zp, M, B, D) are their leading arguments
    (zp: HOST array of the device pointers).  Forward (workspace = the library's size function): (head, P, losses [P + 1], workspace
    tensor); backward: (head, dp, dzs, dzp) = HOST array of the upstream pair gradients (None without), the gradient tensors and
    their HOST array."""
    M = len(zs)
    B, D = zs[0].shape
    P = M * (M - 1) // 2
    arr = lambda ts: (_C.C.c_void_p * len(ts))(*[ptr(t) for t in ts])     # noqa: E731
    head = (arr([_f32(z) for z in zs]), M, B, D)
    if workspace is not None:
        losses = torch.empty((P + 1,), dtype=torch.float32, device=zs[0].device)
        return head, P, losses, torch.empty((workspace(M, B, D),), dtype=torch.uint8, device=zs[0].device)
    dzs = [torch.empty_like(z) for z in zs]
    return head, arr(dpairs) if dpairs is not None else None, dzs, arr(dzs)


def ntxent_multi_fwd(zs, temperature, alpha, norm=True, *, logit_scale=None, max_logit_scale=MAX_LOGIT_SCALE):
    """Every pair of the M = 2 / 3 embeddings `zs` at once: (losses [P + 1] = pair losses in combination order, then their
    sum; workspace for ntxent_multi_bwd).  `logit_scale`: the learnable temperature, as in ntxent_fwd."""
    if logit_scale is not None:
        head, _, losses, ws = _multi_args(zs, lib().tri_ntxent_ls_workspace)
        check(lib().tri_ntxent_multi_ls_fwd(*head, ptr(_logit_scale(logit_scale, zs[0])), float(max_logit_scale), float(alpha), 1 if norm else 0,
                                            ptr(losses), ptr(ws), ws.numel(), stream()), "tri_ntxent_multi_ls_fwd")
        return losses, ws
    head, _, losses, ws = _multi_args(zs, lib().tri_ntxent_multi_workspace)
    check(lib().tri_ntxent_multi_fwd(*head, float(temperature), float(alpha), 1 if norm else 0, ptr(losses), ptr(ws), ws.numel(),
                                     stream()), "tri_ntxent_multi_fwd")
    return losses, ws


def ntxent_multi_bwd(zs, ws, temperature, alpha, norm=True, dpairs=None, dtotal=None, *, logit_scale=None, max_logit_scale=MAX_LOGIT_SCALE):
    """Gradients of all M embeddings in one launch; dpairs (list of 0-d device tensors or None) / dtotal are the upstream
    gradients of the pair losses / of their sum.  With `logit_scale` the list ends with dlogit_scale (0-d; one launch more)."""
    head, dp, dzs, dzp = _multi_args(zs, dpairs=dpairs)
    if logit_scale is not None:
        dls = torch.empty((), dtype=torch.float32, device=zs[0].device)
        check(lib().tri_ntxent_multi_ls_bwd(*head, ptr(_logit_scale(logit_scale, zs[0])), float(max_logit_scale), float(alpha), 1 if norm else 0,
                                            dp, ptr(dtotal), dzp, ptr(dls), ptr(ws), ws.numel(), stream()), "tri_ntxent_multi_ls_bwd")
        return dzs + [dls]
    check(lib().tri_ntxent_multi_bwd(*head, float(temperature), float(alpha), 1 if norm else 0, dp, ptr(dtotal), dzp, ptr(ws),
                                     ws.numel(), stream()), "tri_ntxent_multi_bwd")
    return dzs


def ntxent_fwd_bwd(za, zb, temperature, alpha, norm=True, want_grad=True, *, logit_scale=None, max_logit_scale=MAX_LOGIT_SCALE):
    B, D = za.shape
    loss = torch.empty((), dtype=torch.float32, device=za.device)
    dza = torch.empty_like(za) if want_grad else None
    dzb = torch.empty_like(zb) if want_grad else None
    if logit_scale is not None:                    # (loss, dza, dzb, dlogit_scale)
        dls = torch.empty((), dtype=torch.float32, device=za.device) if want_grad else None
        nbytes = lib().tri_ntxent_ls_workspace(2, B, D)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=za.device)
        check(lib().tri_ntxent_ls_fwd_bwd(ptr(_f32(za.contiguous())), ptr(_f32(zb.contiguous())), B, D, ptr(_logit_scale(logit_scale, za)),
                                          float(max_logit_scale), float(alpha), 1 if norm else 0, ptr(loss), ptr(dza), ptr(dzb), ptr(dls), ptr(ws),
                                          nbytes, stream()), "tri_ntxent_ls_fwd_bwd")
        return loss, dza, dzb, dls
    nbytes = lib().tri_ntxent_workspace(B, D)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=za.device)
    check(lib().tri_ntxent_fwd_bwd(ptr(_f32(za.contiguous())), ptr(_f32(zb.contiguous())), B, D, float(temperature), float(alpha),
                                   1 if norm else 0, ptr(loss), ptr(dza), ptr(dzb), ptr(ws), nbytes, stream()), "tri_ntxent_fwd_bwd")
    return loss, dza, dzb


# ------------------------------------------------------------------------------------------------ Triplet loss
def triplet_fwd(zis, zls, margin):
    """Loss only; returns (loss, counts int32 [2] = (|S|, |H|), workspace) - hand the workspace to triplet_bwd."""
    B, D = zis.shape
    loss = torch.empty((), dtype=torch.float32, device=zis.device)
    counts = torch.empty((2,), dtype=torch.int32, device=zis.device)
    nbytes = lib().tri_triplet_workspace(B, D)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=zis.device)
    check(lib().tri_triplet_fwd(ptr(_f32(zis)), ptr(_f32(zls)), B, D, float(margin), ptr(loss), ptr(counts), ptr(ws), nbytes, stream()),
          "tri_triplet_fwd")
    return loss, counts, ws


def triplet_bwd(zis, zls, ws, margin, dloss):
    """(dzis, dzls) times the upstream scalar dloss (device tensor) in one launch."""
    B, D = zis.shape
    dzis, dzls = torch.empty_like(zis), torch.empty_like(zls)
    check(lib().tri_triplet_bwd(ptr(_f32(zis)), ptr(_f32(zls)), B, D, float(margin), ptr(_f32(dloss)), ptr(dzis), ptr(dzls), ptr(ws),
                                ws.numel(), stream()), "tri_triplet_bwd")
    return dzis, dzls


def triplet_multi_supported(B: int, D: int, M: int) -> bool:
    return M in (2, 3) and 2 <= B <= 512 and 4 <= D <= 2048 and D % 4 == 0


def triplet_multi_fwd(zs, margin):
    """Every pair of the M = 2 / 3 embeddings `zs` at once: (losses [P + 1] = pair losses in combination order, then their
    sum; counts int32 [P, 2] = (|S|, |H|) per pair; workspace for triplet_multi_bwd)."""
    head, P, losses, ws = _multi_args(zs, lib().tri_triplet_multi_workspace)
    counts = torch.empty((P, 2), dtype=torch.int32, device=zs[0].device)
    check(lib().tri_triplet_multi_fwd(*head, float(margin), ptr(losses), ptr(counts), ptr(ws), ws.numel(), stream()), "tri_triplet_multi_fwd")
    return losses, counts, ws


def triplet_multi_bwd(zs, ws, margin, dpairs=None, dtotal=None):
    """Gradients of all M embeddings in one launch; dpairs (list of 0-d device tensors or None) / dtotal are the upstream
    gradients of the pair losses / of their sum."""
    head, dp, dzs, dzp = _multi_args(zs, dpairs=dpairs)
    check(lib().tri_triplet_multi_bwd(*head, float(margin), dp, ptr(dtotal), dzp, ptr(ws), ws.numel(), stream()), "tri_triplet_multi_bwd")
    return dzs


# ------------------------------------------------------------------------------------------------ shape F1 / chamfer
def _cloud_lengths(lengths, N, device):
    if lengths is None:
        return None
    if lengths.dtype != torch.int64 or lengths.shape != (N,) or lengths.device != device or not lengths.is_contiguous():
        raise ValueError(f"lengths must be a contiguous int64 tensor of shape ({N},) on {device}")
    return lengths


def _cloud(x, name):
    if x.dim() != 3 or x.shape[-1] != 3 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError(f"{name} must be a contiguous float32 tensor of shape [N, S, 3], got {tuple(x.shape)} {x.dtype}"
                         + ("" if x.is_contiguous() else " (not contiguous)"))
    return x


def nn_dist2(p, q, lengths_p=None, lengths_q=None, return_idx=False):
    """p [N, S1, 3], q [N, S2, 3] fp32 on the GPU (either side may have batch 1: shared by all N) -> d2 [N, S1] fp32, the squared
    distance of every valid point of p[n] to its nearest valid point of q[n], and with return_idx the int64 index of that point.
    lengths_* (int64 [N]): rows at and beyond a length are padding (outputs 0 / -1)."""
    _cloud(p, "p"), _cloud(q, "q")
    N = max(p.shape[0], q.shape[0])
    if p.shape[0] not in (1, N) or q.shape[0] not in (1, N) or p.shape[0] == 0 or q.shape[0] == 0:
        raise ValueError(f"batch sizes {p.shape[0]} and {q.shape[0]} do not match (one side may be 1)")
    S1, S2 = p.shape[1], q.shape[1]
    lengths_p, lengths_q = _cloud_lengths(lengths_p, N, p.device), _cloud_lengths(lengths_q, N, p.device)
    d2 = torch.empty((N, S1), dtype=torch.float32, device=p.device)
    idx = torch.empty((N, S1), dtype=torch.int64, device=p.device) if return_idx else None
    check(lib().tri_nn_dist2(ptr(p), ptr(q), ptr(lengths_p), ptr(lengths_q), N, S1, S2, int(p.shape[0] == 1 and N > 1),
                             int(q.shape[0] == 1 and N > 1), ptr(d2), ptr(idx), stream()), "tri_nn_dist2")
    return (d2, idx) if return_idx else d2


def f1_counts(d2, thresholds, lengths=None):
    """d2 [N, S] fp32 -> (counts int32 [N, T] of valid points with sqrt(d2) < t, sums fp32 [N] of d2 over the valid points)."""
    N, S = d2.shape
    T = len(thresholds)
    if not 1 <= T <= 8:
        raise ValueError("1 to 8 thresholds")
    counts = torch.empty((N, T), dtype=torch.int32, device=d2.device)
    sums = torch.empty((N,), dtype=torch.float32, device=d2.device)
    thr = (_C.C.c_float * T)(*[float(t) for t in thresholds])
    check(lib().tri_f1_counts(ptr(_f32(d2)), ptr(_cloud_lengths(lengths, N, d2.device)), N, S, thr, T, ptr(counts), ptr(sums), stream()),
          "tri_f1_counts")
    return counts, sums


def f1_finalize(count_p, count_q, sum_p, sum_q, S1, S2, eps, lengths_p=None, lengths_q=None):
    """(precision, recall, f1) fp32 [T, N] and chamfer fp32 [N] from the counts and sums of both directions."""
    N, T = count_p.shape
    out = torch.empty((3, T, N), dtype=torch.float32, device=count_p.device)
    chamfer = torch.empty((N,), dtype=torch.float32, device=count_p.device)
    check(lib().tri_f1_finalize(ptr(count_p), ptr(count_q), ptr(sum_p), ptr(sum_q), ptr(_cloud_lengths(lengths_p, N, count_p.device)),
                                ptr(_cloud_lengths(lengths_q, N, count_p.device)), N, S1, S2, T, float(eps), ptr(out[0]), ptr(out[1]),
                                ptr(out[2]), ptr(chamfer), stream()), "tri_f1_finalize")
    return out[0], out[1], out[2], chamfer


# ------------------------------------------------------------------------------------------------ mesh surface sampling
def _mesh_arg(x, name, dtype, shape_tail=None, numel=None):
    if x.dtype != dtype or not x.is_contiguous() or (shape_tail is not None and (x.dim() != 2 or x.shape[1] != shape_tail)) or \
            (numel is not None and x.shape != (numel,)):
        want = f"[*, {shape_tail}]" if shape_tail is not None else f"[{numel}]"
        raise ValueError(f"{name} must be a contiguous {dtype} tensor of shape {want}, got {tuple(x.shape)} {x.dtype}"
                         + ("" if x.is_contiguous() else " (not contiguous)"))
    return x


def _mesh_batch(verts, faces, vert_off, face_off, scale=None, face_mat=None, mat_kd=None, mat_off=None, also=None, stage=None):
    """Checks the packed batch of csrc/mesh_batch.h (meshes.MeshBatch) -> N.  stage: "render_views" or "voxelize_meshes", the calls that
    need the material tensors and take CPU tensors (for their torch restatements), all on the device of `also`, their camera or frame
    tensor; None for the sampler's calls, which have neither: a host tensor raises "no CPU fallback"."""
    if stage is None:
        for x in (verts, faces, vert_off, face_off, scale):
            ptr(x)
    elif len({x.device for x in (verts, faces, vert_off, face_off, face_mat, mat_kd, mat_off, also)}) != 1:
        raise ValueError(f"{stage}: all tensors must live on one device")
    _mesh_arg(verts, "verts", torch.float32, 3)
    if faces is not None:
        _mesh_arg(faces, "faces", torch.int32, 3)
    N = vert_off.numel() - 1
    if N < 0:
        raise ValueError("vert_off must hold N + 1 offsets")
    _mesh_arg(vert_off, "vert_off", torch.int64, numel=N + 1)
    if face_off is not None:
        _mesh_arg(face_off, "face_off", torch.int64, numel=N + 1)
    if scale is not None:
        _mesh_arg(scale, "scale", torch.float32, numel=N)
    if stage is not None:
        _mesh_arg(mat_off, "mat_off", torch.int64, numel=N + 1)
        _mesh_arg(face_mat, "face_mat", torch.int32, numel=faces.shape[0])
        _mesh_arg(mat_kd, "mat_kd", torch.float32, 3)
    return N


def _mesh_desc(N, verts, faces, vert_off, face_off, face_mat=None, mat_kd=None, mat_off=None, textures=None, mips=None, normals=None,
               brdf=None):
    """The descriptor (include/tricolo_hip.h TriMeshBatch) of a batch whose tensors the caller has checked: the seven batch tensors
    (None where a call has no use for one), then the optional groups - the five texture tensors, the pyramid pair, face_vn, mat_pbr -
    each declared in `fields` when it is given.  The tensors must outlive the call the descriptor goes into."""
    d = _C.TriMeshBatch(*(ptr(x) for x in (verts, faces, vert_off, face_off, face_mat, mat_kd, mat_off)), N)
    if textures is not None:
        d.face_uv, d.mat_tex, d.texels, d.tex_off, d.tex_size = (ptr(x) for x in textures)
        d.T, d.fields = textures[4].shape[0], d.fields | _C.TRI_MESH_TEXTURES
    if mips is not None:
        d.mip_texels, d.mip_off, d.fields = ptr(mips[0]), ptr(mips[1]), d.fields | _C.TRI_MESH_MIPS
    if normals is not None:
        d.face_vn, d.fields = ptr(normals), d.fields | _C.TRI_MESH_NORMALS
    if brdf is not None:
        d.mat_pbr, d.fields = ptr(brdf), d.fields | _C.TRI_MESH_PBR
    return d


def mesh_bbox(verts, vert_off):
    """verts fp32 [sumV, 3], vert_off int64 [N + 1] on the GPU -> bbox fp32 [N, 3, 2]: per-axis (min, max) over all vertices of a mesh."""
    N = _mesh_batch(verts, None, vert_off, None)
    bbox = torch.empty((N, 3, 2), dtype=torch.float32, device=verts.device)
    check(lib().tri_mesh_bbox(_mesh_desc(N, verts, None, vert_off, None), ptr(bbox), stream()), "tri_mesh_bbox")
    return bbox


def mesh_face_cdf(verts, faces, vert_off, face_off, scale=None, max_faces=None):
    """-> (cdf float64 [sumF], total float64 [N]): the per-mesh inclusive prefix sum of the fp32 face areas of the scaled meshes.
    max_faces: the largest face count of the batch when the caller knows it (saves reading face_off back)."""
    N = _mesh_batch(verts, faces, vert_off, face_off, scale)
    if max_faces is None:
        max_faces = int((face_off[1:] - face_off[:-1]).max()) if N else 0
    cdf = torch.empty((faces.shape[0],), dtype=torch.float64, device=verts.device)
    total = torch.empty((N,), dtype=torch.float64, device=verts.device)
    check(lib().tri_mesh_face_cdf(_mesh_desc(N, verts, faces, vert_off, face_off), ptr(scale), int(max_faces), ptr(cdf), ptr(total), stream()),
          "tri_mesh_face_cdf")
    return cdf, total


def mesh_sample_points(verts, faces, vert_off, face_off, cdf, total, num_samples, seed=0, scale=None, return_face_idx=False):
    """num_samples area-weighted surface points per mesh -> points fp32 [N, S, 3] (and face_idx int64 [N, S], local to the mesh): row
    (n, s) is a function of (seed, n, s) and mesh n alone.  cdf / total: mesh_face_cdf's, taken with the same scale."""
    N = _mesh_batch(verts, faces, vert_off, face_off, scale)
    ptr(cdf), ptr(total)
    _mesh_arg(cdf, "cdf", torch.float64, numel=faces.shape[0])
    _mesh_arg(total, "total", torch.float64, numel=N)
    S = int(num_samples)
    if S < 0:
        raise ValueError("num_samples must not be negative")
    points = torch.empty((N, S, 3), dtype=torch.float32, device=verts.device)
    idx = torch.empty((N, S), dtype=torch.int64, device=verts.device) if return_face_idx else None
    check(lib().tri_mesh_sample_points(_mesh_desc(N, verts, faces, vert_off, face_off), ptr(scale), ptr(cdf), ptr(total), S,
                                       int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(points), ptr(idx), stream()), "tri_mesh_sample_points")
    return (points, idx) if return_face_idx else points


# ------------------------------------------------------------------------------------------------ multi-view rendering
RENDER_MAX_PIXELS = 2 ** 31                                                      # csrc/raster.hip RS_MAX_PIXELS: 16 GiB of visibility keys


def _render(stage, N, batch, textures, mips, cam, H, W, yfov, znear, return_visibility, samples, normals=None, brdf=None):
    """The body of render_views and render_views_textured, whose own arguments are checked (batch: the seven tensors of the packed
    batch; textures: its five texture tensors, or None; mips: the checked pyramid pair, or None; normals: the checked face_vn, or
    None; brdf: the checked mat_pbr, or None): the camera, the limits, then tri_raster_render of csrc/raster.hip, which takes its mode
    from the groups the descriptor declares - or data.render.render_views_cpu on CPU tensors."""
    if cam.dtype != torch.float32 or cam.dim() != 3 or cam.shape[0] != N or cam.shape[2] != 12 or not cam.is_contiguous():
        raise ValueError(f"cam must be a contiguous float32 tensor of shape [{N}, views, 12], got {tuple(cam.shape)} {cam.dtype}")
    views, sumF, dev = cam.shape[1], batch[1].shape[0], batch[0].device
    if H < 0 or W < 0 or not (0.0 < float(yfov) < math.pi) or not float(znear) > 0.0:
        raise ValueError(f"{stage}: H and W must not be negative, yfov must lie in (0, pi), znear above 0")
    if sumF >= 2 ** 31:
        raise ValueError(f"{stage}: 2^31 or more faces in one batch")
    if N * views * H * W * samples >= RENDER_MAX_PIXELS or views > 65535:
        what, unit = ("pixels x 4 samples", "samples") if samples == 4 else ("pixels", "pixels")
        raise ValueError(f"{stage}: {N} meshes x {views} views x {H} x {W} {what} need a visibility buffer of "
                         f"{N * views * H * W * samples * 8} bytes; one call takes fewer than 2^31 {unit} and at most 65535 views - split the batch")
    if not batch[0].is_cuda:
        from .data.render import render_views_cpu
        return render_views_cpu(*batch, cam, H, W, yfov, znear, return_visibility, textures=textures, samples=samples, mips=mips,
                                normals=normals, brdf=brdf)
    image = torch.empty((N, views, 3, H, W), dtype=torch.uint8, device=dev)
    vis = torch.empty((N, views, H, W) + ((4,) if samples == 4 else ()), dtype=torch.int32, device=dev) if return_visibility else None
    ws = torch.empty((max(16, lib().tri_raster_workspace(sumF, N, views, H, W, samples)),), dtype=torch.uint8, device=dev)
    if brdf is not None and brdf.shape[0] == 0:                                     # a batch without a material: no row is ever read, but the
        brdf = brdf.new_zeros((1, 2))                                               # resolve kernel is chosen by a mat_pbr that is not null
    desc = _mesh_desc(N, *batch, textures=textures, mips=mips, normals=normals, brdf=brdf)
    check(lib().tri_raster_render(desc, ptr(cam), sumF, views, H, W, float(yfov), float(znear), samples, ptr(ws), ptr(image), ptr(vis), stream()),
          "tri_raster_render")
    return (image, vis) if return_visibility else image


def _render_samples(stage, samples):
    if samples not in (1, 4):
        raise ValueError(f"{stage}: samples must be 1 (the pixel centre) or 4 (the 4x rotated grid), got {samples!r}")
    return int(samples)


def _mesh_normals(stage, faces, normals):
    """Checks the corner normals a call was given for its batch (csrc/mesh_batch.h face_vn; meshes.MeshBatch.face_vn) -> normals."""
    if not torch.is_tensor(normals) or normals.device != faces.device:
        raise ValueError(f"{stage}: normals must be a tensor on the batch's device, {faces.device}")
    if normals.dtype != torch.float32 or tuple(normals.shape) != (faces.shape[0], 3, 3) or not normals.is_contiguous():
        raise ValueError(f"{stage}: normals must be a contiguous float32 tensor of shape [{faces.shape[0]}, 3, 3], got {tuple(normals.shape)} "
                         f"{normals.dtype}")
    return normals


def _mesh_pbr(stage, mat_kd, brdf):
    """Checks the PBR factors a call was given for its batch (csrc/mesh_batch.h mat_pbr; meshes.MeshBatch.mat_pbr) -> brdf."""
    if not torch.is_tensor(brdf) or brdf.device != mat_kd.device:
        raise ValueError(f"{stage}: brdf must be a tensor on the batch's device, {mat_kd.device}")
    if brdf.dtype != torch.float32 or tuple(brdf.shape) != (mat_kd.shape[0], 2) or not brdf.is_contiguous():
        raise ValueError(f"{stage}: brdf must be a contiguous float32 tensor of shape [{mat_kd.shape[0]}, 2] = (metallic, roughness) per "
                         f"material, got {tuple(brdf.shape)} {brdf.dtype}" + ("" if brdf.is_contiguous() else " (not contiguous)"))
    return brdf


def render_views(verts, faces, vert_off, face_off, face_mat, mat_kd, mat_off, cam, H, W, yfov=math.pi / 3, znear=0.05,
                 return_visibility=False, samples=1, normals=None, brdf=None):
    """Render every mesh of a packed batch (meshes.MeshBatch.pack) from every camera -> images uint8 [N, views, 3, H, W], with
    return_visibility also int32 [N, views, H, W]: the face seen at each pixel centre, local to its mesh, -1 for background.
    face_mat int32 [sumF]: a material per face, local to the mesh; mat_kd fp32 [sumM, 3] diffuse colours with mat_off int64 [N + 1];
    cam fp32 [N, views, 12]: eye, then the world-to-camera rotation row by row (data.render.pack_cameras).  The arithmetic is the
    definition (head of csrc/raster.hip): a face with a vertex nearer than znear is dropped whole - there is NO near-plane clipping
    (model_normalized.obj lies within 0.5 of its centre, the reference's camera stands 0.85 away) - both sides are drawn, flat
    Lambert shading, white background.  One call takes fewer than 2^31 faces and fewer than 2^31 pixels over all meshes and views
    (8 bytes of visibility key each); more raises before anything runs.  CPU tensors run data.render.render_views_cpu, the same
    arithmetic in torch (untuned, for checking).
    samples=4 takes coverage and depth at four positions per pixel - (96, 32), (224, 96), (32, 160), (160, 224) in 1/256 pixel from the
    pixel's top-left corner, the 4x rotated grid - by the same rules, colours every sample as a pixel is coloured and writes their
    rounded integer mean (c0 + c1 + c2 + c3 + 2) >> 2; the visibility is then int32 [N, views, H, W, 4], and one call takes fewer than
    2^31 samples.  samples=1, the default, is the pixel centre alone; anything else raises.
    normals=face_vn fp32 [sumF, 3, 3] (meshes.MeshBatch.face_vn: one normal per face corner in the order of `faces`, any length; a
    NaN in face_vn[f, 0, 0] = the face has none) turns smooth shading on: at the pixel centre - with samples=4 at each sample's own
    position - the corner normals of the winning face are interpolated with the perspective-correct weights, the result is turned
    toward the eye and lit as the flat normal is (head of csrc/raster.hip).  A face without normals, and a position where the
    interpolated normal is not finite or has no length, is shaded flat, bit for bit; visibility never changes.  The turn toward the
    eye at every position is this project's own rule.  normals=None, the default, is the call as it was.
    brdf=mat_pbr fp32 [sumM, 2] (meshes.MeshBatch.mat_pbr: metallic and roughness per material, indexed like mat_kd) replaces the
    Lambert shade by the glTF 2.0 metallic-roughness BRDF: at every position the view vector comes from the world position on the
    winning face, the normal is the flat or (with normals=) the smooth one, and the colour is clamp(0.1 base + 3 NL ((1 - F) cdiff /
    pi + F G D / (4 NL NV)), 0, 1) with base = Kd (head of csrc/raster.hip).  Metallic is clamped to [0, 1] and roughness to [0.04, 1],
    a NaN takes the lower bound, a mesh without materials takes (0.2, 0.8).  A position where the view or half vector has no length
    takes the Lambert colour, bit for bit; visibility never changes.  brdf=None, the default, is the call as it was."""
    H, W = int(H), int(W)
    samples = _render_samples("render_views", samples)
    N = _mesh_batch(verts, faces, vert_off, face_off, None, face_mat, mat_kd, mat_off, cam, stage="render_views")
    if normals is not None:
        normals = _mesh_normals("render_views", faces, normals)
    if brdf is not None:
        brdf = _mesh_pbr("render_views", mat_kd, brdf)
    return _render("render_views", N, (verts, faces, vert_off, face_off, face_mat, mat_kd, mat_off), None, None, cam, H, W, yfov, znear,
                   return_visibility, samples, normals, brdf)


def _mesh_textures(stage, faces, mat_kd, face_uv, mat_tex, texels, tex_off, tex_size):
    """Checks the five texture tensors of csrc/mesh_batch.h (meshes.MeshBatch.texture_tensors; their contents are validated where
    they are packed) -> T."""
    if any(x is None for x in (face_uv, mat_tex, texels, tex_off, tex_size)):
        raise ValueError(f"{stage}: the batch was packed without textures (MeshBatch.pack(..., face_uv_list=, mat_tex_list=, textures_list=))")
    if len({x.device for x in (faces, face_uv, mat_tex, texels, tex_off, tex_size)}) != 1:
        raise ValueError(f"{stage}: all tensors must live on one device")
    if face_uv.dtype != torch.float32 or tuple(face_uv.shape) != (faces.shape[0], 3, 2) or not face_uv.is_contiguous():
        raise ValueError(f"face_uv must be a contiguous float32 tensor of shape [{faces.shape[0]}, 3, 2], got {tuple(face_uv.shape)} {face_uv.dtype}")
    _mesh_arg(mat_tex, "mat_tex", torch.int32, numel=mat_kd.shape[0])
    _mesh_arg(texels, "texels", torch.uint8, 4)
    _mesh_arg(tex_size, "tex_size", torch.int32, 2)
    T = tex_size.shape[0]
    _mesh_arg(tex_off, "tex_off", torch.int64, numel=T + 1)
    return T


def texture_mips(texels, tex_off, tex_size):
    """The mip pyramid of every texture of a packed batch (MeshBatch.texture_tensors[2:]) -> (mip_texels u8 [sumMipTexels, 4], mip_off
    int64 [T + 1]) on the textures' device, laid out as csrc/mesh_batch.h says: texture t of size (H0, W0) has floor(log2(max(H0, W0)))
    + 1 levels of size (max(1, H0 >> l), max(1, W0 >> l)), its chain from mip_off[t], level 0 (a copy of the texture) first.  A texel
    of a level l >= 1 is the area-weighted box mean of the part of LEVEL 0 it covers, in exact integers, half rounded up; alpha 255.
    On the GPU one launch of tri_texture_mips builds all levels of all textures; the sizes (not the texels) are read back once to
    size the output and form mip_off.  CPU tensors run data.render.texture_mips_cpu, the same integers in torch.  T == 0 gives an
    empty pyramid."""
    from .meshes import TEXTURE_MAX_SIDE, mip_offsets
    if not all(torch.is_tensor(x) for x in (texels, tex_off, tex_size)) or len({x.device for x in (texels, tex_off, tex_size)}) != 1:
        raise ValueError("texture_mips: texels, tex_off and tex_size must be tensors on one device")
    _mesh_arg(texels, "texels", torch.uint8, 4)
    _mesh_arg(tex_size, "tex_size", torch.int32, 2)
    T = tex_size.shape[0]
    _mesh_arg(tex_off, "tex_off", torch.int64, numel=T + 1)
    size = tex_size.to("cpu", torch.int64)
    if T and (int(size.min()) < 1 or int(size.max()) > TEXTURE_MAX_SIDE):
        raise ValueError(f"texture_mips: every texture needs 1 <= H, W <= 2^24, got sizes from {int(size.min())} to {int(size.max())}")
    if int((size[:, 0] * size[:, 1]).sum()) != texels.shape[0]:
        raise ValueError(f"texture_mips: tex_size describes {int((size[:, 0] * size[:, 1]).sum())} texels, texels holds {texels.shape[0]}")
    if not texels.is_cuda:
        from .data.render import texture_mips_cpu
        return texture_mips_cpu(texels, tex_off, tex_size)
    off = mip_offsets(size)
    mip_off = off.to(texels.device)
    mip_texels = torch.empty((int(off[-1]), 4), dtype=torch.uint8, device=texels.device)
    check(lib().tri_texture_mips(ptr(texels), ptr(tex_off), ptr(tex_size), T, texels.shape[0], ptr(mip_off), mip_texels.shape[0],
                                 ptr(mip_texels), stream()), "tri_texture_mips")
    return mip_texels, mip_off


def _mesh_mips(stage, texels, tex_size, mips):
    """Checks the pyramid pair (texture_mips) a call was given for its textures -> (mip_texels, mip_off): one device with the batch,
    dtypes and shapes, the total tex_size asks for and mip_off, the running sum of its chain lengths - the kernels clamp every texel
    index to mip_off[T] - 1, so that table must not overstate the pyramid.  The few sizes and offsets are read back for it: a call
    with mips= waits for the stream once."""
    from .meshes import mip_offsets
    if not isinstance(mips, (tuple, list)) or len(mips) != 2 or not all(torch.is_tensor(x) for x in mips):
        raise ValueError(f"{stage}: mips must be the pair (mip_texels, mip_off) of ops.texture_mips")
    mip_texels, mip_off = mips
    if mip_texels.device != texels.device or mip_off.device != texels.device:
        raise ValueError(f"{stage}: the mip pyramid lives on {mip_texels.device}, the batch on {texels.device}: all tensors must live on one device")
    _mesh_arg(mip_texels, "mip_texels", torch.uint8, 4)
    _mesh_arg(mip_off, "mip_off", torch.int64, numel=tex_size.shape[0] + 1)
    want = mip_offsets(tex_size)
    if mip_texels.shape[0] != int(want[-1]):
        raise ValueError(f"{stage}: the pyramids of these textures hold {int(want[-1])} texels in all, mip_texels holds {mip_texels.shape[0]} - "
                         "was it built from another batch?")
    if not torch.equal(mip_off.cpu(), want):
        raise ValueError(f"{stage}: mip_off must be the running sum of the chain lengths of tex_size")
    return mip_texels, mip_off


def render_views_textured(verts, faces, vert_off, face_off, face_mat, mat_kd, mat_off, face_uv, mat_tex, texels, tex_off, tex_size, cam, H, W,
                          yfov=math.pi / 3, znear=0.05, return_visibility=False, samples=1, mips=None, normals=None, brdf=None):
    """render_views with map_Kd textures: the packed batch and its five texture tensors (MeshBatch.tensors, MeshBatch.texture_tensors).
    face_uv fp32 [sumF, 3, 2]: one (u, v) per face corner, NaN in face_uv[f, 0, 0] = the face has none; mat_tex int32 [sumM]: a
    batch-global texture index per material, -1 = none; texels u8 [sumTexels, 4] RGBA; tex_off int64 [T + 1]; tex_size int32 [T, 2]
    = (height, width), row 0 the top of the image, v = 0 its bottom.  Visibility is render_views'; a textured face is coloured
    clamp((Kd c) shade, 0, 1), c the texture at the perspective-correct (u, v) of the pixel centre - repeat wrap, bilinear, NO
    mip-maps (head of csrc/raster.hip) - and an untextured one exactly as by render_views.  Same limits; CPU tensors run the torch
    restatement of data.render.  samples=4: render_views' four samples, a textured face sampled at the (u, v) of each sample's own
    position - 4x supersampling of the texture, which eases but does not replace mip-maps.
    mips=(mip_texels, mip_off), the pair of texture_mips for these textures (MeshBatch.with_texture_mips().mip_tensors), turns
    mip-mapping on: the level of detail of a pixel - or of a sample, with samples=4 - comes from (u, v) there, one whole pixel to the
    right and one whole pixel down, rho is the longer of the two steps in texels, and the colour blends the two pyramid levels around
    log2(rho) (head of csrc/raster.hip; no LOD bias, no anisotropy).  Where the texture is magnified (rho <= 1) the colour is the one
    without mips, bit for bit; visibility never changes.  The rule is this project's own definition: no pixel of it has been compared
    with pyrender's mip-mapping.  mips=None, the default, is the call as it was.
    normals=face_vn: render_views' smooth shading, with or without mips and at either sample count; the texel is taken as before and
    multiplies Kd, the smooth shade replaces the flat one.  normals=None, the default, is the call as it was.
    brdf=mat_pbr: render_views' metallic-roughness BRDF in any of those modes; the base colour is Kd times the texel where the face is
    textured.  brdf=None, the default, is the call as it was."""
    H, W = int(H), int(W)
    samples = _render_samples("render_views_textured", samples)
    N = _mesh_batch(verts, faces, vert_off, face_off, None, face_mat, mat_kd, mat_off, cam, stage="render_views_textured")
    _mesh_textures("render_views_textured", faces, mat_kd, face_uv, mat_tex, texels, tex_off, tex_size)
    if mips is not None:
        mips = _mesh_mips("render_views_textured", texels, tex_size, mips)
    if normals is not None:
        normals = _mesh_normals("render_views_textured", faces, normals)
    if brdf is not None:
        brdf = _mesh_pbr("render_views_textured", mat_kd, brdf)
    return _render("render_views_textured", N, (verts, faces, vert_off, face_off, face_mat, mat_kd, mat_off),
                   (face_uv, mat_tex, texels, tex_off, tex_size), mips, cam, H, W, yfov, znear, return_visibility, samples, normals, brdf)


VERTEX_NORMAL_FILL = {"missing": 0, "all": 1}


def mesh_vertex_normals(verts, faces, vert_off, face_off, face_vn=None, fill="missing"):
    """Vertex normals of a packed batch (meshes.MeshBatch.pack) as corner normals -> face_vn fp32 [sumF, 3, 3], what normals= of
    render_views takes.  A definition of this project (head of csrc/mesh_normals.hip): per vertex INDEX of a mesh the fp32 cross
    products of the faces that use it - area-weighted; clamped to +-2^16 per component and rounded to fixed point at 2^36 - are summed
    with 64-bit integer atomics, so the result does not depend on the order of the faces and is bit-reproducible; a corner is that
    sum normalised in float64 and rounded to fp32.  Vertices at one position are not merged.  fill="missing": a face whose incoming
    face_vn[f, 0, 0] is not NaN keeps its nine values bit for bit, the others (all, when face_vn is None) are computed; fill="all":
    every face is computed.  A face with a corner whose sum is (0, 0, 0) - two coincident faces of opposite winding, say - gets nine
    NaNs and renders flat.  A vertex shared by more than 2^10 faces with components at the clamp would wrap its sum (modular, still
    deterministic).  Three launches, no host synchronisation.  CPU tensors run data.render.mesh_vertex_normals_cpu, the same integers
    and float64 in torch."""
    if fill not in VERTEX_NORMAL_FILL:
        raise ValueError(f"mesh_vertex_normals: fill must be one of {sorted(VERTEX_NORMAL_FILL)}, got {fill!r}")
    if not all(torch.is_tensor(x) for x in (verts, faces, vert_off, face_off)) or len({x.device for x in (verts, faces, vert_off, face_off)}) != 1:
        raise ValueError("mesh_vertex_normals: all tensors must live on one device")
    _mesh_arg(verts, "verts", torch.float32, 3)
    _mesh_arg(faces, "faces", torch.int32, 3)
    N = vert_off.numel() - 1
    if N < 0:
        raise ValueError("vert_off must hold N + 1 offsets")
    _mesh_arg(vert_off, "vert_off", torch.int64, numel=N + 1)
    _mesh_arg(face_off, "face_off", torch.int64, numel=N + 1)
    if face_vn is not None:
        face_vn = _mesh_normals("mesh_vertex_normals", faces, face_vn)
    sumV, sumF = verts.shape[0], faces.shape[0]
    if sumV >= 2 ** 31 or sumF >= 2 ** 31:
        raise ValueError("mesh_vertex_normals: 2^31 or more vertices or faces in one batch")
    if not verts.is_cuda:
        from .data.render import mesh_vertex_normals_cpu
        return mesh_vertex_normals_cpu(verts, faces, vert_off, face_off, face_vn, fill == "all")
    out = torch.empty((sumF, 3, 3), dtype=torch.float32, device=verts.device)
    ws = torch.empty((max(16, lib().tri_mesh_vertex_normals_workspace(sumV)),), dtype=torch.uint8, device=verts.device)
    check(lib().tri_mesh_vertex_normals(_mesh_desc(N, verts, faces, vert_off, face_off), sumV, sumF, VERTEX_NORMAL_FILL[fill], ptr(ws),
                                        ptr(face_vn), ptr(out), stream()), "tri_mesh_vertex_normals")
    return out


def mesh_face_colours(batch):
    """One colour per face of a meshes.MeshBatch packed with textures -> fp32 [sumF, 3]: Kd for an untextured face, else Kd times the
    mean of four bilinear samples of its texture (barycentric (1/3, 1/3, 1/3), (2/3, 1/6, 1/6), (1/6, 2/3, 1/6), (1/6, 1/6, 2/3) of
    the face's UVs, used affinely; head of csrc/raster.hip).  batch.with_face_colours(...) of it is what ops.voxelize_meshes takes to
    colour voxels from textures.  CPU tensors run data.render.mesh_face_colours_cpu, the same arithmetic in torch."""
    verts, faces, vert_off, face_off, face_mat, mat_kd, mat_off = batch.tensors
    if face_mat is None:
        raise ValueError("mesh_face_colours: the batch was packed without materials")
    N = _mesh_batch(verts, faces, vert_off, face_off, None, face_mat, mat_kd, mat_off, verts, stage="mesh_face_colours")
    _mesh_textures("mesh_face_colours", faces, mat_kd, *batch.texture_tensors)
    sumF = faces.shape[0]
    if sumF >= 2 ** 31:
        raise ValueError("mesh_face_colours: 2^31 or more faces in one batch")
    if not verts.is_cuda:
        from .data.render import mesh_face_colours_cpu
        return mesh_face_colours_cpu(*batch.tensors, *batch.texture_tensors)
    colours = torch.empty((sumF, 3), dtype=torch.float32, device=verts.device)
    check(lib().tri_mesh_face_colours(_mesh_desc(N, *batch.tensors, textures=batch.texture_tensors), sumF, ptr(colours), stream()),
          "tri_mesh_face_colours")
    return colours


# ------------------------------------------------------------------------------------------------ mesh voxelisation
VOXELIZE_SIZES = (32, 64, 128)
VOXELIZE_MAX_FACES, VOXELIZE_MAX_VOXELS = 2 ** 24, 2 ** 31                       # csrc/voxelize.hip VX_MAX_FACES, VX_MAX_VOXELS
VOXELIZE_FILL = {"surface": 0, "carve": 1}


def voxelize_meshes(verts, faces, vert_off, face_off, face_mat, mat_kd, mat_off, frame, V, fill="carve", return_labels=False):
    """Coloured voxel grids of every mesh of a packed batch (the batch of render_views) -> uint8 [N, 4, V, V, V] indexed
    [channel, x, y, z], with return_labels also uint8 [N, V, V, V]: 0 exterior, 1 surface, 2 interior.  frame fp32 [N, 4]: per mesh
    the grid's origin and cell size (data.voxelize.default_frames); a mesh with cell <= 0 or a non-finite frame gives zeros.  The
    arithmetic is the definition (head of csrc/voxelize.hip): a voxel is on the surface when its closed box overlaps a face snapped
    to 1/256 voxel, its colour is the rounded mean of the 8-bit Kd of all overlapping faces (each weighs the same); fill="carve"
    makes every non-surface voxel with a surface voxel on all six axis rays interior, coloured like the nearest of them;
    fill="surface" keeps the shell.  Alpha is 255 on surface and interior voxels, everything is 0 elsewhere.  V is 32, 64 or 128;
    one call takes fewer than 2^24 faces and fewer than 2^31 voxels; more raises before anything runs.  CPU tensors run
    data.voxelize.voxelize_meshes_cpu, the same arithmetic in torch (untuned, for checking)."""
    V = int(V)
    if fill not in VOXELIZE_FILL:
        raise ValueError(f"voxelize_meshes: fill must be one of {sorted(VOXELIZE_FILL)}, got {fill!r}")
    N = _mesh_batch(verts, faces, vert_off, face_off, None, face_mat, mat_kd, mat_off, frame, stage="voxelize_meshes")
    if frame.dtype != torch.float32 or frame.shape != (N, 4) or not frame.is_contiguous():
        raise ValueError(f"frame must be a contiguous float32 tensor of shape [{N}, 4], got {tuple(frame.shape)} {frame.dtype}")
    sumF = faces.shape[0]
    if V not in VOXELIZE_SIZES:
        raise ValueError(f"voxelize_meshes: V must be one of {VOXELIZE_SIZES}, got {V}")
    if sumF >= VOXELIZE_MAX_FACES or N * V ** 3 >= VOXELIZE_MAX_VOXELS:
        raise ValueError(f"voxelize_meshes: {sumF} faces, {N} meshes x {V}^3 voxels; one call takes fewer than 2^24 faces and fewer "
                         "than 2^31 voxels - split the batch")
    if not verts.is_cuda:
        from .data.voxelize import voxelize_meshes_cpu
        return voxelize_meshes_cpu(verts, faces, vert_off, face_off, face_mat, mat_kd, mat_off, frame, V, VOXELIZE_FILL[fill], return_labels)
    grid = torch.empty((N, 4, V, V, V), dtype=torch.uint8, device=verts.device)
    labels = torch.empty((N, V, V, V), dtype=torch.uint8, device=verts.device) if return_labels else None
    ws = torch.empty((max(16, lib().tri_voxelize_workspace(sumF, N, V)),), dtype=torch.uint8, device=verts.device)
    check(lib().tri_voxelize_meshes(_mesh_desc(N, verts, faces, vert_off, face_off, face_mat, mat_kd, mat_off), ptr(frame), sumF, V,
                                    VOXELIZE_FILL[fill], ptr(ws), ptr(grid), ptr(labels), stream()), "tri_voxelize_meshes")
    return (grid, labels) if return_labels else grid


# ------------------------------------------------------------------------------------------------ Adam
def adam_tick(step):
    check(lib().tri_adam_tick(ptr(step), stream()), "tri_adam_tick")


def adam_guard(g, step):
    """Per-step overflow guard over a flat gradient: flags the attempt in step[2] when g holds an inf / NaN (call before adam_tick)."""
    check(lib().tri_adam_guard(ptr(_f32(g)), g.numel(), ptr(step), stream()), "tri_adam_guard")


def adam_guard_segments(grad_ptrs, grad_starts, n, step):
    check(lib().tri_adam_guard_segments(ptr(grad_ptrs), ptr(grad_starts), grad_starts.numel(), n, ptr(step), stream()), "tri_adam_guard_segments")


def adam_step_segments(p, grad_ptrs, grad_starts, m, v, step, lr, b1, b2, eps, wd, gscale=1.0, lr_dev=None):
    """Fused Adam over the flat buffers with the gradients read in place through a device (pointer, start) table.
    lr_dev (1-element fp32 device tensor) overrides lr at run time: a captured graph then follows an LR schedule."""
    check(lib().tri_adam_step_segments(ptr(p), ptr(grad_ptrs), ptr(grad_starts), grad_starts.numel(), ptr(m), ptr(v), p.numel(), ptr(step),
                                       lr, ptr(lr_dev), b1, b2, eps, wd, gscale, stream()), "tri_adam_step_segments")


def adam_step(p, g, m, v, step, lr, b1, b2, eps, wd, gscale=1.0, lr_dev=None):
    check(lib().tri_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), ptr(step), lr, ptr(lr_dev), b1, b2, eps, wd, gscale, stream()),
          "tri_adam_step")


# ------------------------------------------------------------------------------------------------ gradient clipping (include/tricolo_hip.h)
def grad_norm_blocks(n: int) -> int:
    """Doubles one grad_sumsq / grad_sumsq_segments call over n elements writes (a host query: no launch)."""
    nblk = lib().tri_grad_norm_blocks(int(n))
    check(min(nblk, 0), "tri_grad_norm_blocks")
    return nblk


def _partial(partial, nblk):
    assert partial.dtype == torch.float64 and partial.is_contiguous() and partial.numel() >= nblk, "expected a contiguous float64 partial buffer of at least nblk elements"
    return partial


def grad_sumsq(g, partial) -> int:
    """partial[:nblk] = per-workgroup sums of g^2 in double over a flat fp32 gradient (any size, 4-byte alignment); returns nblk."""
    nblk = grad_norm_blocks(g.numel())
    check(lib().tri_grad_sumsq(ptr(_f32(g)), g.numel(), ptr(_partial(partial, nblk)), stream()), "tri_grad_sumsq")
    return nblk


def grad_sumsq_segments(grad_ptrs, grad_starts, n, partial) -> int:
    """The same over adam_step_segments' pointer table (null pointers are not part of the norm); n: the flat size the starts count in."""
    nblk = grad_norm_blocks(n)
    check(lib().tri_grad_sumsq_segments(ptr(grad_ptrs), ptr(grad_starts), grad_starts.numel(), n, ptr(_partial(partial, nblk)), stream()),
          "tri_grad_sumsq_segments")
    return nblk


def grad_clip_coef(partial, nblk, gscale, max_norm, rec, clipped):
    """rec[0] = |gscale| * sqrt(sum(partial[:nblk])), rec[1] = min(1, max_norm / (rec[0] + 1e-6)) (1 when the norm is not finite);
    clipped[0] += 1 when rec[1] < 1.  rec: fp32 [2], clipped: int32 [1], both on the device."""
    assert rec.dtype == torch.float32 and rec.numel() >= 2 and clipped.dtype == torch.int32 and clipped.numel() >= 1
    check(lib().tri_grad_clip_coef(ptr(_partial(partial, nblk)) if nblk else None, nblk, gscale, max_norm, ptr(rec), ptr(clipped), stream()),
          "tri_grad_clip_coef")


def adam_step_clipped(p, g, m, v, step, lr, b1, b2, eps, wd, gscale=1.0, lr_dev=None, coef_dev=None, clip_value=math.inf):
    """adam_step with the gradient multiplied by the device scalar coef_dev (None: 1) and, for a finite clip_value, clamped to
    [-clip_value, clip_value] before the weight decay is added."""
    check(lib().tri_adam_step_clipped(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), ptr(step), lr, ptr(lr_dev), b1, b2, eps, wd, gscale,
                                      ptr(coef_dev), clip_value, stream()), "tri_adam_step_clipped")


def adam_step_segments_clipped(p, grad_ptrs, grad_starts, m, v, step, lr, b1, b2, eps, wd, gscale=1.0, lr_dev=None, coef_dev=None,
                               clip_value=math.inf):
    check(lib().tri_adam_step_segments_clipped(ptr(p), ptr(grad_ptrs), ptr(grad_starts), grad_starts.numel(), ptr(m), ptr(v), p.numel(),
                                               ptr(step), lr, ptr(lr_dev), b1, b2, eps, wd, gscale, ptr(coef_dev), clip_value, stream()),
          "tri_adam_step_segments_clipped")


# ------------------------------------------------------------------------------------------------ dynamic loss scaling (include/tricolo_hip.h)
def check_loss_scale(value, what) -> float:
    """A loss scale is a power of two in [2^-100, 2^100] (its reciprocal and its products with a coefficient are exact), as F16_GRAD_SCALE is."""
    s = float(value)
    if not (math.isfinite(s) and s > 0.0 and math.frexp(s)[0] == 0.5 and -99 <= math.frexp(s)[1] <= 101):
        raise ValueError(f"{what}={value!r}: must be a power of two in [2^-100, 2^100] (the kernels divide it out exactly)")
    return s


def loss_scale_step(state, cnt, step, partial, nblk, gscale, max_norm, growth_interval, min_scale, max_scale, rec, clipped):
    """One launch between adam_tick (and the sum-of-squares launches) and the *_clipped update.  With s = state[0], the scale the step's
    backward was seeded with: rec[0] = |gscale| / s * sqrt(sum(partial[:nblk])), rec[1] = c / s with grad_clip_coef's c (1 when nblk == 0),
    clipped[0] += 1 when c < 1; then the scale for the next backward: halved down to min_scale when the guard skipped this step, doubled up to
    max_scale after growth_interval applied steps in a row.  state: fp32 [2] = {s, 1 / s}, cnt: int32 [3] = {streak, backoffs, growths},
    step: adam_tick's int32 [4], rec: fp32 [2], clipped: int32 [1], all on the device; partial may be None with nblk == 0."""
    assert state.dtype == torch.float32 and state.numel() >= 2 and cnt.dtype == torch.int32 and cnt.numel() >= 3
    assert step.dtype == torch.int32 and step.numel() >= 4
    assert rec.dtype == torch.float32 and rec.numel() >= 2 and clipped.dtype == torch.int32 and clipped.numel() >= 1
    check(lib().tri_loss_scale_step(ptr(state), ptr(cnt), ptr(step), ptr(_partial(partial, nblk)) if nblk else None, nblk, gscale, max_norm,
                                    int(growth_interval), min_scale, max_scale, ptr(rec), ptr(clipped), stream()), "tri_loss_scale_step")


# ------------------------------------------------------------------------------------------------ counter-based dropout
DROPOUT_BITS = 24                                                   # uniform bits compared with p (csrc/dropout.hip)
_M32, _M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF


def dropout_threshold_scale(p):
    """p in [0, 1] -> (threshold, scale) of tri_dropout_apply: an element is dropped when its 24 uniform bits are below
    threshold = round(p * 2^24) (float64); a kept one is multiplied by scale = fp32(1 / (1 - p)), 0 at p = 1."""
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"dropout probability has to be between 0 and 1, but got {p}")
    scale = 0.0 if p == 1.0 else float(torch.tensor(1.0 / (1.0 - p), dtype=torch.float32).item())
    return int(p * 16777216.0 + 0.5), scale


def dropout_mask(rows, cols, p, seed, step, row0=0, tower=0):
    """The multiplier m of dropout_apply as a CPU fp32 [rows, cols] tensor (0 or scale), from Python ints: the torch restatement of
    csrc/dropout.hip on evaluation.mesh.philox4x32_10, the same bits."""
    from .evaluation.mesh import philox4x32_10
    threshold, scale = dropout_threshold_scale(p)
    rows, cols, seed = int(rows), int(cols), int(seed) & _M64
    groups = (cols + 3) // 4
    g = torch.arange(groups, dtype=torch.int64)[None, :].expand(rows, groups)
    r = (((int(row0) & _M32) + torch.arange(rows, dtype=torch.int64)) & _M32)[:, None].expand(rows, groups)
    zero = torch.zeros((rows, groups), dtype=torch.int64)
    words = philox4x32_10((g, r, zero + (int(step) & _M32), zero + (int(tower) & _M32)), (seed & _M32, seed >> 32))
    w = torch.stack(words, dim=-1).reshape(rows, groups * 4)[:, :cols]
    return torch.where((w >> 8) < threshold, 0.0, scale).to(torch.float32)


def dropout_tick(step):
    """used = step.clone(); step += 1, as one launch on the current stream (step, used: int64 [1] on step's device).  `used` is what
    dropout_apply reads, in this forward and in its backward; under HIP-graph replay both follow the counter."""
    if step.dtype != torch.int64 or step.numel() != 1:
        raise ValueError("dropout_tick: step must be an int64 tensor with one element")
    if not step.is_cuda:
        used = step.clone()
        step += 1
        return used
    used = torch.empty((1,), dtype=torch.int64, device=step.device)
    check(lib().tri_dropout_tick(ptr(step), ptr(used), stream()), "tri_dropout_tick")
    return used


def dropout_apply(x, p, seed, used, row0=0, tower=0):
    """y = x * m for fp32 x [rows, cols]: m(r, c) = 0 where the counter-based mask of (seed, used[0], tower, row0 + r, c) drops the
    element, fp32(1 / (1 - p)) elsewhere (head of csrc/dropout.hip; inf / NaN propagate through the multiply as in torch).  The same
    call serves the backward (dx = dy * m).  used: the int64 [1] tensor of dropout_tick.  row0: the global index of row 0 (a
    data-parallel rank passes rank * B_local and draws the rows of the global batch).  CPU tensors run the torch restatement
    dropout_mask: the same bits."""
    threshold, scale = dropout_threshold_scale(p)
    if x.dim() != 2 or x.dtype != torch.float32 or x.shape[1] < 1:
        raise ValueError(f"dropout_apply: x must be float32 [rows, cols >= 1], got {x.dtype} {tuple(x.shape)}")
    if used.dtype != torch.int64 or used.numel() != 1 or used.device != x.device:
        raise ValueError("dropout_apply: used must be the int64 [1] tensor of dropout_tick, on x's device")
    x = x.contiguous()
    rows, cols = x.shape
    if not x.is_cuda:
        return x * dropout_mask(rows, cols, p, seed, int(used.item()), row0, tower)
    y = torch.empty_like(x)
    check(lib().tri_dropout_apply(ptr(x), ptr(y), rows, cols, threshold, scale, int(seed) & _M64, ptr(used), int(row0) & _M64,
                                  int(tower) & _M32, stream()), "tri_dropout_apply")
    return y
