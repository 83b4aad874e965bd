"""Generate tests/golden/bn_bwd_traces.json: which launches the BatchNorm / pooling wrappers of tricolo_amd.ops make.  TEST INFRASTRUCTURE.

    python tools/make_bn_trace_golden.py            # record the traces of the tricolo_amd that comes first on the path

The wrappers of the sections "BatchNorm" and "pooling" decide on the host which entry points of the library a call becomes (DESIGN.md
section 5, "BatchNorm backward by caller").  Those decisions need neither a GPU nor the library: here the wrappers run on CPU tensors
with four names of tricolo_amd.ops replaced - `lib` (a recorder that answers every query with a fixed number and every launch with 0;
tri_conv_stem_wgrad_bn with a settable code), `ptr`, `stream`, `check` - and `conv_wgrad` / `_workspace` stubbed.  The file pins the
result over a sweep, so that a change to the routing shows as a changed cell.  It was recorded before the wrappers were rewritten
around one finisher.  It holds

    query_value     the number every query (*_num_blocks, *_scratch) answered
    launches        the distinct launches: [entry point, argument, ...]
    traces          the distinct traces: lists of indices into `launches`, or an exception's type name for a call that raised
    cases           per case of sweep(), in its order: index into `traces`
    cases_sha256    SHA-256 of the case ids of sweep(), one per line

A launch is an entry point declared with a stream (queries are dropped), or one of three pseudo entries: "conv_wgrad" (the stub: its
operands, scale and the batch's arena cursor), "return" (the tensors the wrapper handed back) and "batch" (the stub batch's cursor and
how many reduce descriptors / gradient tensors it collected).  Arguments: integers, floats and strings as they are, None as null, a
pointer as the name of the caller's operand it equals ("y", "co.mean", "rows[0]", ...) or else as "t<k>", numbered by first appearance
in the trace - so aliasing (dy in place of g, g_masked = g) and the order of the five finalize outputs are part of the trace,
addresses are not; anything else (a ctypes reference) as its type's name.  Every tensor whose pointer was taken stays alive until the
case ends: a recycled address cannot look like aliasing.

tests/test_bn_traces.py replays every case.  Re-record only when a launch sequence is MEANT to change, and say so in the commit.
"""
import contextlib
import hashlib
import itertools
import json
import os
import sys
import types

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.append(REPO)                        # (behind what is there: a parent worktree put first on the path is the one recorded)
OUT = os.path.join(REPO, "tests", "golden", "bn_bwd_traces.json")

QUERY_VALUE = 3
F32, F16 = torch.float32, torch.float16
UNSUPPORTED = -2                                 # TRI_ERR_UNSUPPORTED


def _stream_entry_points():
    from tests.guard_bands import stream_entry_points
    return stream_entry_points()


class Recorder:
    """Stands in for the library handle: notes (entry point, arguments) of every launch."""

    def __init__(self):
        self.calls, self.stem_rc, self._launch = [], 0, _stream_entry_points()

    def __getattr__(self, name):
        if name not in self._launch:
            return lambda *a: QUERY_VALUE

        def launch(*a):
            self.calls.append((name, a))
            return self.stem_rc if name == "tri_conv_stem_wgrad_bn" else 0
        return launch


class Batch:
    """What maxpool_bn_bwd_wgrad uses of ops.WgradBatch."""

    def __init__(self):
        self.ci, self.off, self.descs, self.dws = 0, 0, [], {}

    def slab(self, nbytes):
        self.off += nbytes
        return torch.empty(nbytes, dtype=torch.uint8)


@contextlib.contextmanager
def traced(ops, world=1, stem_rc=0, **flags):
    """Patch tricolo_amd.ops as the module docstring says (flags: module flags such as _BN_SMALL=False); yields the Recorder, whose
    `keep` list holds every tensor whose pointer was taken."""
    rec = Recorder()
    rec.stem_rc, rec.keep = stem_rc, []

    def ptr(t):
        if t is None:
            return None
        rec.keep.append(t)
        return ("ptr", t.data_ptr())

    def conv_wgrad(x, dout, g, like, precision, row_mask=None, out_scale=1.0, batch=None, rows=None):
        dw = torch.empty_like(like)
        rec.calls.append(("conv_wgrad", (ptr(x), ptr(dout), ptr(like), precision, ptr(row_mask), float(out_scale), rows,
                                         None if batch is None else batch.ci, None if batch is None else batch.off, ptr(dw))))
        return dw

    new = dict(lib=lambda: rec, ptr=ptr, stream=lambda: 0, check=lambda rc, what="": None, conv_wgrad=conv_wgrad,
               _workspace=lambda nbytes, device: torch.empty(nbytes, dtype=torch.uint8), _sync_world=lambda: world, _sync_sum=lambda t: t, **flags)
    old = {k: getattr(ops, k) for k in new}
    for k, v in new.items():
        setattr(ops, k, v)
    try:
        yield rec
    finally:
        for k, v in old.items():
            setattr(ops, k, v)


def canonical(calls, operands):
    """The trace of recorded calls (module docstring).  operands: name -> tensor of the caller's own operands."""
    names = {}
    for n, t in operands.items():
        names.setdefault(t.data_ptr(), n)

    fresh = {}

    def token(a):
        if a is None or isinstance(a, (int, float, str)):
            return a
        if isinstance(a, tuple) and len(a) == 2 and a[0] == "ptr":
            return names[a[1]] if a[1] in names else fresh.setdefault(a[1], f"t{len(fresh)}")
        return type(a).__name__
    return [[name] + [token(a) for a in args] for name, args in calls]


# ------------------------------------------------------------------------------------------------ operands
def _coeffs(ops, C, tag="co"):
    co = ops.BNCoeffs(C, "cpu")
    return co, {f"{tag}.{k}": getattr(co, k) for k in ("mean", "invstd", "scale", "shift")}


def _rows(n, tag):
    r = (torch.empty(n, dtype=torch.int32), torch.empty(1, dtype=torch.int32))
    return r, {f"{tag}[0]": r[0], f"{tag}[1]": r[1]}


def _geom(N, H, W, C):
    from tricolo_amd import _C
    OH, OW = H, W
    return types.SimpleNamespace(desc=_C.make_desc(N, 1, 2 * OH, 2 * OW, 4, 1, OH, OW, C, 1, 7, 7, 2, 0, 3, 3), strides=(147, 1, 49), kernel=(1, 7, 7),
                                 flops=1, wgrad_ws=4096, cin=3, M=N * OH * OW)


def _finish(rec, out, operands, batch=None):
    """Append the pseudo entries "return" and "batch", -> the canonical trace."""
    outs = out if isinstance(out, tuple) else (out,)
    rec.calls.append(("return", tuple(None if t is None else ("ptr", t.data_ptr()) for t in outs)))
    if batch is not None:
        rec.calls.append(("batch", (batch.ci, batch.off, len(batch.descs), len(batch.dws))))
    return canonical(rec.calls, operands)


# ------------------------------------------------------------------------------------------------ the wrappers, one runner each
def run_bn_bwd(ops, M, C, mask, mode, partial, inplace, keep, small, world):
    y, g, gamma = torch.empty(M, C), torch.empty(M, C), torch.empty(C)
    co, names = _coeffs(ops, C)
    names.update(y=y, g=g, gamma=gamma)
    kw = {}
    if mask:
        kw["row_mask"], kw["count_dev"] = torch.empty((M + 31) // 32 * 32, dtype=torch.uint8), torch.ones(1, dtype=torch.int32)
    else:
        kw["count_host"] = M
    if mode == "relu":
        kw["relu"] = True
    elif mode == "relu_out":
        kw["relu_out"], kw["g_masked"] = torch.empty(M, C), g
    if partial:
        kw["partial"] = torch.zeros(5, 2, C)
    names.update({k: v for k, v in kw.items() if isinstance(v, torch.Tensor) and k != "g_masked"})
    with traced(ops, world=world, _BN_SMALL=small) as rec:
        out = ops.bn_bwd(y, g, co, gamma, inplace=inplace, out_scale=0.25, keep_inactive=keep, **kw)
        return _finish(rec, out, names)


def run_pool3d_bn_bwd(ops, B, D, C, dtype, fused, keep, rows, rows_out, vox_rows, route_red, world):
    Do = D // 2
    y, pooled, dpooled = (torch.empty(B, D, D, D, C, dtype=dtype), torch.empty(B, Do, Do, Do, C, dtype=dtype), torch.empty(B, Do, Do, Do, C, dtype=dtype))
    mask, gamma, count = torch.empty((B * D ** 3 + 31) // 32 * 32, dtype=torch.uint8), torch.empty(C), torch.ones(1, dtype=torch.int32)
    co, names = _coeffs(ops, C)
    names.update(y=y, pooled=pooled, dpooled=dpooled, mask=mask, gamma=gamma, count_dev=count)
    r = ro = None
    if rows:
        r, n = _rows(B * D ** 3, "rows")
        names.update(n)
    if rows_out:
        ro, n = _rows(B * Do ** 3, "rows_out")
        names.update(n)
    with traced(ops, world=world, _VOX_ROWS=vox_rows, _ROUTE_RED=route_red) as rec:
        out = ops.pool3d_bn_bwd(y, co, mask, pooled, dpooled, B, D, C, gamma, count, out_scale=0.25, fused=fused, keep_inactive=keep, rows=r, rows_out=ro)
        return _finish(rec, out, names)


def _stem_operands(ops, N, H, W, C, dtype, with_pooled):
    Hp, Wp = (H + 1) // 2, (W + 1) // 2
    y, arg = torch.empty(N, 1, H, W, C, dtype=dtype), torch.empty(N, 1, Hp, Wp, C, dtype=torch.uint8)
    dpool, pooled, gamma = torch.empty(N, 1, Hp, Wp, C, dtype=dtype), torch.empty(N, 1, Hp, Wp, C, dtype=dtype), torch.empty(C)
    co, names = _coeffs(ops, C)
    names.update(y=y, arg=arg, dpool=dpool, gamma=gamma)
    if with_pooled:
        names["pooled"] = pooled
    return y, arg, dpool, pooled if with_pooled else None, gamma, co, names


def run_maxpool_bn_bwd(ops, dtype, C, with_pooled, stem_pooled, world):
    y, arg, dpool, pooled, gamma, co, names = _stem_operands(ops, 2, 16, 16, C, dtype, with_pooled)
    with traced(ops, world=world, _STEM_POOLED=stem_pooled) as rec:
        out = ops.maxpool_bn_bwd(y, arg, dpool, co, gamma, out_scale=0.25, pooled=pooled)
        return _finish(rec, out, names)


def run_maxpool_bn_bwd_wgrad(ops, H, W, dtype, C, with_pooled, with_batch, stem_rc, world):
    N = 2
    y, arg, dpool, pooled, gamma, co, names = _stem_operands(ops, N, H, W, C, dtype, with_pooled)
    x0, like = torch.empty(N, 1, 2 * H, 2 * W, 4, dtype=dtype), torch.empty(C, 3, 7, 7)
    names.update(x0=x0, like=like)
    batch = Batch() if with_batch else None
    with traced(ops, world=world, stem_rc=stem_rc) as rec:
        out = ops.maxpool_bn_bwd_wgrad(x0, y, arg, dpool, co, gamma, _geom(N, H, W, C), like, "f16" if dtype == F16 else "bf16x3", out_scale=0.25,
                                       batch=batch, pooled=pooled)
        return _finish(rec, out, names, batch)


def stem_composition(ops, H, W, dtype, C, with_batch):
    """What maxpool_bn_bwd_wgrad has to launch on a map with an odd side: the max-pool backward, the BatchNorm backward that recomputes the
    ReLU mask, the weight gradient.  Operands and names as run_maxpool_bn_bwd_wgrad's."""
    N = 2
    y, arg, dpool, _, gamma, co, names = _stem_operands(ops, N, H, W, C, dtype, False)
    x0, like = torch.empty(N, 1, 2 * H, 2 * W, 4, dtype=dtype), torch.empty(C, 3, 7, 7)
    names.update(x0=x0, like=like)
    batch = Batch() if with_batch else None
    g = _geom(N, H, W, C)
    with traced(ops) as rec:
        dz = ops.maxpool2d_bwd(arg, dpool, tuple(y.shape))
        dy, dgamma, dbeta = ops.bn_bwd(y, dz, co, gamma, count_host=g.M, relu=True, out_scale=0.25)
        dw = ops.conv_wgrad(x0, dy, g, like, "f16" if dtype == F16 else "bf16x3", out_scale=0.25, batch=batch)
        return _finish(rec, (dw, dgamma, dbeta), names, batch)


def run_single(ops, which):
    """One case each of the wrappers that launch one kernel (family)."""
    M, C, B, D = 640, 64, 2, 4
    y, g, gamma, beta = torch.empty(M, C), torch.empty(M, C), torch.empty(C), torch.empty(C)
    co, names = _coeffs(ops, C)
    names.update(y=y, g=g, gamma=gamma)
    with traced(ops) as rec:
        if which == "bn_bwd_pair":
            yb, out, cob = torch.empty(M, C), torch.empty(M, C), _coeffs(ops, C, "cob")
            names.update(cob[1], yb=yb, relu_out=out, gamma_b=beta)
            r = ops.bn_bwd_pair(y, co, gamma, yb, cob[0], beta, g, out, M, g_masked=g, out_scale=0.25)
        elif which == "bn_bwd_rows":
            rows, n = _rows(M, "rows")
            names.update(n)
            r = ops.bn_bwd_rows(y, g, co, gamma, rows, out_scale=0.25)
        elif which == "bn_act":
            res, res_co = torch.empty(M, C), _coeffs(ops, C, "res_co")
            names.update(res_co[1], res=res)
            r = ops.bn_act(y, co, relu=True, res=res, res_co=res_co[0])
        elif which == "relu_bwd":
            names["out"] = out = torch.empty(M, C)
            r = ops.relu_bwd(g, out, inplace=True)
        elif which == "bn_finalize":
            stats, rm, rv, nbt = torch.empty(5, 2, C), torch.empty(C), torch.empty(C), torch.zeros((), dtype=torch.long)
            names.update(stats=stats, beta=beta, running_mean=rm, running_var=rv, nbt=nbt)
            names.update(_coeffs_names(ops.bn_finalize(stats, C, gamma, beta, rm, rv, nbt, count_host=M)))
            r = None
        elif which == "bn_eval_coeffs":
            rm, rv = torch.empty(C), torch.empty(C)
            names.update(beta=beta, running_mean=rm, running_var=rv)
            names.update(_coeffs_names(ops.bn_eval_coeffs(C, gamma, beta, rm, rv)))
            r = None
        elif which in ("bn_relu_pool3d_fwd", "pool3d_bwd_route", "pool3d_bwd_route_rows"):
            y5, mask = torch.empty(B, D, D, D, C), torch.empty(B * D ** 3, dtype=torch.uint8)
            pooled, dpooled = torch.empty(B, 2, 2, 2, C), torch.empty(B, 2, 2, 2, C)
            names.update(y=y5, mask=mask, pooled=pooled, dpooled=dpooled)
            if which == "bn_relu_pool3d_fwd":
                r = ops.bn_relu_pool3d_fwd(y5, co, mask, B, D, C)
            elif which == "pool3d_bwd_route":
                r = ops.pool3d_bwd_route(y5, co, mask, pooled, dpooled, B, D, C)
            else:
                rows_out, n = _rows(B * 8, "rows_out")
                names.update(n)
                r = ops.pool3d_bwd_route_rows(y5, co, mask, pooled, dpooled, B, D, C, rows_out)
        elif which in ("maxpool2d_fwd", "maxpool2d_fwd_bn", "maxpool2d_bwd"):
            x, arg, dout = torch.empty(2, 1, 15, 16, C), torch.empty(2, 1, 8, 8, C, dtype=torch.uint8), torch.empty(2, 1, 8, 8, C)
            names.update(x=x, arg=arg, dout=dout)
            if which == "maxpool2d_bwd":
                r = ops.maxpool2d_bwd(arg, dout, tuple(x.shape))
            else:
                r = ops.maxpool2d_fwd(x, bn=co if which.endswith("_bn") else None)
        elif which == "bn_bwd_mixed_storage":                      # refused: y and g in different storage types
            r = ops.bn_bwd(y, g.to(F16), co, gamma, count_host=M)
        elif which == "maxpool_bn_bwd_wgrad_mixed_storage":        # refused likewise, whatever the geometry
            y5, arg, dpool = torch.empty(2, 1, 16, 16, C, dtype=F16), torch.empty(2, 1, 8, 8, C, dtype=torch.uint8), torch.empty(2, 1, 8, 8, C)
            r = ops.maxpool_bn_bwd_wgrad(torch.empty(2, 1, 32, 32, 4, dtype=F16), y5, arg, dpool, co, gamma, _geom(2, 16, 16, C), torch.empty(C, 3, 7, 7), "f16")
        else:
            raise KeyError(which)
        return _finish(rec, r, names)


def _coeffs_names(co):
    """The coefficients a wrapper RETURNED, named like an operand so that the order of the four outputs shows."""
    return {f"out.{k}": getattr(co, k) for k in ("mean", "invstd", "scale", "shift")}


SINGLES = ("bn_bwd_pair", "bn_bwd_rows", "bn_act", "relu_bwd", "bn_finalize", "bn_eval_coeffs", "bn_relu_pool3d_fwd", "pool3d_bwd_route",
           "pool3d_bwd_route_rows", "maxpool2d_fwd", "maxpool2d_fwd_bn", "maxpool2d_bwd", "bn_bwd_mixed_storage", "maxpool_bn_bwd_wgrad_mixed_storage")
POOL3D_SHAPES = ((1, 2, 64), (1, 4, 64), (2, 16, 32), (5, 16, 32), (5, 16, 6), (5, 16, 24), (5, 16, 2048))
# (_VOX_ROWS, _ROUTE_RED, world) settings of the pool3d sweep and (_BN_SMALL, world) of the bn_bwd sweep
POOL3D_SETTINGS = ((True, True, 1), (False, True, 1), (True, False, 1), (True, True, 2))
BN_BWD_SETTINGS = ((True, 1), (False, 1), (True, 2))


def sweep():
    """[(case id, runner, arguments)] in the recorded order.  bn_bwd with ready-made sums AND a row mask is left out: the call was refused
    when the file was recorded and is legal since (pool3d_bn_bwd's sums with the site mask; tests/test_bn_traces.py checks it live)."""
    bits = (False, True)
    cases = []
    for (small, world), M, C, mask, mode, partial, inplace, keep in itertools.product(BN_BWD_SETTINGS, (256, 512, 513, 20000), (32, 64, 96), bits,
                                                                                      ("final", "relu", "relu_out"), bits, bits, bits):
        if (partial and mask) or (keep and not mask):
            continue
        cases.append((f"bn_bwd M{M} C{C} mask{mask:d} {mode} partial{partial:d} inplace{inplace:d} keep{keep:d} small{small:d} world{world}",
                      run_bn_bwd, (M, C, mask, mode, partial, inplace, keep, small, world)))
    for (vox_rows, route_red, world), (B, D, C), dtype, fused, keep, rows, rows_out in itertools.product(POOL3D_SETTINGS, POOL3D_SHAPES, (F32, F16),
                                                                                                       bits, bits, bits, bits):
        cases.append((f"pool3d_bn_bwd {B}x{D}x{C} {'f16' if dtype == F16 else 'fp32'} fused{fused:d} keep{keep:d} rows{rows:d} rows_out{rows_out:d} "
                      f"vox_rows{vox_rows:d} route_red{route_red:d} world{world}",
                      run_pool3d_bn_bwd, (B, D, C, dtype, fused, keep, rows, rows_out, vox_rows, route_red, world)))
    for dtype, C, with_pooled, stem_pooled, world in itertools.product((F32, F16), (64, 24), bits, bits, (1, 2)):
        cases.append((f"maxpool_bn_bwd {'f16' if dtype == F16 else 'fp32'} C{C} pooled{with_pooled:d} stem_pooled{stem_pooled:d} world{world}",
                      run_maxpool_bn_bwd, (dtype, C, with_pooled, stem_pooled, world)))
    for dtype, C, with_pooled, with_batch, rc, world in itertools.product((F32, F16), (64, 32), bits, bits, (0, UNSUPPORTED), (1, 2)):
        cases.append((f"maxpool_bn_bwd_wgrad 16x16 {'f16' if dtype == F16 else 'fp32'} C{C} pooled{with_pooled:d} batch{with_batch:d} rc{rc} world{world}",
                      run_maxpool_bn_bwd_wgrad, (16, 16, dtype, C, with_pooled, with_batch, rc, world)))
    cases += [(name, run_single, (name,)) for name in SINGLES]
    return cases


def run_case(ops, runner, args):
    """The canonical trace of one case, or the type name of what it raised."""
    try:
        return runner(ops, *args)
    except Exception as e:               # noqa: BLE001 - a refused call is a result
        return type(e).__name__


def cases_sha256(cases):
    return hashlib.sha256("\n".join(c[0] for c in cases).encode()).hexdigest()


def expand(rec, index):
    """Trace number `index` of a loaded file, launches written out."""
    t = rec["traces"][index]
    return t if isinstance(t, str) else [rec["launches"][i] for i in t]


def main():
    from tricolo_amd import ops
    cases = sweep()
    launches, traces, lidx, tidx, per_case = [], [], {}, {}, []
    for _, runner, args in cases:
        tr = run_case(ops, runner, args)
        if not isinstance(tr, str):
            tr = [lidx.setdefault(json.dumps(l), len(lidx)) for l in tr]
        per_case.append(tidx.setdefault(json.dumps(tr), len(tidx)))
    launches = [json.loads(k) for k in lidx]
    traces = [json.loads(k) for k in tidx]
    with open(OUT, "w") as f:
        json.dump(dict(query_value=QUERY_VALUE, launches=launches, traces=traces, cases=per_case, cases_sha256=cases_sha256(cases)), f,
                  separators=(",", ":"))
        f.write("\n")
    reached = sorted({l[0] for l in launches})
    print(f"{len(cases)} cases, {len(traces)} traces, {len(launches)} launches from {os.path.dirname(ops.__file__)} -> {OUT} "
          f"({os.path.getsize(OUT)} bytes); entry points: {', '.join(reached)}")


if __name__ == "__main__":
    main()
