"""Self-tests of tests/guard_bands.py on host tensors (the proxy and banded() run with a device argument of "cpu"), and the planner's
word on which kernel families the guarded conv cases of tests/test_gpu_guard_bands.py reach.  No GPU needed."""
import pytest
import torch

from tests import guard_bands as gb
from tests.guard_bands import BAND, POISON, ZERO
from tricolo_amd import ops


def _parent(view):
    return view._band.parent


@pytest.mark.parametrize("shape,dtype", [((5, 7), torch.float32), ((3, 1, 9), torch.bfloat16), ((), torch.float32), ((33,), torch.uint8),
                                         ((4097,), torch.float16)])
def test_view_offset_size_and_contents(shape, dtype):
    t = (torch.arange(max(1, int(torch.tensor(shape).prod())) if shape else 1) % 7).to(dtype).reshape(shape)
    v = gb.banded(t, POISON)
    b = v._band
    nbytes = t.numel() * t.element_size()
    assert v.shape == t.shape and v.dtype == t.dtype and v.is_contiguous() and torch.equal(v, t)
    assert b.nbytes == nbytes and b.parent.numel() == 2 * BAND + nbytes and b.parent.dtype == torch.uint8
    assert v.data_ptr() - b.parent.data_ptr() == BAND and BAND % gb.ALIGN == 0 and BAND >= 2 * 256 * 512 * 4
    assert v.untyped_storage().data_ptr() == b.parent.untyped_storage().data_ptr()          # one allocation
    assert bool((b.parent[:BAND] == POISON).all()) and bool((b.parent[BAND + nbytes:] == POISON).all())
    assert b.damage() == []


def test_poison_is_nan_in_the_three_float_types_and_active_in_a_mask():
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        v = gb.banded(torch.zeros(8, dtype=dtype), POISON)
        band = _parent(v)[:BAND].view(dtype)
        assert bool(torch.isnan(band).all()), dtype
        assert bool((_parent(gb.banded(torch.zeros(8, dtype=dtype), ZERO))[:BAND].view(dtype) == 0).all())
    m = gb.banded(torch.zeros(32, dtype=torch.uint8), POISON)
    assert bool((_parent(m)[:BAND] != 0).all())


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_index_tensors_get_zero_bands(dtype):
    v = gb.banded(torch.arange(10, dtype=dtype), POISON)
    assert v._band.fill == ZERO and bool((_parent(v) [:BAND] == 0).all()) and bool((_parent(v)[BAND + v._band.nbytes:] == 0).all())
    with gb.guarded_ops(POISON, device="cpu", device_types=("cpu",), record=False) as g:
        t = ops.torch.empty((6,), dtype=dtype, device="cpu")
        assert t._band.fill == ZERO and bool((t == 0).all())          # the unwritten interior of an index tensor is zeros too
        f = ops.torch.empty((6,), dtype=torch.float32, device="cpu")
        assert f._band.fill == POISON and bool(torch.isnan(f).all())


def _stray_write(view, where):
    """A fake kernel: writes one element just outside the view, through the parent buffer."""
    p, es = view._band.parent, view.element_size()
    at = BAND - es if where == "before" else BAND + view._band.nbytes
    p[at:at + es] = 0x3C


@pytest.mark.parametrize("where", ["before", "after"])
@pytest.mark.parametrize("fill", [POISON, ZERO])
def test_a_stray_write_is_caught_on_either_side_with_its_offset(where, fill):
    x = torch.randn(19, 64)
    with pytest.raises(gb.GuardBandError) as e:
        with gb.guarded_ops(fill, device="cpu", device_types=("cpu",), record=False) as g:
            v = g.put(x.to(torch.bfloat16))
            out = ops.torch.empty_like(v)
            out.copy_(v)
            _stray_write(out, where)
    (r,) = e.value.records
    assert r["side"] == where and r["shape"] == (19, 64) and r["dtype"] == torch.bfloat16 and r["origin"] == "ops torch.empty_like"
    assert r["offset"] == (-2 if where == "before" else 19 * 64 * 2)
    assert "byte offset" in str(e.value) and "bfloat16" in str(e.value)


def test_a_stray_write_into_a_registered_operand_is_caught_and_a_clean_run_passes():
    with gb.guarded_ops(POISON, device="cpu", device_types=("cpu",), record=False) as g:
        v = g.put(torch.ones(3, 5))
        w = ops.torch.zeros((3, 5), dtype=torch.float32, device="cpu")
        w.add_(v)                                                   # a clean "kernel"
    assert torch.equal(w, torch.ones(3, 5)) and len(g.ledger) == 2
    with pytest.raises(gb.GuardBandError) as e:
        with gb.guarded_ops(POISON, device="cpu", device_types=("cpu",), record=False) as g:
            v = g.put(torch.ones(3, 5))
            _parent(v)[BAND + 60 + 7] = 1                           # 7 bytes past the end of the operand
    assert [(r["side"], r["offset"], r["origin"]) for r in e.value.records] == [("after", 67, "input")]


def test_a_zero_write_next_to_an_index_tensor_is_the_documented_blind_spot():
    with gb.guarded_ops(POISON, device="cpu", device_types=("cpu",), record=False) as g:
        v = g.put(torch.arange(4, dtype=torch.int32))
        _parent(v)[BAND - 4:BAND] = 0                               # a stray write of a zero: not seen (module docstring)
    with pytest.raises(gb.GuardBandError):
        with gb.guarded_ops(POISON, device="cpu", device_types=("cpu",), record=False) as g:
            v = g.put(torch.arange(4, dtype=torch.int32))
            _parent(v)[BAND - 4] = 9


def test_allocator_semantics_and_tags_survive_the_proxy():
    with gb.guarded_ops(POISON, device="cpu", device_types=("cpu",), record=False) as g:
        px = ops.torch
        assert px.float16 is torch.float16 and px.nn is torch.nn and px.cuda is torch.cuda       # everything else is the real module's
        a = px.empty((4, 6), dtype=torch.float16, device="cpu")
        a.tri_frag = 1
        b = px.empty_like(a)
        assert b.shape == (4, 6) and b.dtype == torch.float16 and b.is_contiguous() and a.tri_frag == 1 and not hasattr(b, "tri_frag")
        assert px.empty_like(a, dtype=torch.float32).dtype == torch.float32
        z = px.zeros((2, 3), dtype=torch.float32, device="cpu")
        assert bool((z == 0).all()) and bool((px.zeros_like(a) == 0).all())
        assert px.zeros(5, device="cpu").shape == (5,) and px.empty(2, 3, device="cpu").shape == (2, 3)
        f = px.full((7,), 2.5, dtype=torch.float32, device="cpu")
        assert bool((f == 2.5).all()) and px.full((3,), 4, device="cpu").dtype == torch.int64
        s = px.empty((), dtype=torch.float32, device="cpu")
        assert s.shape == () and s.numel() == 1
        host = px.empty((3,), dtype=torch.float32)                   # no device: a host allocation passes through
        assert not hasattr(host, "_band")
        assert not hasattr(px.empty((3,), dtype=torch.float32, device="meta"), "_band")
        n = len(g.ledger)
        ws = ops._workspace(1000, "cpu")                            # exactly the bytes asked for, not max(nbytes, 1 MiB)
        assert ws.numel() == 1000 and ws.dtype == torch.uint8 and len(g.ledger) == n + 1
        batch = ops.WgradBatch.__new__(ops.WgradBatch)
        batch.device = torch.device("cpu")
        assert batch.slab(1000).numel() == 1024 and batch.slab(256).numel() == 256            # the slab's own rounding to 256 is kept
        # a packed operand's tag, set by ops itself on a tensor the proxy made
        pair = (px.empty((8, 64), dtype=torch.bfloat16, device="cpu"), None)
        pair[0].tri_frag = 1
        assert getattr(pair[0], "tri_frag", 0) == 1


def test_ops_is_itself_again_after_an_exception():
    real_ws, real_slab = ops._workspace, ops.WgradBatch.slab
    ops._wgrad_ws["stale"] = torch.empty(1)
    with pytest.raises(KeyError):
        with gb.guarded_ops(POISON, device="cpu", device_types=("cpu",), record=False):
            assert ops.torch is not torch and "stale" not in ops._wgrad_ws
            raise KeyError("inside")
    assert ops.torch is torch and ops._workspace is real_ws and ops.WgradBatch.slab is real_slab
    assert ops._wgrad_ws == {} and ops.WgradBatch._arenas == {}


def test_recording_wrapper_notes_entry_points_and_restores_the_handle():
    from tricolo_amd import _C
    real = _C.lib()
    with gb.recording() as rec:
        assert _C.lib() is rec
        ops.lib().tri_conv_kpad(27, 32)
        ops.lib().tri_version()
        assert rec.calls == ["tri_conv_kpad"] and rec.launches() == []        # a size query is noted but is no launch
    assert _C.lib() is real
    assert gb.RecordingLib.is_query("tri_bn_bwd_rows_scratch") and not gb.RecordingLib.is_query("tri_bn_bwd_rows")
    # launches are told from queries by the header's `void* stream` parameter, not by their names
    launches = gb.stream_entry_points()
    assert launches <= set(_C.SIGNATURES) and len(launches) > 80
    assert {"tri_conv_fwd", "tri_conv_wgrad_partial_group", "tri_wgrad_reduce_grouped", "tri_adam_tick", "tri_conv_plan_build"} <= launches
    assert not launches & {"tri_conv_wgrad_group_info", "tri_conv_plan_bytes", "tri_conv_num_records", "tri_mask_compact_multi_scratch",
                           "tri_linear_small_supported", "tri_version", "tri_last_error"}
    assert all(_C.SIGNATURES[n][1][-1] is _C.P and _C.SIGNATURES[n][0] is _C.I for n in launches)
    with pytest.raises(ZeroDivisionError):
        with gb.recording():
            1 / 0
    assert _C.lib() is real


def test_same_bytes_compares_bits():
    nan = torch.full((4,), float("nan"))
    assert gb.same_bytes(nan, nan.clone()) and not torch.equal(nan, nan.clone())
    assert not gb.same_bytes(torch.zeros(2), -torch.zeros(2)) and not gb.same_bytes(torch.zeros(2), torch.zeros(3))


# ------------------------------------------------------------------------------------------------ the conv case table, by the planner
def test_conv_case_table_reaches_every_family():
    """The planner answers without a GPU (256 compute units assumed).  tests/test_conv_plan.py records which family codes exist on the
    default switch set: forward {0, 2, 3, 4, 5, 6, 9, 12, 13, 14, 15} (14 on 16^3 grids), data gradient {0, 2, 3, 5, 9, 10, 12, 13} (10 is
    a data-gradient family: the forward never plans it)."""
    import os
    if any(k.startswith("TRICOLO_") and k != "TRICOLO_HELDOUT_STEPS" for k in os.environ):
        pytest.skip("a TRICOLO_* variable is set: the case table is the default switch set's")
    if torch.cuda.is_available() and torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip("the plans are those of 256 compute units")
    from tests import test_gpu_guard_bands as T
    from tests.test_conv_plan import GROUP_FAMILIES, WGRAD_FAMILIES
    fwd, dgrad, halo_tiles, splitk, partial = set(), set(), set(), 0, set()
    for cc, store, prec in T.CONV_RUNS:
        g = T.geom_of(cc.case)
        mode = T.plan_mode(store, prec)
        for tr in (False, True):
            if ("dgrad" if tr else "fwd") not in cc.dirs:
                continue
            code = g.kernel_family[(tr, mode)]
            fam = code & 255
            (dgrad if tr else fwd).add(fam)
            if fam in (3, 5):
                halo_tiles.add((code >> 8) & 255)
            # a row list or a row mask takes a split-K layer off the split-K plan: count the dense calls only
            splitk += int(g.splitk(tr, mode) and cc.form == "dense")
            if T.partial_last_tile(g, tr, code):
                partial.add(fam)
    assert fwd >= {0, 2, 3, 4, 5, 6, 9, 12, 13, 14, 15}, fwd
    assert dgrad >= {0, 2, 3, 5, 9, 10, 12, 13}, dgrad
    assert fwd | dgrad >= {0, 2, 3, 4, 5, 6, 9, 10, 12, 13, 14, 15}
    assert halo_tiles == {2, 3} and splitk >= 1
    assert partial >= T.FAMILIES_WITH_PARTIAL_TILES, T.FAMILIES_WITH_PARTIAL_TILES - partial
    wfam, gfam = set(), set()
    for case, store in T.wgrad_geometries():
        g = T.geom_of(case)
        fmt = ops._FMT[store]
        wfam.add(ops.lib().tri_conv_wgrad_kernel_family(ops._C.C.byref(g.desc), 1 if fmt else 0))
        gfam.add(g.wgrad_group(fmt)[0])
    assert wfam >= WGRAD_FAMILIES, (wfam, WGRAD_FAMILIES)
    assert gfam >= GROUP_FAMILIES, (gfam, GROUP_FAMILIES)
