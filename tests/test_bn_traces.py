"""Which launches the BatchNorm / pooling wrappers of tricolo_amd.ops make, pinned on the CPU (tests/golden/bn_bwd_traces.json,
tools/make_bn_trace_golden.py: how a trace is taken without a GPU or the library, and what it holds).

The file was recorded before ops.bn_bwd, ops.pool3d_bn_bwd and the stem wrappers were rewritten around one finisher (DESIGN.md section 5,
"BatchNorm backward by caller"): every case must still make the same launches with the same arguments, aliasing included.  Two calls
were refused when the file was recorded and have no recorded trace; they are checked against their composition, taken live:
ops.maxpool_bn_bwd_wgrad on a map with an odd side, and ops.bn_bwd with ready-made sums and a row mask."""
import importlib.util
import json
import os

import pytest

from tests.guard_bands import stream_entry_points

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "bn_bwd_traces.json")

_spec = importlib.util.spec_from_file_location("make_bn_trace_golden", os.path.join(REPO, "tools", "make_bn_trace_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

PSEUDO = ("conv_wgrad", "return", "batch")
# the launch sequences of ops.pool3d_bn_bwd that tests/test_gpu_bn_family.py::test_voxel_level_forward_and_backward asserts by count, and
# the one no level of the voxel tower takes (own row list, none of the pooled level)
POOL3D_SEQUENCES = {
    ("tri_pool3d_bwd_route_rows_reduce", "tri_bn_bwd_finalize", "tri_bn_bwd_apply_rows"),
    ("tri_pool3d_bwd_route_rows_reduce", "tri_bn_bwd_finalize", "tri_bn_bwd_apply"),
    ("tri_pool3d_bwd_route_rows", "tri_bn_bwd_rows"),
    ("tri_pool3d_bwd_route_rows", "tri_bn_bwd_reduce", "tri_bn_bwd_finalize", "tri_bn_bwd_apply"),
    ("tri_pool3d_bwd_route_reduce", "tri_bn_bwd_finalize", "tri_bn_bwd_apply"),
    ("tri_pool3d_bwd_route", "tri_bn_bwd_small"),
    ("tri_pool3d_bwd_route", "tri_bn_bwd_reduce", "tri_bn_bwd_finalize", "tri_bn_bwd_apply"),
    ("tri_pool3d_bwd_route", "tri_bn_bwd_rows"),
}


@pytest.fixture(scope="module")
def rec():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ops():
    from tricolo_amd import ops
    return ops


def test_every_case_reproduces_its_recorded_trace(rec, ops):
    cases = gen.sweep()
    assert rec["query_value"] == gen.QUERY_VALUE and rec["cases_sha256"] == gen.cases_sha256(cases) and len(rec["cases"]) == len(cases)
    bad = []
    for (cid, runner, args), index in zip(cases, rec["cases"]):
        got, want = gen.run_case(ops, runner, args), gen.expand(rec, index)
        if got != want:
            bad.append((cid, got, want))
    assert not bad, f"{len(bad)} of {len(cases)} cases changed their launches; the first:\n  {bad[0][0]}\n  now      {bad[0][1]}\n  recorded {bad[0][2]}"


def test_recorded_traces_reach_every_entry_point(rec):
    """A trimmed sweep cannot pass by leaving an entry point, a launch sequence or the refused calls out."""
    from tricolo_amd import _C
    assert os.path.getsize(GOLDEN) < 128 * 1024
    want = {n for n in _C.SIGNATURES if n in stream_entry_points() and n.startswith(("tri_bn_", "tri_pool3d_", "tri_maxpool", "tri_relu_bwd"))}
    want.add("tri_conv_stem_wgrad_bn")
    assert len(want) == 24
    reached = {l[0] for l in rec["launches"]}
    assert want <= reached, sorted(want - reached)
    assert reached - set(PSEUDO) <= stream_entry_points()                     # queries are not part of a trace
    pool3d = {tuple(l[0] for l in gen.expand(rec, i) if l[0] not in PSEUDO)
              for (cid, _, _), i in zip(gen.sweep(), rec["cases"]) if cid.startswith("pool3d_bn_bwd") and cid.endswith("world1")}
    assert pool3d == POOL3D_SEQUENCES
    assert "AssertionError" in rec["traces"]


@pytest.mark.parametrize("with_batch", [False, True], ids=["alone", "batch"])
@pytest.mark.parametrize("store", ["fp32", "f16"])
@pytest.mark.parametrize("H,W", [(15, 15), (15, 16), (16, 15)])
def test_stem_on_an_odd_map_is_the_three_call_composition(ops, H, W, store, with_batch):
    """ops.maxpool_bn_bwd_wgrad where H or W is odd: ops.maxpool2d_bwd, then ops.bn_bwd(relu=True, count_host=g.M), then ops.conv_wgrad,
    whatever else is passed (the forward's pooled tensor, a refusing stem kernel)."""
    dtype = gen.F16 if store == "f16" else gen.F32
    want = gen.stem_composition(ops, H, W, dtype, 64, with_batch)
    assert [l[0] for l in want][:3] == ["tri_maxpool2d_bwd", "tri_bn_bwd_small", "conv_wgrad"]       # (2 x 15 x 15 rows: the one-launch form)
    for with_pooled, rc in ((False, 0), (True, gen.UNSUPPORTED)):
        assert gen.run_maxpool_bn_bwd_wgrad(ops, H, W, dtype, 64, with_pooled, with_batch, rc, 1) == want


@pytest.mark.parametrize("keep", [False, True], ids=["zeroed", "keep_inactive"])
def test_bn_bwd_takes_given_sums_with_a_row_mask(ops, keep):
    """Ready-made sums and a row mask together: the launches of the three-pass form without its tri_bn_bwd_reduce, the given sums in
    the place of its own."""
    given = gen.run_bn_bwd(ops, 20000, 64, True, "final", True, True, keep, True, 1)
    own = gen.run_bn_bwd(ops, 20000, 64, True, "final", False, True, keep, True, 1)
    assert [l[0] for l in own] == ["tri_bn_bwd_reduce", "tri_bn_bwd_finalize", "tri_bn_bwd_apply", "return"] and own[0][5] == "t0"
    want = [[a if a != "t0" else "partial" for a in l] for l in own[1:]]
    want = [[f"t{int(a[1:]) - 1}" if isinstance(a, str) and a[0] == "t" and a[1:].isdigit() else a for a in l] for l in want]
    want[0][2] = 5                                                            # (the given sums hold five blocks, the query answers three)
    assert given == want
