"""The conv planner's answers, pinned on the CPU (tests/golden/conv_plan.npz, tools/make_conv_plan_golden.py).

Which kernel family runs a tri_conv_fwd / tri_conv_dgrad / weight-gradient call, how many BatchNorm records it writes and how much
scratch it needs are host decisions: the planner answers them without a GPU (256 compute units assumed, the MI355X's).  The table
was recorded before the routing code was rewritten around one family table (route_table: before the weight gradient's was, through a literal
copy of its if-chain); every cell must come out the same, by default and under every A/B switch that shows in
a plan query.  TRICOLO_S2D_TY, TRICOLO_HALO_PROD and TRICOLO_HALO_XCG act at launch time only
and stay with their GPU tests.

Where the GPU suite reaches each outcome of each row of conv_families[] (csrc/conv_igemm.hip), bit for bit against torch on integer
data (tests/test_gpu_ops.py unless named otherwise; "16bit" = test_conv_16bit_storage_integer_exact):
  vox0       runs / refuses a row list: test_voxel_level0_brick_kernel.
  voxb       runs / refuses a row list: test_voxel_level1_ranked_brick_kernel (32^3: test_opt_in_kernels_child_process[voxb32]).
  voxg       runs forward and data gradient / refuses a row list: test_voxel_coarse_grid_kernel.
  stem       runs: 16bit[stem_*]; falls through (row mask, conv_igemm_kernel): 16bit[stem_3x3].
  pw         runs both directions, falls through (accumulate, conv_dma_kernel): 16bit[c1x1s2, pw_*].
  c64        runs both directions, with accumulate, statistics and BatchNorm-backward sums (none on 56- / 64-wide images): 16bit[c64k_*,
             c64_*, big_nosplit, h_56, h_many]; falls through (row mask) and refuses (row mask + statistics): 16bit[c64k_16].
  s2g        runs / refuses bias + activation: test_stride2_slab_kernel; a row-major operand: test_packed_operand_order_is_checked.
  s2d        runs, with accumulate; its layer's forward falls through to conv_dma_kernel: 16bit[s2d_*]; row mask: 16bit[s2d_16].
  halo rows  runs with statistics / accumulate: 16bit[h_*]; falls through (row mask): 16bit[h_8x8].
  halo2d     runs: test_gpu_bench_plan.py (layer2 at the bench shape) and, with the row mask, test_halo_kernels_ab_switch[0].
  dma, igemm every other case, masked / row-list / split-K forms: test_conv_16bit_storage_masked_stats, test_gpu_modules.py.
The forward-only rows' "falls through on a data gradient" needs a layer whose data-gradient view looks like their forward (a 64 -> 32
channel 3x3x3 layer on a 16^3 grid for voxb; none exists for vox0 and stem, whose views would have 4 output channels): no tower has
one; the recorded table pins what the family query answers for it.
"""
import importlib.util
import os

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")

_spec = importlib.util.spec_from_file_location("make_conv_plan_golden", os.path.join(REPO, "tools", "make_conv_plan_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

FWD_DGRAD_FAMILIES = {0, 2, 3, 4, 5, 6, 9, 10, 12, 13, 14, 15}
WGRAD_FAMILIES = {0, 2, 6, 7}                                   # tri_conv_wgrad_kernel_family: the layer's class
WGRAD_ROUTE_FAMILIES = {0, 2, 4, 6, 7, 9}                       # tri_conv_wgrad_route: the kernel of a call, every row of wgrad_families[]
GROUP_FAMILIES = {0, 1, 2, 4, 5, 7}


@pytest.fixture(scope="module")
def rec():
    return dict(np.load(os.path.join(GOLDEN, "conv_plan.npz"), allow_pickle=False))


def _col(rec, prefix):
    cols = [i for i, c in enumerate(rec["columns"]) if str(c).startswith(prefix)]
    assert cols, prefix
    return rec["table"][:, cols]


def _skip_unless_reference_machine():
    if any(k.startswith("TRICOLO_") and k not in ("TRICOLO_HELDOUT_STEPS",) for k in os.environ):
        pytest.skip("a TRICOLO_* variable is set: the recorded table is the default switch set's")
    import torch
    if torch.cuda.is_available() and torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip("the table was recorded for 256 compute units")


def test_recorded_table_covers_every_family(rec):
    """A trimmed sweep cannot pass by leaving a family out."""
    assert os.path.getsize(os.path.join(GOLDEN, "conv_plan.npz")) < 128 * 1024
    assert list(rec["columns"]) == gen.COLUMNS and list(rec["switches"]) == gen.SWITCHES
    assert np.array_equal(rec["desc"], gen.descriptors())
    fam = _col(rec, "family_")
    assert set((fam & 255).ravel().tolist()) == FWD_DGRAD_FAMILIES
    halo = fam[np.isin(fam & 255, (3, 5))]
    assert set(((halo >> 8) & 255).tolist()) == {2, 3}                         # both halo tile sizes
    assert int(((fam >> 16) & 1).sum()) >= 1000                                # split-K plans
    assert set(_col(rec, "wgrad_family_").ravel().tolist()) == WGRAD_FAMILIES
    rc = _col(rec, "wgrad_group_rc_")
    assert set(_col(rec, "wgrad_group_family_")[rc == 0].tolist()) == GROUP_FAMILIES
    assert list(rec["route_columns"]) == gen.ROUTE_COLUMNS and rec["route_table"].shape == (len(rec["desc"]), len(gen.ROUTE_COLUMNS))
    route = {k: rec["route_table"][:, [str(c).endswith(k) for c in rec["route_columns"]]] for k in ("dense", "mask", "rows")}
    codes = {k: set((v[v >= 0] & 255).tolist()) for k, v in route.items()}
    assert codes["dense"] | codes["mask"] | codes["rows"] == WGRAD_ROUTE_FAMILIES
    assert {4, 9} <= codes["dense"] and not {4, 9} & (codes["mask"] | codes["rows"])    # stem and c64: dense calls only
    assert 6 in codes["mask"] and (rec["route_table"] < 0).any()                        # the brick kernel; refused calls
    assert (_col(rec, "dgrad_bn_records_") > 0).any() and (_col(rec, "workspace_") > 0).any()
    assert len(set(rec["switch_sha256"].tolist())) > 1 and gen.table_sha256(rec["table"]) not in set(rec["switch_sha256"].tolist())
    assert gen.table_sha256(np.hstack([rec["table"], rec["route_table"]])) not in set(rec["switch_sha256_all"].tolist())


def test_default_table_reproduces(rec):
    _skip_unless_reference_machine()
    got = gen.compute_table(rec["desc"])
    want = rec["table"]
    bad = np.argwhere(got != want)
    for i, c in bad[:20]:
        print(f"desc {rec['desc'][i].tolist()} column {rec['columns'][c]}: recorded {want[i, c]}, computed {got[i, c]}")
    assert len(bad) == 0, f"{len(bad)} cells of the plan table changed"
    got, want = gen.compute_routes(rec["desc"]), rec["route_table"]
    bad = np.argwhere(got != want)
    for i, c in bad[:20]:
        print(f"desc {rec['desc'][i].tolist()} column {rec['route_columns'][c]}: recorded {want[i, c]}, computed {got[i, c]}")
    assert len(bad) == 0, f"{len(bad)} cells of the weight-gradient route table changed"


@pytest.mark.parametrize("switch", gen.SWITCHES)
def test_switch_table_reproduces(rec, switch):
    """One A/B switch, set in a fresh child process (the library reads each switch once): the table's SHA-256, and that of the table
    and the weight-gradient route table side by side."""
    _skip_unless_reference_machine()
    want = dict(zip(rec["switches"].tolist(), rec["switch_sha256"].tolist()))[switch]
    assert gen.switch_sha256(switch) == want, f"the plan table under {switch} changed"
    want = dict(zip(rec["switches"].tolist(), rec["switch_sha256_all"].tolist()))[switch]
    assert gen.switch_sha256(switch, all_columns=True) == want, f"the weight-gradient route table under {switch} changed"


def test_python_family_table_matches_recorded_codes(rec):
    """ops.CONV_FAMILIES restates, per family code, what Python needs of the C table: every recorded code is a key, and the
    site-mask walkers / fragment-major readers are the ones the literals named before the table existed."""
    from tricolo_amd import ops
    fam = _col(rec, "family_") & 255
    assert set(fam.ravel().tolist()) <= set(ops.CONV_FAMILIES)
    brick = np.vectorize(lambda c: ops.CONV_FAMILIES[c].site_mask)(fam)
    frag = np.vectorize(lambda c: ops.CONV_FAMILIES[c].frag)(fam)
    assert np.array_equal(brick, np.isin(fam, (6, 13, 14)))
    assert np.array_equal(frag, np.isin(fam, (13, 14, 15)))
    g = ops.ConvGeom(2, (4, 4, 4), 128, 128, 256, (3, 3, 3), 1, (1, 1, 1), (27 * 128, 128, 1))      # a voxg layer
    code = g.kernel_family[(False, 2)]
    assert code & 255 == 13 and g.brick(False, 2) and g.packed_frag(False, "f16") == 1 and g.voxg_spu(False, 2) == (code >> 24) & 127
    assert not g.brick(False, 0) and g.packed_frag(False, "bf16x3") == 0 and g.voxg_spu(False, 0) == 0
    assert g.splitk(False, 0) == bool(g.kernel_family[(False, 0)] >> 16 & 1)
