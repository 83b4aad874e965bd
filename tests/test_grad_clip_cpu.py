"""CPU: the float64 reference of gradient clipping (tests/grad_clip_reference.py) agrees with torch's own utilities, each planted defect
moves it by more than 100x the tolerance of tests/test_gpu_grad_clip.py at that file's shapes, FusedAdam.set_gradient_clip validates its
arguments, and the new entry points refuse bad arguments before they launch anything.

train.fit's wiring is NOT tested here: fit() hands autograd the cached ops.one(device) scalar, which asks the HIP runtime whether a
capture is under way and fails on a box without a device, also with device="cpu".  That part is tests/test_gpu_grad_clip.py::
test_fit_reads_the_trainer_keys (FusedAdam and torch.optim.Adam)."""
import math
import os

import numpy as np
import pytest
import torch

from tests import grad_clip_reference as R


@pytest.fixture(scope="module")
def case():
    init, steps = R.case_tensors()
    return init, steps, R.adam_loop(init, steps, max_norm=R.MAX_NORM)


def test_norm_loop_agrees_with_torch_in_float64(case):
    init, steps, ref = case
    want, norms = R.torch_loop(init, steps, torch.float64, max_norm=R.MAX_NORM)
    assert R.max_distance(ref["p"], want) < 1e-13
    np.testing.assert_allclose(ref["norms"], norms, rtol=1e-14)
    # the case is what the issue describes: four steps clip, two do not
    assert [n > R.MAX_NORM for n in ref["norms"]] == [True, True, False, True, True, False] and ref["clipped"] == 4
    np.testing.assert_allclose(ref["norms"], [51, 1463, 4.96, 1469, 49.8, 5.01], rtol=0.02)
    # measure only: max_norm = inf is the unclipped loop
    free = R.adam_loop(init, steps, max_norm=math.inf)
    assert free["clipped"] == 0 and R.max_distance(free["p"], R.torch_loop(init, steps, torch.float64)[0]) < 1e-13


def test_value_loop_agrees_with_torch_in_float64(case):
    init, steps, _ = case
    for wd in (R.WD, R.WD_VALUE):
        got = R.adam_loop(init, steps, wd=wd, clip_value=R.CLIP_VALUE)
        want, _ = R.torch_loop(init, steps, torch.float64, wd=wd, clip_value=R.CLIP_VALUE)
        assert R.max_distance(got["p"], want) < 1e-13


def test_a_parameter_without_a_gradient_is_left_out(case):
    init, steps, _ = case
    holed = [[g if (i, j) != (1, 1) else None for j, g in enumerate(gs)] for i, gs in enumerate(steps)]
    got = R.adam_loop(init, holed, max_norm=R.MAX_NORM)
    want, norms = R.torch_loop(init, holed, torch.float64, max_norm=R.MAX_NORM)
    np.testing.assert_allclose(got["norms"], norms, rtol=1e-14)
    # (parameter 1 itself is not compared: torch counts ITS steps, FusedAdam - and so the reference - keeps one counter for all)
    assert R.max_distance([got["p"][0], got["p"][2]], [want[0], want[2]]) < 1e-13
    assert torch.equal(R.adam_loop(init, holed[1:2], max_norm=R.MAX_NORM)["p"][1], init[1].double())       # and it is left alone


def test_fp32_loop_distance_is_what_the_tolerance_assumes(case):
    """ATOL is four times the distance of torch's fp32 loop from its float64 loop on the GPU test's inputs (4.6e-7)."""
    init, steps, ref = case
    t32, _ = R.torch_loop(init, steps, torch.float32, max_norm=R.MAX_NORM)
    d = R.max_distance(t32, ref["p"])
    print(f"fp32 CPU loop vs float64: {d:.3e}")
    assert 0.5 * R.FP32_LOOP_DISTANCE < d < 1.05 * R.FP32_LOOP_DISTANCE
    assert R.ATOL == 4 * R.FP32_LOOP_DISTANCE
    # the test has something to see: without clipping more than 98 % of the elements end more than 100 tolerances away
    free = R.adam_loop(init, steps)
    far = torch.cat([(a - b).abs().reshape(-1) for a, b in zip(free["p"], ref["p"])])
    assert float((far > 100 * R.ATOL).double().mean()) > 0.98 and 5e-3 < float(far.median()) < 2e-2


def test_planted_defects_move_the_result_by_more_than_100_tolerances(case):
    init, steps, ref = case
    # the coefficient not applied to one segment (optimizer-path case, ATOL)
    bad = R.adam_loop(init, steps, max_norm=R.MAX_NORM, defect="coef_skips_segment")
    assert float((bad["p"][1] - ref["p"][1]).abs().max()) > 100 * R.ATOL
    # the clamp applied after the weight decay (value case, ATOL)
    good = R.adam_loop(init, steps, wd=R.WD_VALUE, clip_value=R.CLIP_VALUE)
    bad = R.adam_loop(init, steps, wd=R.WD_VALUE, clip_value=R.CLIP_VALUE, defect="clamp_after_decay")
    assert R.max_distance(bad["p"], good["p"]) > 100 * R.ATOL
    # ... which wd = 1e-6 could not show (why the value case has a weight decay of its own)
    weak = R.max_distance(R.adam_loop(init, steps, clip_value=R.CLIP_VALUE, defect="clamp_after_decay")["p"],
                          R.adam_loop(init, steps, clip_value=R.CLIP_VALUE)["p"])
    assert weak < R.ATOL
    # a NULL segment counted in the norm (segment case: equality, and NORM_RTOL for random values)
    for make in (R.integer_gradient, lambda n, s: torch.randn(n, generator=torch.Generator().manual_seed(s))):
        segs = [make(n, 100 + n) for n in R.SEG_SIZES]
        present = [segs[0], None, segs[2], segs[3]]
        a, b = R.total_norm(present), R.total_norm(present, defect="null_counted", stale=segs)
        assert abs(a - b) / a > 100 * R.NORM_RTOL
        assert R.rec_fp32(a, R.MAX_NORM) != R.rec_fp32(b, R.MAX_NORM)
    # the last ragged piece dropped (flat case, the size that has one)
    n = R.FLAT_SIZES[3]
    assert n % 4
    for g in (R.integer_gradient(n, n), torch.randn(n, generator=torch.Generator().manual_seed(n))):
        a, b = R.total_norm([g]), R.total_norm([g], defect="ragged_dropped")
        assert abs(a - b) / a > 100 * R.NORM_RTOL and R.rec_fp32(a, R.MAX_NORM)[0] != R.rec_fp32(b, R.MAX_NORM)[0]


def test_integer_gradients_sum_exactly():
    """|g| <= 1024 and integer: every partial sum is an integer below 2^53, so the order of the additions cannot matter."""
    n = R.FLAT_SIZES[-1]
    g = R.integer_gradient(n, n)
    assert float(g.abs().max()) <= 1024 and bool((g == g.round()).all()) and n * 2 ** 20 < 2 ** 53
    s = (g.double() ** 2)
    assert float(s.sum()) == float(s.flip(0).sum()) == float(s.reshape(-1, 4).sum(0).sum())


def test_coefficient_rule():
    assert R.coefficient(10.0, 20.0) == 1.0 and R.coefficient(0.0, 20.0) == 1.0 and R.coefficient(1e30, math.inf) == 1.0
    assert R.coefficient(40.0, 20.0) == 20.0 / (40.0 + 1e-6)
    assert R.coefficient(math.inf, 20.0) == 1.0 and R.coefficient(math.nan, 20.0) == 1.0
    r = R.rec_fp32(math.inf, 20.0)
    assert np.isinf(r[0]) and r[1] == np.float32(1.0)


def test_set_gradient_clip_validation():
    from tricolo_amd.optim import FusedAdam
    w = [torch.nn.Parameter(torch.zeros(8))]
    opt = FusedAdam(w)
    assert opt._clip is None and opt.grad_norm() is None and opt.clipped_steps() == 0
    for bad in (0, 0.0, -1.0, math.nan):
        for alg in ("norm", "value"):
            with pytest.raises(ValueError, match="positive"):
                opt.set_gradient_clip(bad, alg)
            with pytest.raises(ValueError, match="positive"):
                FusedAdam(w, **{"max_grad_norm" if alg == "norm" else "clip_grad_value": bad})
    with pytest.raises(ValueError, match="algorithm"):
        opt.set_gradient_clip(1.0, "inf")
    with pytest.raises(ValueError, match="exclude"):
        FusedAdam(w, max_grad_norm=1.0, clip_grad_value=1.0)
    assert opt._clip is None                                         # a refused call changes nothing
    opt.set_gradient_clip(2, "norm")
    assert opt._clip == ("norm", 2.0)
    opt.set_gradient_clip(math.inf)                                  # measure only
    assert opt._clip == ("norm", math.inf)
    opt.set_gradient_clip(0.5, algorithm="value")
    assert opt._clip == ("value", 0.5)
    opt.set_gradient_clip(None)
    assert opt._clip is None
    assert FusedAdam(w, max_grad_norm=20)._clip == ("norm", 20.0) and FusedAdam(w, clip_grad_value=0.5)._clip == ("value", 0.5)
    # the checkpoint format does not know about clipping
    assert set(FusedAdam(w, max_grad_norm=20).state_dict()) == set(FusedAdam(w).state_dict()) == {"state", "param_groups"}
    assert "max_grad_norm" not in FusedAdam(w, max_grad_norm=20).state_dict()["param_groups"][0]


def test_entry_points_refuse_bad_arguments_before_launching():
    """max_norm <= 0 or NaN, clip_value <= 0 or NaN, nblk < 0 and NULL outputs are TRI_ERR_ARG with a message; the checks run on the host,
    ahead of any HIP call, so no device is needed (the pointers below are never dereferenced)."""
    from tricolo_amd import _C
    if not os.path.exists(_C.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _C.lib()
    fake = 4096                                                      # a non-NULL address
    assert lib.tri_grad_norm_blocks(0) == 1 and lib.tri_grad_norm_blocks(4) == 1 and lib.tri_grad_norm_blocks(1020) == 1
    assert lib.tri_grad_norm_blocks(1024) == 2 and lib.tri_grad_norm_blocks(R.FLAT_SIZES[-1]) == 4096 == lib.tri_grad_norm_blocks(1 << 40)
    assert lib.tri_grad_norm_blocks(-1) == _C.TRI_ERR_ARG
    for max_norm in (0.0, -1.0, math.nan):
        assert lib.tri_grad_clip_coef(fake, 1, 1.0, max_norm, fake, fake, None) == _C.TRI_ERR_ARG
        assert b"max_norm" in lib.tri_last_error()
    assert lib.tri_grad_clip_coef(fake, -1, 1.0, 1.0, fake, fake, None) == _C.TRI_ERR_ARG
    assert lib.tri_grad_clip_coef(fake, 1, 1.0, 1.0, None, fake, None) == _C.TRI_ERR_ARG
    assert lib.tri_grad_clip_coef(fake, 1, 1.0, 1.0, fake, None, None) == _C.TRI_ERR_ARG
    assert lib.tri_grad_clip_coef(None, 1, 1.0, 1.0, fake, fake, None) == _C.TRI_ERR_ARG
    assert lib.tri_grad_sumsq(fake, 4, None, None) == _C.TRI_ERR_ARG and lib.tri_grad_sumsq(fake, -4, fake, None) == _C.TRI_ERR_ARG
    assert lib.tri_grad_sumsq(fake + 2, 4, fake, None) == _C.TRI_ERR_ARG
    assert lib.tri_grad_sumsq_segments(fake, fake, 1, 8, None, None) == _C.TRI_ERR_ARG
    assert lib.tri_grad_sumsq_segments(fake, fake, 0, 8, fake, None) == _C.TRI_ERR_ARG
    assert lib.tri_grad_sumsq_segments(fake, fake, 1025, 8, fake, None) == _C.TRI_ERR_ARG
    assert lib.tri_grad_sumsq_segments(fake, fake, 1, 6, fake, None) == _C.TRI_ERR_ARG
    for cv in (0.0, -0.5, math.nan):
        assert lib.tri_adam_step_clipped(fake, fake, fake, fake, 4, fake, 1e-3, None, 0.9, 0.999, 1e-8, 0.0, 1.0, None, cv, None) == _C.TRI_ERR_ARG
        assert b"clip_value" in lib.tri_last_error()
        assert lib.tri_adam_step_segments_clipped(fake, fake, fake, 1, fake, fake, 4, fake, 1e-3, None, 0.9, 0.999, 1e-8, 0.0, 1.0, None, cv,
                                                  None) == _C.TRI_ERR_ARG
