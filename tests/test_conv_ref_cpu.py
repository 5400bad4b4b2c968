"""The float64 convolution reference of tests/_conv_ref.py against a plain loop nest, the exactness conditions of every
integer case, and the branches of the depthwise dispatch that the case lists reach (no device needed)."""
import pytest
import torch

from tests import _conv_ref as R


@pytest.mark.parametrize("case", [
    (2, 3, 3, 5, 4, 3, 1, 1, 1, 3),              # depthwise 3x3
    (2, 4, 6, 7, 6, (3, 2), 2, 2, 2, 2),         # grouped + dilated + strided, rectangular filter, holes in dx
], ids=R.case_id)
def test_float64_reference_matches_loop_nest(case):
    B, C, N, H, W, k, s, p, d, g = case
    x, w, dy = R.int_operands(*case, seed=5)
    got = R.conv_ref(x, w, dy, s, p, d, g)
    want = R.conv_loops(x, w, dy, s, p, d, g)
    for a, b, what in zip(got, want, ("y", "dx", "dw")):
        assert a.shape == b.shape and torch.equal(a, b), what
    assert got[0].shape[2:] == R.out_hw(H, W, k, s, p, d)
    assert got[0].abs().sum() > 0 and got[1].abs().sum() > 0 and got[2].abs().sum() > 0


def _all_exact_cases():
    cases = [(B, C, C, H, W, k, s, p, d, C) for (B, C, H, W, k, s, p, d) in R.all_dw_cases()]
    cases += R.GROUPED_CASES
    cases += [c + (1,) for c in R.DENSE_CASES + R.DILATED_SPECIAL_CASES]
    return cases


@pytest.mark.parametrize("case", _all_exact_cases(), ids=R.case_id)
def test_exactness_conditions_hold_for_every_case(case):
    """|y|, 2|dx| <= 256 (bf16-exact integers), per-channel sum of y^2 and |2 dw| < 2^24 (f32-exact integers): asserted inside
    exact_case, for the seed the device tests use and two more."""
    big = case[:5] == (4, 1024, 1024, 66, 80)
    for seed in ((R.SEED,) if big else (1, 2, 3)):
        x, w, dy = R.int_operands(*case, seed=seed)
        y, dx, dw = R.conv_ref(x, w, dy, *case[6:])
        R.assert_exact_conditions(x, dy, y, dx, dw)
        assert y.abs().max() > 0 and dw.abs().max() > 0


def test_exactness_conditions_reject_a_case_that_rounds():
    x, w, dy = R.int_operands(2, 64, 64, 15, 17, 3, 2, 2, 2, 1)
    y, dx, dw = R.conv_ref(x, 40 * w, dy, 2, 2, 2, 1)
    with pytest.raises(AssertionError):
        R.assert_exact_conditions(x, dy, y, dx, dw)


def test_case_lists_hold_what_the_api_accepts():
    for dt in R.DTYPES:
        epc = 4 if dt == torch.float32 else 8
        for (B, C, N, H, W, k, s, p, d, g) in R.grouped_cases(dt):
            assert 1 < g < C and C % g == 0 and N % g == 0 and (C // g) % epc == 0 and (N // g) % epc == 0
        for (B, C, N, H, W, k, s, p, d) in R.DENSE_CASES + R.DILATED_SPECIAL_CASES:
            assert C % epc == 0 and N % epc == 0
    assert len(R.grouped_cases(torch.float32)) == 5 and len(R.grouped_cases(torch.float16)) == 4
    # the stride-2 / dilation-2 cases leave input parity classes without a tap, and so does the 3x1 filter at stride 2 (one
    # column tap at pad 1: only odd input columns are ever read)
    assert [R.dgrad_has_holes(*c[5:9]) for c in R.GROUPED_CASES] == [True, True, False, False, False]
    assert [R.dgrad_has_holes(*c[5:9]) for c in R.DENSE_CASES] == [False] * 5 + [True, False, False, True]
    for kk, s, p, d in R.DW_GEOMS:
        kh, kw = R.pair(kk)
        assert kh * kw <= 9


def test_depthwise_cases_reach_every_dispatch_branch():
    seen, labels = set(), {}
    for dt in R.DTYPES:
        for case in R.dw_cases(dt):
            B, C, H, W, k, s, p, d = case
            b = R.dw_branches(dt, C, H, W, k, s, p, d)
            labels[(dt, case)] = b
            seen |= {b["fwd"], b["dgrad"], b["wgrad"]}
            if b["channel_blocks"] > 1:
                seen.add(("second block", b["fwd"]))
        C = R.DW_SLICE_SHAPE[1]
        assert R.dw_branches(dt, C, 9, 20, 3, 1, 1, 1, ld=C + 16)["fwd"] == "window0"
        assert R.dw_branches(dt, C, 9, 20, 3, 1, 1, 1, ld=C + 4, aligned=False)["fwd"] == "scalar"
    assert {"window0", "window1", "window2", "vec", "scalar", "f16_3x3", ("second block", "vec"), ("second block", "scalar")} <= seen
    # the branch each shape was chosen for, for f16
    f16 = torch.float16
    assert labels[(f16, (2, 8, 7, 7, 3, 1, 1, 1))]["cpv"] == 1 and labels[(f16, (2, 8, 7, 7, 3, 1, 1, 1))]["fwd"] == "window0"
    assert labels[(f16, (1, 1024, 6, 13, 3, 1, 1, 1))]["fwd"] == "window0"
    assert labels[(torch.float32, (1, 1024, 6, 13, 3, 1, 1, 1))]["cpv"] == 256
    b = labels[(f16, (2, 24, 7, 5, 3, 1, 1, 1))]
    assert (b["fwd"], b["wgrad"], b["cpv"], b["rows_pb"]) == ("vec", "f16_3x3", 3, 85)
    assert labels[(f16, (1, 2056, 3, 4, 3, 1, 1, 1))]["channel_blocks"] == 2
    assert labels[(f16, (1, 300, 4, 5, 3, 1, 1, 1))] == {"fwd": "scalar", "dgrad": "scalar", "wgrad": "scalar", "cpv": 300, "rows_pb": 1,
                                                         "channel_blocks": 2}
    b = labels[(f16, R.DW_ADVANCE_CASE[0] + R.DW_ADVANCE_CASE[1])]
    assert b["wgrad"] == "f16_3x3" and b["rows_pb"] == 256 > 3 * 3          # more pixel rows per block than one image has outputs
    assert labels[(f16, R.DW_SHAPE_BIG + (3, 1, 1, 1))]["wgrad"] == "window2"
    for g in R.DW_GEOMS:                                                     # none of the other geometries may take the window kernel
        assert labels[(f16, R.DW_GEOM_SHAPE + g)]["fwd"] == "vec"
    assert {labels[(torch.float32, sh + (3, 1, 1, 1))]["fwd"] for sh in R.DW_SHAPES_F32_ONLY} == {"window0", "vec", "scalar"}


def test_real_family_bounds_are_finite_and_cover_a_float32_evaluation():
    """The bound has to be a bound: an f32 evaluation of the same convolution (what a correct kernel does at best) stays inside."""
    case = (2, 8, 8, 7, 6, 3, 2, 2, 2, 2)
    r = R.real_case(*case, dtype=torch.float16)
    y32 = torch.nn.functional.conv2d(r["x"].float(), r["w"].float(), None, 2, 2, 2, 2)
    assert R.worst_ratio(y32, r["y"], r["bound_y"] - R.U_OUT[torch.float16] * r["y"].abs()) <= 1.0
    for key in ("bound_y", "bound_y_bias", "bound_dx", "bound_dw", "bound_sum", "bound_sumsq"):
        assert torch.isfinite(r[key]).all() and (r[key] >= 0).all()
    # stride 2 with dilation 2: odd input rows receive no tap, so both the reference and the bound are zero there
    assert (r["dx"][:, :, 1::2] == 0).all() and (r["bound_dx"][:, :, 1::2] == 0).all() and (r["bound_dx"][:, :, 0::2] > 0).any()


def test_bn_tail_reference():
    ref = R.bn_tail_ref([10.0, -6.0], [60.0, 20.0], 4, [1.0, 2.0], [0.5, -0.5], 1e-3, 0.03, [0.0, 1.0], [1.0, 2.0])
    mu, var = 2.5, 60.0 / 4 - 2.5 ** 2
    assert ref["mean"][0][0] == mu and ref["mean"][1][0] == 0
    assert abs(ref["rstd"][0][0] - (var + 1e-3) ** -0.5) < 1e-7
    assert abs(ref["running_var"][0][0] - (0.97 * 1.0 + 0.03 * var * 4 / 3)) < 1e-6
    assert 0 < ref["scale"][1][0] < 1e-6 and set(ref) == {"mean", "rstd", "scale", "shift", "running_mean", "running_var"}
    assert set(R.bn_tail_ref([1.0], [1.0], 2, [1.0], [0.0], 1e-3, 0.03)) == {"mean", "rstd", "scale", "shift"}
