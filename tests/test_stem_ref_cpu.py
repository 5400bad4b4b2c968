"""CPU: the case table of tests/_stem_ref.py reaches every kernel, template and branch of the first layer that
tests/test_stem_kernels_gpu.py promises to check, every exact row satisfies the conditions that bit-equality rests on, and the
float64 reference agrees with a plain loop nest."""
import itertools

import pytest
import torch

from tests import _conv_ref as R
from tests import _stem_ref as S

SIXTEEN = (S.F16, S.BF16)


def rows_with(op, code):
    return [r for r in S.EXACT_ROWS if S.row_branches(r)[op] == code]


def test_mirror_on_the_shapes_the_model_and_the_older_tests_use():
    assert S.stem_branches(S.F16, 32, 64, 640, 640, 2, 1) == {"fwd": S.TILE_VEC, "wgrad": S.TILE_VEC}
    assert S.stem_branches(S.F16, 16, 2, 16, 16, 2, 1) == {"fwd": S.GATHER, "wgrad": S.GATHER}
    assert S.stem_branches(S.F32, 64, 2, 40, 36, 2, 1) == {"fwd": S.GATHER, "wgrad": S.GATHER}
    assert S.stem_branches(S.F16, 32, 2, 21, 18, 2, 1) == {"fwd": S.TILE_SCALAR, "wgrad": S.TILE_SCALAR}
    # the padding guard moves the forward only
    assert S.stem_branches(S.F16, 32, 2, 20, 20, 3, 1) == {"fwd": S.MMA, "wgrad": S.MMA}
    assert S.stem_branches(S.F16, 32, 2, 20, 20, 3, 2) == {"fwd": S.GATHER, "wgrad": S.MMA}
    assert S.stem_branches(S.BF16, 64, 2, 8, 8, 1, 4) == {"fwd": S.GATHER, "wgrad": S.MMA}
    assert S.stem_branches(S.BF16, 64, 2, 8, 3, 1, 1) == {"fwd": S.MMA, "wgrad": S.MMA}
    # slices and alignment
    assert S.stem_branches(S.F16, 32, 2, 21, 18, 2, 1, y_ld=48, dy_ld=48) == {"fwd": S.GATHER, "wgrad": S.TILE_SCALAR}
    assert S.stem_branches(S.F16, 32, 2, 21, 18, 2, 1, dy_ld=36)["wgrad"] == S.GATHER
    assert S.stem_branches(S.F16, 32, 2, 21, 18, 2, 1, y_aligned=False, dy_aligned=False) == {"fwd": S.GATHER, "wgrad": S.GATHER}
    assert S.stem_branches(S.F16, 32, 2, 20, 20, 2, 1, x_aligned=False) == {"fwd": S.TILE_SCALAR, "wgrad": S.TILE_SCALAR}


def test_tiling_constants_stay_inside_what_the_kernels_assume():
    """NV <= 39 (the range the multiply-shift group index was checked for), a tile row fits its 136-element LDS row, and the tile's
    groups fit the 1024 group slots of a workgroup, for every stride and padding the tiling accepts."""
    for s, p in itertools.product((1, 2), (0, 1, 2, 3)):
        t = S.stem_tiling(2, 40, 40, s, p)
        assert t and t["shift"] == (-p) % 4 and t["NV"] <= 39 and 4 * t["NV"] <= 136 and 3 * t["RH"] * t["NV"] <= 1024
        assert t["shift"] + 63 * s + 2 < 4 * t["NV"]                 # the last column any operand slot reads
        mag = (65536 + t["NV"] - 1) // t["NV"]
        assert all((i * mag) >> 16 == i // t["NV"] for i in range(1024))
    assert S.stem_tiling(2, 40, 40, 3, 1) is None and S.stem_tiling(2, 40, 40, 1, 4) is None and S.stem_tiling(2, 40, 3, 1, 1) is None


def test_table_reaches_every_kernel_dtype_and_template():
    names = [S.row_id(r) for r in S.EXACT_ROWS + S.REAL_ROWS]
    assert len(names) == len(set(names))
    seen = S.promised()
    want = set()
    for op in ("fwd", "wgrad"):
        for code in (S.MMA, S.TILE_VEC, S.TILE_SCALAR):
            want |= {(op, code, dt, n) for dt in SIXTEEN for n in (32, 64)}
        want |= {(op, S.GATHER, dt, n) for dt in R.DTYPES for n in (16, 32, 64)}
    assert seen == want, (sorted(map(str, want - seen)), sorted(map(str, seen - want)))
    # the gather kernels at the width of each template and strictly inside it, in f32; inside it in 16 bit
    for op in ("fwd", "wgrad"):
        ns = {(r[1], r[2]) for r in rows_with(op, S.GATHER)}
        assert {(S.F32, n) for n in (5, 16, 24, 32, 48, 64)} <= ns
        assert {(dt, n) for dt in SIXTEEN for n in (5, 24, 48)} <= ns
    # 16-bit N = 32 / 64 on the gather kernels: the forward through the guard and through a y slice, the gradient through dy slices
    assert {r[2] for r in rows_with("fwd", S.GATHER) if r[1] in SIXTEEN and r[8] == r[2]} >= {32, 64}
    assert any(r[8] > r[2] and r[2] in (32, 64) and r[1] in SIXTEEN for r in rows_with("fwd", S.GATHER))
    assert any(r[9] % 8 and r[2] in (32, 64) and r[1] in SIXTEEN for r in rows_with("wgrad", S.GATHER))
    assert any(r[9] > r[2] and r[9] % 8 == 0 for r in rows_with("wgrad", S.MMA))
    assert any(r[9] > r[2] and r[9] % 8 == 0 for r in rows_with("wgrad", S.TILE_SCALAR) + rows_with("wgrad", S.TILE_VEC))
    assert all(1 <= r[3] <= 3 for r in S.EXACT_ROWS if r[0] not in S.CAP_ROWS)


def test_table_reaches_every_tiled_branch():
    tiled = [r for r in S.EXACT_ROWS if S.row_branches(r)["fwd"] >= S.TILE_VEC and r[0] not in S.CAP_ROWS]
    for code in (S.TILE_VEC, S.TILE_SCALAR):
        combos = {(r[6], r[7]) for r in tiled if S.row_branches(r)["fwd"] == code and r[13] == "exact"}
        assert combos == set(itertools.product((1, 2), (0, 1, 2, 3))), (code, combos)
    assert {S.stem_tiling(*r[3:8])["shift"] for r in tiled} == {0, 1, 2, 3}
    ohw = [S.out_hw(r[4], r[5], r[6], r[7]) for r in tiled]
    assert {1, 63, 64, 65, 130} <= {ow for _, ow in ohw} and {1, 3, 4, 5, 9} <= {oh for oh, _ in ohw}
    t = [S.stem_tiling(*r[3:8]) for r in tiled]
    assert any(g["tiles_x"] == 1 for g in t) and any(g["tiles_x"] > 1 for g in t)
    assert any(g["tiles_y"] == 1 for g in t) and any(g["tiles_y"] > 1 for g in t)
    assert any(g["tiles_x"] == 1 and g["tiles_y"] == 1 for g in t)
    assert any(r[5] == 4 for r in tiled), "IW = 4 is the smallest map the tiling takes"
    assert any(r[13] == "exact-xoff" and r[5] % 4 == 0 and S.row_branches(r)["fwd"] == S.TILE_SCALAR for r in tiled)


def test_table_reaches_the_gather_mma_branches_and_the_guard():
    mma = rows_with("fwd", S.MMA)
    assert {(r[6], r[7]) for r in mma} >= {(3, 0), (3, 1), (1, 1)} and any(r[5] == 3 for r in mma)
    assert all(r[7] <= 1 for r in mma), "a padding >= 2 shape must never reach stem_fwd_mma"
    M = [r[3] * S.out_hw(r[4], r[5], r[6], r[7])[0] * S.out_hw(r[4], r[5], r[6], r[7])[1] for r in mma]
    assert any(m < 32 for m in M) and any(m > 256 for m in M) and all(m % 128 for m in M)
    guarded = [r for r in S.EXACT_ROWS if r[0].startswith("guard")]
    assert {(r[6], r[7]) for r in guarded} >= {(3, 2), (1, 4)}
    for r in guarded:
        assert r[1] in SIXTEEN and r[2] in (32, 64) and S.row_branches(r) == {"fwd": S.GATHER, "wgrad": S.MMA}


def test_gather_rows_have_ragged_blocks_and_cap_rows_loop():
    for r in S.EXACT_ROWS:
        if r[0].startswith("gather") and "slices" not in r[0]:
            oh, ow = S.out_hw(r[4], r[5], r[6], r[7])
            M = r[3] * oh * ow
            g = S.stem_grids(*r[1:8])
            assert M > 1024 and M % 256 and g["fwd"][0] > 1 and g["wgrad"][0] > 1 and M % 64
    fwd, wg = S.find_row("cap-fwd"), S.find_row("cap-wgrad")
    assert fwd[1] in SIXTEEN and wg[1] in SIXTEEN and fwd[2] == wg[2] == 32
    g = S.stem_grids(*fwd[1:8])
    assert g["fwd"][1] > g["fwd"][0] == S.FWD_WG_CAP
    g = S.stem_grids(*wg[1:8])
    assert g["wgrad"][1] > 8 * S.WGRAD_WG_CAP and g["wgrad"][0] == S.WGRAD_WG_CAP


@pytest.mark.parametrize("row", S.EXACT_ROWS, ids=S.row_id)
def test_exact_row_satisfies_the_exactness_conditions(row):
    """`exact` asserts them (so a violated row cannot reach a comparison); the sparse rows past the caps are checked here first."""
    r = S.exact(row)
    N, B = row[2], row[3]
    oh, ow = S.out_hw(row[4], row[5], row[6], row[7])
    assert r["y"].shape == (B, N, oh, ow) and r["dw"].shape == (N, 3, 3, 3) and r["dy"].shape == r["y"].shape
    S.assert_stem_exact_conditions(r["x"], r["w"], r["dy"], r["y"], r["dw"], r["bias"])
    assert r["y"].abs().max() > 0 and r["dw"].abs().max() > 0
    if row[13] == "exact-sparse":
        assert set(r["x"].unique().tolist()) == {-1.0, 0.0, 1.0} and 0.2 < (r["dy"] != 0).double().mean() < 0.3


def test_conditions_refuse_a_row_that_would_round():
    x, w, dy = S.stem_int_operands(32, 12, 700, 65, 1, 1, sparse=False)
    y, _, dw = R.conv_ref(x, w, dy, 1, 1, 1, 1)
    with pytest.raises(AssertionError):
        S.assert_stem_exact_conditions(x, w, dy, y, dw)
    x, w, dy = S.stem_int_operands(8, 1, 5, 5, 1, 1, sparse=False)
    y, _, dw = R.conv_ref(x, w, dy, 1, 1, 1, 1)
    S.assert_stem_exact_conditions(x, w, dy, y, dw)
    with pytest.raises(AssertionError, match="bf16-exact"):
        S.assert_stem_exact_conditions(x, w, dy, y, dw, bias=torch.full((8,), 257.0, dtype=torch.float64))
    with pytest.raises(AssertionError, match="integers"):
        S.assert_stem_exact_conditions(x + 0.5, w, dy, y, dw)


@pytest.mark.parametrize("geo", [(2, 5, 6, 7, 2, 1), (1, 3, 4, 5, 1, 2)], ids=["s2p1", "s1p2"])
def test_reference_agrees_with_plain_loops(geo):
    B, N, H, W, s, p = geo
    x, w, dy = S.stem_int_operands(N, B, H, W, s, p, sparse=False)
    y, _, dw = R.conv_ref(x, w, dy, s, p, 1, 1)
    yl, _, dwl = R.conv_loops(x, w, dy, s, p, 1, 1)
    assert torch.equal(y, yl) and torch.equal(dw, dwl)


def test_real_rows_and_bn_rows():
    for row in S.REAL_ROWS:
        assert row[10] and row[11] and row[13] == "real" and row[8] == row[2] == row[9]
    assert {(S.row_branches(r)["fwd"], r[1]) for r in S.REAL_ROWS} == \
        {(c, dt) for c in (1, 2, 3, 4) for dt in SIXTEEN} | {(S.GATHER, S.F32)}
    assert [S.row_branches(S.find_row(n))["fwd"] for n in S.BN_ROWS] == [S.GATHER, S.MMA, S.TILE_VEC, S.TILE_SCALAR]
    rr = S.real(S.REAL_ROWS[0])
    r64, r32 = S.silu_refs(rr, 2, 1, True)
    assert r64.dtype == torch.float64 and r32.dtype == torch.float32 and (r64 - r32).abs().max() < 1e-5
