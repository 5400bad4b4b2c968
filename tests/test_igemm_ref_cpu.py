"""The case table of tests/_igemm_ref.py held to the restated dispatch rule, the exactness conditions of its integer cases, the
proof that sparse operands do not blind the exact comparison, six deliberate mistakes, and a float32 emulation of an MFMA-ordered
sum against the real family's bounds (no device needed).

Six deliberate mistakes (`I.mistakes`), applied to the float64 reference of every shape of `I.REAL_KERNELS` (to the results the real
family measures there: dw alone on the filter-gradient-only shapes): every one makes the exact comparison fail, and on real operands
lands above 1.0 x the bound of tests/_conv_ref.py `real_case`.  Smallest |wrong - right| / bound over those shapes and their
dtypes, computed by this file on the CPU: border tap 1.0e3 (H16x16 f16), last K stage 7.9e2 (h8x16 f16), statistics row 1.56 (H16x16
f16), tile one channel too wide inf (the neighbour of a slice has bound 0), parity class 1.8e3 (s2odd f16), pixel split 5.9e2 (w1056
bf16).  The test prints every figure; the assertion is > 1.0 and nothing is tuned to them.  The statistics figure is thin on purpose
of the bound, not of the test: `bound_sum` grows with K + M, one missing pixel is 1 / M of the sum, so the real family sees it at
K + M = 1088 (1.56) and would NOT see it on c192 (K + M = 2016: 0.97) — which is why the generic kernels' real-family shape is c40 /
k384, and why the exact family (where one missing pixel changes an integer) carries the mask checking.
"""
import pytest
import torch

from tests import _conv_ref as R
from tests import _igemm_ref as I

ROWS = I.rows()
TABLE_SHAPES = [n for n, e in I.SHAPES.items() if e["fwd"] or e["dgrad"] or e["wgrad"]]


def test_every_row_runs_the_configuration_it_names():
    """The table is the claim: forcing a row's configuration on its shape is legal by the restated rule, so the GPU test may demand
    that exactly this configuration ran."""
    assert len(ROWS) > 400
    for row in ROWS:
        op, cfg, dt, epi, name = row
        got = I.expected_cfg(row, cfg)
        if cfg >= 0:
            assert got == cfg, f"{I.row_id(row)}: the rule runs {got}"
        else:
            assert 0 <= got < (I.WGRAD_NCFG if op == "wgrad" else I.IGEMM_NCFG) or got == I.HALO_DGRAD_S2


def test_every_configuration_dtype_and_epilogue_is_in_the_table():
    have = {(op, cfg, dt, epi) for (op, cfg, dt, epi, _) in ROWS}
    for cfg in range(I.IGEMM_NCFG):
        if cfg in I.NEVER_LEGAL_IGEMM:
            continue
        for dt in I.igemm_dtypes(cfg):
            for epi in I.fwd_epis(cfg):
                assert ("fwd", cfg, dt, epi) in have, (cfg, dt, epi)
            for epi in I.DGRAD_EPIS:
                assert ("dgrad", cfg, dt, epi) in have, (cfg, dt, epi)
    for cfg in range(I.WGRAD_NCFG):
        for dt in I.wgrad_dtypes(cfg):
            assert ("wgrad", cfg, dt, 0) in have, (cfg, dt)
    # the fused-parity stride-2 input gradient, both channel tiles, and the same problems as four parity launches
    for name in ("s2odd", "s2even"):
        row = ("dgrad", -1, I.F16, 0, name)
        assert row in ROWS and I.expected_cfg(row, -1) == I.HALO_DGRAD_S2
        assert 0 <= I.expected_cfg(row, -1, {"dgrad_s2_halo": 0}) < I.IGEMM_NCFG
        assert I.expected_cfg(("dgrad", -1, I.BF16, 0, name), -1) < I.IGEMM_NCFG
    # stride-2 forward halo tiles keep their three specialisations
    for epi in (0, 1, 6):
        assert ("fwd", 15, I.F16, epi, "s2odd") in ROWS and ("fwd", 16, I.F16, epi, "s2even") in ROWS


def test_configuration_23_is_never_legal():
    """igemm.hip lists 23 (64 channels x 64-byte stages), sy11_igemm8_legal refuses it for every problem: no shape of the table, in
    either direction, makes the rule accept it — it is the one configuration the table cannot hold."""
    for name in TABLE_SHAPES:
        sh = I.SHAPES[name]["shape"]
        for epi in (0, 1, 6):
            assert not I.cfg_legal(I.fwd_args(sh, I.F16, epi), I.F16, 23)
        for a in I.dgrad_launches(sh, I.F16, False):
            assert not I.cfg_legal(a, I.F16, 23)


def test_every_patch_filter_gradient_instantiation_is_in_the_table():
    seen = set()
    for (op, cfg, dt, epi, name) in ROWS:
        sh = I.SHAPES[name]["shape"]
        if op == "wgrad" and 12 <= cfg < 16:
            ws = I.wgrad3x3p_ws(sh)
            seen.add((dt, ws, I.wgrad3x3p_sp(sh, ws), 64 if sh[1] > 32 else 32, 64 if sh[2] > 32 else 32))
    want = {(dt, ws, sp, cb, nb) for dt in I.HALF for (ws, sp) in I.PATCH_TILINGS for cb in (32, 64) for nb in (32, 64)}
    assert seen == want


def test_edges_the_shapes_were_chosen_for():
    sh = {n: e["shape"] for n, e in I.SHAPES.items()}
    M = lambda n: I.fwd_args(sh[n], I.F16, 0)["M"]
    assert M("c40") % 128 and M("c40") % 256 and sh["c40"][2] % 128 and sh["c40"][2] % 64 and sh["c40"][2] % 256
    assert (9 * sh["c40"][1]) % 32 and sh["c40"][1] < 64 and sh["c192"][1] % 64 == 0 and sh["c192"][2] % 64 == 0
    assert 9 * sh["c192"][1] // 64 > 4 and sh["k384"][1] == 384 and sh["p1x1"][1] == 128
    assert I.fwd_args(sh["c40"], I.F16, 1, y_ld=184)["vec_out"] and not I.fwd_args(sh["n20"], I.F16, 1)["vec_out"]
    assert not I.fwd_args(sh["n18"], I.F32, 1)["vec_out"] and not I.fwd_args(sh["n18"], I.F32, 18)["vec_out"]
    assert M("w1056") >= 1024 and I.cdiv(M("w1056"), 8 * 64) > 1                  # more than one pixel split
    # forced-but-illegal rows really are illegal, and the heuristic they fall back to differs from the forced value
    for row in I.FALLBACK_ROWS:
        assert I.expected_cfg(row, row[1]) != row[1], I.row_id(row)
    # igemm_deep: the heuristic pick is promoted where the rule allows, and only there
    assert I.expected_fwd(sh["c192"], I.F16, 1, {"igemm_deep": 1}) == 11 and I.expected_fwd(sh["c192"], I.F16, 2, {"igemm_deep": 2}) == 2
    assert I.expected_fwd(sh["c192"], I.BF16, 1, {"igemm_deep": 2}) == 2 and I.expected_fwd(sh["c120"], I.F16, 1, {"igemm_deep": 2}) == 2


@pytest.mark.parametrize("name", list(I.SHAPES))
def test_exactness_and_sensitivity_of_every_exact_case(name):
    """`exact` asserts the exactness conditions (|y|, 2|dx| <= 256, sums below 2^24) for the density the table sets; then: zeroing any
    one tap, or any 32-channel K slab of one tap, changes y / dx inside every 128-pixel x 32-channel block, and dropping any
    64-pixel stage of an image changes every 64 x 64 block of dw."""
    r = I.exact(name)
    assert r["y"].abs().max() > 0 and r["dx"].abs().max() > 0 and r["dw"].abs().max() > 0
    for seed in (2, 3):
        x, w, dy = R.int_operands(*I.case10(name), seed=seed, density=I.SHAPES[name]["density"])
        R.assert_exact_conditions(x, dy, *R.conv_ref(x, w, dy, *I.case10(name)[6:]))
    assert I.sensitivity_failures(name) == []


def test_density_default_is_unchanged_and_sparse_draw_is_sparse():
    a = R.int_operands(2, 8, 8, 5, 5, 3, 1, 1, 1, 1)
    g = torch.Generator().manual_seed(R.SEED)
    assert torch.equal(a[0], torch.randint(-1, 2, (2, 8, 5, 5), generator=g).double())
    x, w, dy = R.int_operands(2, 64, 64, 9, 9, 3, 1, 1, 1, 1, density=0.25)
    for t in (x, w, dy):
        assert set(t.unique().tolist()) == {-1.0, 0.0, 1.0} and 0.2 < (t != 0).double().mean() < 0.3


REAL_SHAPES = sorted({(name, dt, op) for (_, op, _, name, dts) in I.REAL_KERNELS for dt in dts}, key=str)


def _ops(name, dt=None):
    """The results the real family checks on a shape: everything where a forward kernel is measured, dw alone where only a filter
    gradient is."""
    kinds = {op for n, d, op in REAL_SHAPES if n == name and (dt is None or d == dt)}
    return ("wgrad",) if kinds == {"wgrad"} else ("fwd", "dgrad", "wgrad")

_worst = {}


@pytest.mark.parametrize("name", sorted({n for n, _, _ in REAL_SHAPES}))
def test_six_deliberate_mistakes_fail_both_families(name):
    case = I.case10(name)
    r = I.exact(name)
    wrong = I.mistakes(r, case)
    assert "one pixel split missing from dW" in wrong
    for what, (key, t) in wrong.items():
        assert not torch.equal(t, I.mistake_reference(r, key)), f"{name}: '{what}' passes the exact comparison"
    for dt in sorted({d for n, d, _ in REAL_SHAPES if n == name}, key=str):
        rr = I.real(name, dt)
        for what, (key, t) in I.mistakes(rr, case, _ops(name, dt)).items():
            ratio = R.worst_ratio(t, I.mistake_reference(rr, key), I.mistake_bound(rr, key))
            _worst[what] = min(_worst.get(what, float("inf")), ratio)
            print(f"MISTAKE {name} {str(dt)[6:]} {what}: {ratio:.3g} x bound")
            assert ratio > 1.0, f"{name} {dt}: '{what}' stays inside the real family's bound ({ratio:.3f})"


def test_all_six_mistakes_were_made_somewhere():
    names = set()
    for name in sorted({n for n, _, _ in REAL_SHAPES}):
        names |= set(I.mistakes(I.exact(name), I.case10(name)))
    assert len(names) == 6, names


@pytest.mark.parametrize("name", ["c192", "w1056"])
def test_float32_mfma_ordered_sum_stays_inside_half_the_bounds(name):
    """The largest K (c192: 1728) and the largest M (w1056) of the table: a float32 accumulation in MFMA-sized chunks — what a
    correct kernel does at best — uses at most half of each bound (without the output rounding term)."""
    for dt in I.ALL:
        rr = I.real(name, dt)
        y32, dw32 = I.mfma_ordered_sums(rr, I.case10(name))
        ry = R.worst_ratio(y32, rr["y"], rr["bound_y"] - R.U_OUT[dt] * rr["y"].abs())
        rw = R.worst_ratio(dw32, rr["dw"], rr["bound_dw"])
        print(f"EMULATION {name} {str(dt)[6:]}: y {ry:.3g} dw {rw:.3g}")
        assert ry <= 0.5 and rw <= 0.5
