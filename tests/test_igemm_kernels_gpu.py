"""Every dense convolution tile configuration (igemm 0..25, the fused-parity stride-2 input gradient, wgrad 0..19) against the
float64 reference, with proof of which configuration ran: after every call "igemm_last_cfg" / "wgrad_last_cfg" must equal the
restated dispatch rule of tests/_igemm_ref.py (`expected_cfg`) BEFORE anything is compared.

Exact family (integer operands, results BIT-EQUAL to float64): one test per (shape, dtype) of the table, on contiguous tensors and
on channel slices of wider buffers whose neighbours hold a sentinel.  Per forced configuration: y with 1-D and 8-slot statistics in
both reduction modes, plain y, y + bias, y + bias as f32, statistics + bias (no specialisation: the runtime-flag build, in f16 and
f32 too — the wrapper accepts the combination; statistics are taken before the bias), bias + SiLU against the project's bar
(`close_to_scale`, mult 2), dx plain and accumulated onto itself, dw after one and two calls in both modes.
Fallbacks: one forced-but-illegal configuration per legality clause; the heuristic pick must run and the result stays exact.
Real family: one shape per distinct kernel, element-by-element bounds of tests/_conv_ref.py `real_case`, worst err / bound printed.

The tests run with "tune" 0 and an EMPTY pick table (a recorded pick would be honoured over the heuristic); the table of the
process is put back afterwards.

Worst err / bound of the real family per kernel, MI355X, when the tests were written (y / y + bias / dx / dw; sum and sumsq stay
below 1e-3; the 16-bit y and dx figures are the rounding of the stored output, the u_out term being exactly half an ulp):
igemm 64- and 128-byte stages (cfg 0 / 4, c40) f32 0.005 / 0.005 / 0.002 / 0.006, f16 0.72 / 0.71 / 0.37 / 0.002, bf16 0.92 / 0.92 /
0.75 / 0.002; 4-deep ring (9), 256 x 128 (3), igemm8 kb 128 / kb 64 / bn 256 / persistent (20 / 22 / 24 / 25) on c40 f16: y 0.72,
y + bias 0.71; 3-deep ring (12, k384) 0.62 / 0.62; 1x1 persistent (7) f16 0.88 / 0.87 / 0.92, bf16 0.96 / 0.98 / 0.98; halo
128-pixel (15) 0.52 / 0.53, 256-pixel (17) 0.51 / 0.58 / 0.58; few-channel (19) f16 0.88 / 0.87 / 0.77, bf16 0.98 / 0.97 / 0.94;
halo_dgrad_s2 dx 0.93; dw: wgrad_kernel<float> 0.001, wgrad16 plain / pixel-split / wide tile < 0.001 in f16 and bf16, patch kernel
0.004 / 0.003.  Nothing is tuned to these figures: the bounds come from the operation counts.
"""
import pytest
import torch

from tests import _conv_ref as R
from tests import _igemm_ref as I
from tests.test_conv_variants_gpu import (DEV, View, close_to_scale, filter_gradient, forward_and_stats, input_gradient, krsc, lib, ops,
                                          options, same)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def empty_pick_table():
    """No measuring, and no recorded pick either: the dispatch is the forced configuration or the static heuristic."""
    L = lib()
    saved = L.tune_export()
    L.check(L.load().sy11_tune_clear(), "sy11_tune_clear")
    with options(tune=0, igemm_cfg=-1, wgrad_cfg=-1, igemm_deep=0, igemm_korder=1, igemm_bpol=0, dgrad_s2_halo=1):
        yield
    L.check(L.load().sy11_tune_clear(), "sy11_tune_clear")
    L.tune_import(saved)


class Checked:
    """The three conv entry points of sy11.ops; after each call the configuration that ran must be the one the rule names."""

    def __init__(self, name, dt, forced_igemm=-1, forced_wgrad=-1, lds=None, **opts):
        self.o, self.name, self.dt, self.fi, self.fw, self.lds, self.opts = ops(), name, dt, forced_igemm, forced_wgrad, lds or {}, opts
        self.weight_transpose = self.o.weight_transpose

    def _check(self, op, epi, forced, option):
        row = (op, forced, self.dt, epi, self.name)
        want = I.expected_cfg(row, forced, dict(self.opts, **self.lds))
        got = lib().get_option(option)
        assert got == want, f"{I.row_id(row)} {self.opts}: configuration {got} ran, the rule names {want}"
        return got

    def conv2d_fwd(self, x, w, y, k, s=1, p=0, d=1, groups=1, bias=None, stats=None, silu=False, out_f32=False):
        self.o.conv2d_fwd(x, w, y, k, s, p, d, groups, bias=bias, stats=stats, silu=silu, out_f32=out_f32)
        return self._check("fwd", (1 if stats else 0) | (2 if bias is not None else 0) | (4 if silu else 0) | (16 if out_f32 else 0), self.fi,
                           "igemm_last_cfg")

    def conv2d_dgrad(self, dy, wt, dx, y_shape, k, s=1, p=0, d=1, groups=1, accumulate=False):
        self.o.conv2d_dgrad(dy, wt, dx, y_shape, k, s, p, d, groups, accumulate=accumulate)
        return self._check("dgrad", 8 if accumulate else 0, self.fi, "igemm_last_cfg")

    def conv2d_wgrad(self, x, dy, dw, k, s=1, p=0, d=1, groups=1):
        self.o.conv2d_wgrad(x, dy, dw, k, s, p, d, groups)
        return self._check("wgrad", 0, self.fw, "wgrad_last_cfg")


class Tensors:
    """Device operands of one exact (or real) case, contiguous or as channel slices of wider buffers."""

    def __init__(self, name, dt, r, sliced):
        B, C, N, H, W, k, s = I.SHAPES[name]["shape"]
        OH, OW = R.out_hw(H, W, k, s, k // 2, 1)
        sl = (lambda ch, pad, off: (ch + pad, off)) if sliced else (lambda ch, pad, off: (None, 0))
        self.x, self.dy = View(B, H, W, C, dt, *sl(C, 16, 8), src=r["x"]), View(B, OH, OW, N, dt, *sl(N, 16, 8), src=r["dy"])
        self.y, self.dx = View(B, OH, OW, N, dt, *sl(N, 24, 16)), View(B, H, W, C, dt, *sl(C, 8, 8))
        self.y32 = View(B, OH, OW, N, torch.float32, *sl(N, 24, 16))
        self.wk = krsc(r["w"], dt)
        self.wt = ops().weight_transpose(self.wk)
        self.geo = (k, s, k // 2, 1)
        self.lds = {"x_ld": self.x.buf.shape[-1], "y_ld": self.y.buf.shape[-1], "dy_ld": self.dy.buf.shape[-1], "dx_ld": self.dx.buf.shape[-1]}
        gen = torch.Generator().manual_seed(9)
        self.bias64 = torch.randint(-3, 4, (N,), generator=gen).double()
        self.bias = self.bias64.float().to(DEV)


def forward_epilogue(o, r, t, epi, what):
    """One forward epilogue of an exact case other than plain statistics (forward_and_stats covers epi 1)."""
    k, s, p, d = t.geo
    N = r["y"].shape[1]
    yb = r["y"] + t.bias64.view(1, -1, 1, 1)
    assert yb.abs().max().item() <= 256, "y + bias leaves the bf16-exact integers: fix the case"
    out = t.y32 if epi & 16 else t.y
    out.buf.fill_(77.0)
    st = torch.zeros(2, N, device=DEV)
    o.conv2d_fwd(t.x.v, t.wk, out.v, k, s, p, d, 1, bias=t.bias if epi & 2 else None, stats=(st[0], st[1]) if epi & 1 else None,
                 silu=bool(epi & 4), out_f32=bool(epi & 16))
    if epi & 4:
        close_to_scale(out.nchw(), torch.nn.functional.silu(yb), t.x.v.dtype, f"{what} bias + SiLU", mult=2)
    else:
        same(out.nchw(), yb if epi & 2 else r["y"], f"{what} y (epi {epi})")
    if epi & 1:
        same(st[0], r["y"].sum((0, 2, 3)), f"{what} sum (epi {epi})")
        same(st[1], (r["y"] * r["y"]).sum((0, 2, 3)), f"{what} sumsq (epi {epi})")
    out.assert_neighbours_untouched(f"{what} y (epi {epi})")
    t.x.assert_neighbours_untouched(f"{what} x")


def run_rows(name, dt, sliced, rows, pick=None, **opts):
    """Every row of one (shape, dtype): rows grouped by (op, forced configuration), the float64 reference computed once.  `opts` are
    library options set for the calls; `pick` is what the pick table holds for the forward problem (the caller imported it)."""
    r = I.exact(name)
    t = Tensors(name, dt, r, sliced)
    groups = {}
    for (op, cfg, _, epi, _) in rows:
        groups.setdefault((op, cfg), []).append(epi)
    ran = {}
    for (op, cfg), epis in groups.items():
        what = f"{name} {str(dt)[6:]} {'sliced' if sliced else 'contiguous'} {op} cfg {cfg} {opts}"
        if op == "wgrad":
            o = Checked(name, dt, forced_wgrad=cfg, lds=t.lds, **opts)
            for det in (1, 0):
                with options(wgrad_cfg=cfg, deterministic=det, **opts):
                    filter_gradient(o, r, t.x, t.dy, t.geo, 1, f"{what} deterministic={det}")
            continue
        o = Checked(name, dt, forced_igemm=cfg, lds=t.lds, pick=pick, **opts)
        with options(igemm_cfg=cfg, **opts):
            for epi in epis:
                if op == "fwd" and epi == 1:
                    for det in (1, 0):
                        with options(deterministic=det):
                            forward_and_stats(o, r, t.x, t.wk, t.y, t.geo, 1, f"{what} deterministic={det}")
                elif op == "fwd":
                    forward_epilogue(o, r, t, epi, what)
                elif epi == 0:            # epi 8 rides along: input_gradient runs plain, then accumulated onto itself
                    input_gradient(o, r, t.dy, t.wt, t.dx, t.geo, 1, what, plain_refused=False)
            ran[(op, cfg)] = lib().get_option("igemm_last_cfg")
    t.dy.assert_neighbours_untouched(f"{name} dy")
    return ran


@pytest.mark.parametrize("sliced", [False, True], ids=["contiguous", "sliced"])
@pytest.mark.parametrize("name,dt", I.shape_dtype_pairs(), ids=lambda v: v if isinstance(v, str) else str(v)[6:])
def test_exact_rows(name, dt, sliced):
    run_rows(name, dt, sliced, I.rows_of(name, dt))


# ------------------------------------------------------------------------------------------------------------ options
KORDER_CFGS = {"c192": [0, 1, 2, 4, 9, 12, 3, 20, 22, 25], "c40": [0, 4, 20, 24, 25]}


@pytest.mark.parametrize("name", list(KORDER_CFGS))
@pytest.mark.parametrize("dt", I.ALL, ids=lambda d: str(d)[6:])
def test_k_order_and_filter_cache_policy(name, dt):
    """igemm_korder 0 (channels innermost) on one configuration of each family; the default 1 is what every other test runs.  c192 has
    whole stages per tap (the two orders really differ); c40 does not, and the order silently degrades to 0.  igemm_bpol 1 / 2: the
    library stores it in the argument struct and no kernel of this build reads it — the results must not change."""
    rows = [r for r in I.rows_of(name, dt) if r[1] in KORDER_CFGS[name] and r[0] != "wgrad" and r[3] in (1, 0, 8)]
    assert rows
    run_rows(name, dt, True, rows, igemm_korder=0)
    for bpol in (1, 2):
        run_rows(name, dt, False, [r for r in rows if r[1] in (0, 20, 25)], igemm_bpol=bpol)


@pytest.mark.parametrize("deep", [1, 2])
@pytest.mark.parametrize("name", ["c192", "c40", "p1x1", "c120", "h8x16"])
def test_deep_rings_promote_the_heuristic_pick(name, deep):
    """igemm_deep 1 / 2 moves the heuristic's 0..2 to 9..11 where that is legal (f16, K >= 128, the training / inference epilogues) —
    read back from igemm_last_cfg — and nothing else: not bf16 / f32, not the bias epilogue, not K = 120, not a halo pick, and
    never a forced configuration."""
    sh = I.SHAPES[name]["shape"]
    for dt in I.ALL:
        rows = [("fwd", -1, dt, e, name) for e in (1, 0, 2, 6)] + [("dgrad", -1, dt, e, name) for e in (0, 8)]
        ran = run_rows(name, dt, False, rows, igemm_deep=deep)
        if name in ("c192", "c40"):
            assert (9 <= ran[("dgrad", -1)] <= 11) == (dt == I.F16), (name, dt, ran)
            assert I.expected_fwd(sh, dt, 1, {"igemm_deep": deep}) == (11 if dt == I.F16 else 2)
    run_rows(name, I.F16, False, [("fwd", 0, I.F16, 1, name)], igemm_deep=deep)


@pytest.mark.parametrize("pick", [4, 5, 6])
def test_deep_rings_promote_a_recorded_pick(pick):
    """4..6 -> 12..14: the heuristic never picks a 128-byte-stage configuration, a recorded pick does (honoured with "tune" 0).  The
    record is imported under the problem hash restated in `pick_key`, so the hash is checked on the device too: a wrong one would
    leave the heuristic's 2 (or 11) in igemm_last_cfg."""
    import struct
    name, dt, L = "c192", I.F16, lib()
    sh = I.SHAPES[name]["shape"]
    L.tune_import(struct.pack("<Qii", I.pick_key(I.fwd_args(sh, dt, 0), dt), 0, pick))
    try:
        rows = [("fwd", -1, dt, e, name) for e in (1, 0, 2, 6)]
        for deep, want in ((0, pick), (1, pick + 8), (2, pick + 8)):
            assert I.expected_fwd(sh, dt, 1, {"igemm_deep": deep, "pick": pick}) == want
            assert I.expected_fwd(sh, dt, 2, {"igemm_deep": deep, "pick": pick}) == pick          # the bias epilogue has no deep ring
            assert run_rows(name, dt, False, rows, igemm_deep=deep, pick=pick)[("fwd", -1)] == want
    finally:
        L.check(L.load().sy11_tune_clear(), "sy11_tune_clear")


@pytest.mark.parametrize("name", ["s2odd", "s2even"])
def test_stride2_input_gradient_fused_and_as_four_parity_launches(name):
    rows = [("dgrad", -1, I.F16, e, name) for e in (0, 8)]
    for sliced in (False, True):
        assert run_rows(name, I.F16, sliced, rows)[("dgrad", -1)] == I.HALO_DGRAD_S2
        assert run_rows(name, I.F16, sliced, rows, dgrad_s2_halo=0)[("dgrad", -1)] < I.IGEMM_NCFG


# ------------------------------------------------------------------------------------------------------------ fallbacks
@pytest.mark.parametrize("row", I.FALLBACK_ROWS, ids=I.row_id)
def test_forced_but_illegal_configuration_falls_back(row):
    op, cfg, dt, epi, name = row
    want = I.expected_cfg(row, cfg)
    assert want != cfg
    rows = [row] + ([("dgrad", cfg, dt, 8, name)] if op == "dgrad" else [])
    ran = run_rows(name, dt, False, rows)
    if op != "wgrad":
        assert ran[(op, cfg)] != cfg
    else:
        assert lib().get_option("wgrad_last_cfg") == want


# ------------------------------------------------------------------------------------------------------------ real family
def real_params():
    return [pytest.param(label, op, cfg, name, dt, id=f"{label.replace(' ', '_')}-{str(dt)[6:]}") for (label, op, cfg, name, dts) in I.REAL_KERNELS
            for dt in dts]


@pytest.mark.parametrize("label,op,cfg,name,dt", real_params())
def test_real_family(label, op, cfg, name, dt):
    """y, y + bias, sum, sumsq and dx through the forced forward / input-gradient configuration (where the rule says the input
    gradient takes it too; the heuristic otherwise), dw through the forced filter-gradient one."""
    rr = I.real(name, dt)
    t = Tensors(name, dt, rr, False)
    k, s, p, d = t.geo
    B, C, N, H, W = I.SHAPES[name]["shape"][:5]
    bias = rr["bias"].float().to(DEV)
    ratios = {}
    if op != "wgrad":
        fi = cfg
        o = Checked(name, dt, forced_igemm=fi)
        with options(igemm_cfg=fi):
            st = torch.zeros(2, N, device=DEV)
            o.conv2d_fwd(t.x.v, t.wk, t.y.v, k, s, p, d, 1, stats=(st[0], st[1]))
            ratios["y"] = R.worst_ratio(t.y.nchw(), rr["y"], rr["bound_y"])
            ratios["sum"] = R.worst_ratio(st[0].cpu(), rr["y"].sum((0, 2, 3)), rr["bound_sum"])
            ratios["sumsq"] = R.worst_ratio(st[1].cpu(), (rr["y"] * rr["y"]).sum((0, 2, 3)), rr["bound_sumsq"])
            yb = rr["y"] + rr["bias"].view(1, -1, 1, 1)
            o.conv2d_fwd(t.x.v, t.wk, t.y.v, k, s, p, d, 1, bias=bias)
            ratios["y+bias"] = R.worst_ratio(t.y.nchw(), yb, rr["bound_y_bias"])
            o.conv2d_fwd(t.x.v, t.wk, t.y.v, k, s, p, d, 1, bias=bias, silu=True)
            close_to_scale(t.y.nchw(), torch.nn.functional.silu(yb), dt, f"{label} bias + SiLU", mult=2)
            ran = o.conv2d_dgrad(t.dy.v, t.wt, t.dx.zero(), tuple(t.y.v.shape), k, s, p, d, 1, accumulate=False)
            ratios[f"dx[cfg {ran}]"] = R.worst_ratio(t.dx.nchw(), rr["dx"], rr["bound_dx"])
    fw = cfg if op == "wgrad" else -1
    o = Checked(name, dt, forced_wgrad=fw)
    with options(wgrad_cfg=fw):
        dw = torch.zeros(N, k, k, C, device=DEV)
        ran = o.conv2d_wgrad(t.x.v, t.dy.v, dw, k, s, p, d, 1)
        ratios[f"dw[cfg {ran}]"] = R.worst_ratio(dw.permute(0, 3, 1, 2).cpu(), rr["dw"], rr["bound_dw"])
    print(f"\nREAL {label} cfg {cfg} {name} {str(dt)[6:]} K={rr['K']} M={rr['M']}: worst err/bound " + " ".join(f"{n}={v:.3g}" for n, v in ratios.items()))
    for n, v in ratios.items():
        assert v <= 1.0, f"{label} {name} {dt}: {n} error is {v:.3f} x its bound"
