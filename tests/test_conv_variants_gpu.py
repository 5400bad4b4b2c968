"""Depthwise, grouped and off-diagonal dense convolutions against the float64 reference of tests/_conv_ref.py.

Exact family: integer operands, every device result BIT-EQUAL to float64, in f32 / f16 / bf16 and in both reduction modes
(ordered and atomic).  It carries the index, mask and tail checking: one wrong pixel, channel or tap changes an integer.
Real family: uniform operands, element-by-element error bounds that hold for any summation order; the worst err / bound
ratio of each test is printed (run with -s to see them).

Measured when the tests were written (worst err / bound over y, y + bias, dx, dw, sum, sumsq; f32 / f16 / bf16): depthwise
window 0.11 / 0.99 / 0.99, generic vec 0.13 / 0.99 / 0.99, scalar 0.09 / 0.94 / 0.97, grouped 0.02 / 0.91 / 0.98, dense
0.01 / 0.59 / 0.86.  The 16-bit figures are the rounding of the stored output (the u_out term is exactly half an ulp); sum,
sumsq and dw alone stay below 0.013.  Nothing is tuned to these figures: the bounds come from the operation counts.
"""
import contextlib

import pytest
import torch

from tests import _conv_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 77.0        # exact in every dtype; fills the channels next to a slice


def ops():
    from sy11 import ops as o
    return o


def lib():
    from sy11 import _lib
    return _lib


@contextlib.contextmanager
def options(**kw):
    """Set library options for the body and put the previous values back, whatever happens inside."""
    L = lib()
    old = {k: L.get_option(k) for k in kw}
    try:
        for k, v in kw.items():
            L.set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            L.set_option(k, v)


class View:
    """An NHWC device view of `C` channels at channel offset `off` of a [B][H][W][ld] buffer pre-filled with SENTINEL."""

    def __init__(self, B, H, W, C, dtype, ld=None, off=0, src=None):
        ld = C if ld is None else ld
        self.buf = torch.full((B, H, W, ld), SENTINEL, dtype=dtype, device=DEV)
        self.v = self.buf[..., off:off + C]
        self.off, self.C = off, C
        if src is not None:
            self.v.copy_(src.permute(0, 2, 3, 1).to(DEV, dtype))

    def zero(self):
        self.v.zero_()
        return self.v

    def nchw(self):
        return self.v.double().cpu().permute(0, 3, 1, 2)

    def assert_neighbours_untouched(self, what):
        left, right = self.buf[..., :self.off], self.buf[..., self.off + self.C:]
        assert (left == SENTINEL).all() and (right == SENTINEL).all(), f"{what}: wrote outside its channel slice"


def same(got, ref, what):
    """Bit-equality with the float64 reference (both hold integers, so == on float64 is equality of the stored bits)."""
    got = got.double().cpu() if got.is_cuda or got.dtype != torch.float64 else got
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    bad = got != ref
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {i}: got {got[i].item()} want {ref[i].item()}")


def krsc(w, dtype):
    """OIHW float64 -> the library's [N][KH][KW][C/g] filter on the device."""
    return w.permute(0, 2, 3, 1).contiguous().to(DEV, dtype)


def forward_and_stats(o, r, xv, wk, yv, geo, g, what):
    """y, 1-D statistics and [8][N] slotted statistics of one exact case."""
    k, s, p, d = geo
    N = r["y"].shape[1]
    ref_sum, ref_sq = r["y"].sum((0, 2, 3)), (r["y"] * r["y"]).sum((0, 2, 3))
    for shape in ((N,), (8, N)):
        st = torch.zeros((2,) + shape, device=DEV)
        yv.buf.fill_(SENTINEL)
        o.conv2d_fwd(xv.v, wk, yv.v, k, s, p, d, g, stats=(st[0], st[1]))
        same(yv.nchw(), r["y"], f"{what} y (stats {shape})")
        yv.assert_neighbours_untouched(f"{what} y")
        tot = st.double().cpu().reshape(2, -1, N).sum(1)
        same(tot[0], ref_sum, f"{what} sum {shape}")
        same(tot[1], ref_sq, f"{what} sumsq {shape}")


def input_gradient(o, r, dyv, w_dgrad, dxv, geo, g, what, plain_refused):
    k, s, p, d = geo
    y_shape = (r["y"].shape[0],) + tuple(r["y"].shape[2:]) + (r["y"].shape[1],)
    if plain_refused:
        with pytest.raises(lib().Sy11Error):
            o.conv2d_dgrad(dyv.v, w_dgrad, dxv.zero(), y_shape, k, s, p, d, g, accumulate=False)
    dxv.buf.fill_(SENTINEL)
    o.conv2d_dgrad(dyv.v, w_dgrad, dxv.zero(), y_shape, k, s, p, d, g, accumulate=plain_refused)
    same(dxv.nchw(), r["dx"], f"{what} dx")
    o.conv2d_dgrad(dyv.v, w_dgrad, dxv.v, y_shape, k, s, p, d, g, accumulate=True)
    same(dxv.nchw(), 2 * r["dx"], f"{what} dx accumulated onto itself")
    dxv.assert_neighbours_untouched(f"{what} dx")


def filter_gradient(o, r, xv, dyv, geo, g, what):
    k, s, p, d = geo
    N, cg, kh, kw = r["w"].shape
    dw = torch.zeros(N, kh, kw, cg, device=DEV)
    for n in (1, 2):
        o.conv2d_wgrad(xv.v, dyv.v, dw, k, s, p, d, g)
        same(dw.permute(0, 3, 1, 2), n * r["dw"], f"{what} dw after call {n}")


# ------------------------------------------------------------------------------------------------------------ depthwise
def run_depthwise_exact(dtype, case, ld_off=(None, 0)):
    o = ops()
    B, C, H, W, k, s, p, d = case
    r = R.exact_case(B, C, C, H, W, k, s, p, d, C)
    OH, OW = R.out_hw(H, W, k, s, p, d)
    ld, off = ld_off
    xv, dyv = View(B, H, W, C, dtype, ld, off, r["x"]), View(B, OH, OW, C, dtype, ld, off, r["dy"])
    yv, dxv = View(B, OH, OW, C, dtype, ld, off), View(B, H, W, C, dtype, ld, off)
    wk = krsc(r["w"], dtype)                                     # [C][kh][kw][1]: forward AND input gradient take this one
    esz = torch.empty((), dtype=dtype).element_size()
    label = R.dw_label(dtype, case, ld=ld, aligned=(off * esz) % 16 == 0)
    for det in (1, 0):
        what = f"depthwise {R.case_id(case)} {dtype} [{label}] deterministic={det}"
        with options(deterministic=det):
            forward_and_stats(o, r, xv, wk, yv, (k, s, p, d), C, what)
            input_gradient(o, r, dyv, wk, dxv, (k, s, p, d), C, what, plain_refused=False)
            filter_gradient(o, r, xv, dyv, (k, s, p, d), C, what)


def _dw_params():
    out = []
    for dt in R.DTYPES:
        out += [pytest.param(dt, c, id=f"{str(dt)[6:]}-{R.case_id(c)}") for c in R.dw_cases(dt)]
    return out


@pytest.mark.parametrize("dtype,case", _dw_params())
def test_depthwise_exact(dtype, case):
    run_depthwise_exact(dtype, case)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("ld_off", [(80, 8), (68, 2)], ids=["aligned_ld80", "misaligned_ld68"])
def test_depthwise_exact_on_channel_slices(ld_off, dtype):
    """x, y, dy, dx inside wider buffers: ld = C + 16 at a 16-byte-aligned offset keeps the window kernel (ld > C); ld = C + 4 at
    channel 2 is misaligned in every dtype and forces VEC = 1.  The neighbouring channels hold a sentinel and must keep it."""
    B, C, H, W = R.DW_SLICE_SHAPE
    esz = torch.empty((), dtype=dtype).element_size()
    want = "window0" if ld_off[0] == 80 else "scalar"
    assert R.dw_branches(dtype, C, H, W, 3, 1, 1, 1, ld=ld_off[0], aligned=(ld_off[1] * esz) % 16 == 0)["fwd"] == want
    run_depthwise_exact(dtype, (B, C, H, W, 3, 1, 1, 1), ld_off)


def check_bn_tail(v, rm, rv, st, ticket, r, ch, count, gamma, beta, eps, mom, rm0, rv0, what):
    """Statistics rows, mean / rstd / scale / shift, running statistics and tickets of channels `ch` after conv2d_fwd_bn."""
    N = st.shape[-1]
    tot = st.double().cpu().reshape(2, -1, N).sum(1)
    s1, s2 = r["y"].sum((0, 2, 3)), (r["y"] * r["y"]).sum((0, 2, 3))
    same(tot[0], s1, f"{what} sum")
    same(tot[1], s2, f"{what} sumsq")
    ref = R.bn_tail_ref(s1.numpy(), s2.numpy(), count, gamma.cpu().numpy(), beta.cpu().numpy(), eps, mom,
                        None if rm0 is None else rm0.cpu().numpy(), None if rm0 is None else rv0.cpu().numpy())
    got = {"mean": v[0], "rstd": v[1], "scale": v[2], "shift": v[3]}
    if rm0 is not None:
        got.update(running_mean=rm, running_var=rv)
    assert set(got) == set(ref)
    for name, t in got.items():
        want, tol = ref[name]
        err = (t.double().cpu() - torch.from_numpy(want)).abs()[ch]
        assert (err <= torch.from_numpy(tol)[ch]).all(), f"{what} {name}: worst error {err.max().item():.3e} (allowed {tol[ch].max():.3e})"
    assert int(ticket.abs().sum()) == 0, f"{what}: tickets not returned at zero"


def run_fwd_bn(dtype, case10, running, what):
    o = ops()
    B, C, N, H, W, k, s, p, d, g = case10
    r = R.exact_case(*case10)
    OH, OW = R.out_hw(H, W, k, s, p, d)
    xv, yv = View(B, H, W, C, dtype, src=r["x"]), View(B, OH, OW, N, dtype)
    wk = krsc(r["w"], dtype)
    gen = torch.Generator().manual_seed(7)
    gamma, beta = (torch.rand(N, generator=gen) + 0.5).to(DEV), (torch.randn(N, generator=gen) * 0.1).to(DEV)
    rm0, rv0 = ((torch.randn(N, generator=gen) * 0.3).to(DEV), (torch.rand(N, generator=gen) + 0.5).to(DEV)) if running else (None, None)
    rm, rv = (rm0.clone(), rv0.clone()) if running else (None, None)
    eps, mom, count = 1e-3, 0.03, B * OH * OW
    st, v = torch.zeros(2, 8, N, device=DEV), torch.full((4, N), float("nan"), device=DEV)
    ntick = g if 1 < g < C else 1
    ticket = torch.zeros(ntick, dtype=torch.int32, device=DEV)
    o.conv2d_fwd_bn(xv.v, wk, yv.v, k, s, p, d, g, (st[0], st[1]), (count, gamma, beta, eps, mom, rm, rv, v[0], v[1], v[2], v[3], ticket))
    same(yv.nchw(), r["y"], f"{what} y")
    check_bn_tail(v, rm, rv, st, ticket, r, slice(None), count, gamma, beta, eps, mom, rm0, rv0, what)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("running", [True, False], ids=["running", "norunning"])
@pytest.mark.parametrize("shape", [(3, 64, 9, 20), (2, 24, 7, 5)], ids=["C64_tail_in_kernel", "C24_separate_finalize"])
def test_depthwise_fwd_bn(shape, running, dtype):
    B, C, H, W = shape
    label = R.dw_label(dtype, shape + (3, 1, 1, 1))
    run_fwd_bn(dtype, (B, C, C, H, W, 3, 1, 1, 1, C), running, f"depthwise fwd_bn {shape} {dtype} [{label}]")


# ------------------------------------------------------------------------------------------------------------ grouped / dense
def run_mfma_exact(dtype, case10, what, dets=(1, 0), fwd=True, wgrad=True):
    o = ops()
    B, C, N, H, W, k, s, p, d, g = case10
    r = R.exact_case(*case10)
    OH, OW = R.out_hw(H, W, k, s, p, d)
    xv, dyv = View(B, H, W, C, dtype, src=r["x"]), View(B, OH, OW, N, dtype, src=r["dy"])
    yv, dxv = View(B, OH, OW, N, dtype), View(B, H, W, C, dtype)
    wk = krsc(r["w"], dtype)
    wt = o.weight_transpose(wk, groups=g) if g > 1 else o.weight_transpose(wk)
    ng = N // g
    per_group = torch.stack([wk[i * ng:(i + 1) * ng].permute(3, 1, 2, 0) for i in range(g)])      # [g][C/g][kh][kw][N/g]
    assert torch.equal(wt.reshape(per_group.shape), per_group), f"{what}: weight_transpose"
    holes = R.dgrad_has_holes(k, s, p, d)
    for det in dets:
        w2 = f"{what} deterministic={det}"
        with options(deterministic=det):
            if fwd:
                forward_and_stats(o, r, xv, wk, yv, (k, s, p, d), g, w2)
                input_gradient(o, r, dyv, wt, dxv, (k, s, p, d), g, w2, plain_refused=holes)
            if wgrad:
                filter_gradient(o, r, xv, dyv, (k, s, p, d), g, w2)


def _grouped_params():
    out = []
    for dt in R.DTYPES:
        out += [pytest.param(dt, c, id=f"{str(dt)[6:]}-{R.case_id(c)}") for c in R.grouped_cases(dt)]
    return out


@pytest.mark.parametrize("dtype,case", _grouped_params())
def test_grouped_exact(dtype, case):
    """Per-group pointer offsets of x / y / dy / dx, the filter blocks, the statistics at g * N/g and the dw blocks; the two
    stride-2 / dilation-2 cases have input parity classes without a tap: plain dgrad must refuse, accumulate into zeros is exact."""
    run_mfma_exact(dtype, case, f"grouped {R.case_id(case)} {dtype}")


@pytest.mark.parametrize("dtype,case", _grouped_params())
@pytest.mark.parametrize("running", [True, False], ids=["running", "norunning"])
def test_grouped_fwd_bn(running, dtype, case):
    """One ticket and one channel block of gamma / beta / mean / rstd / scale / shift / running statistics per group."""
    run_fwd_bn(dtype, case, running, f"grouped fwd_bn {R.case_id(case)} {dtype}")


@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("case", R.DENSE_CASES, ids=R.case_id)
def test_dense_tap_table_exact(case, dtype):
    run_mfma_exact(dtype, case + (1,), f"dense {R.case_id(case)} {dtype}")


@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("case", R.DILATED_SPECIAL_CASES, ids=R.case_id)
def test_special_kernels_refuse_dilated_taps(case, dtype):
    """Shapes the halo / few-channel / patch kernels would take, but with dilation 2: forcing their configurations must fall
    back to a kernel that reads the tap table, and the result stays exact."""
    what = f"dilated {R.case_id(case)} {dtype}"
    with options(tune=0, igemm_cfg=-1, wgrad_cfg=-1):
        for cfg in R.FORCED_IGEMM_CFGS:
            lib().set_option("igemm_cfg", cfg)
            run_mfma_exact(dtype, case + (1,), f"{what} igemm_cfg={cfg}", dets=(1,), wgrad=False)
        lib().set_option("igemm_cfg", -1)
        for cfg in R.FORCED_WGRAD_CFGS:
            lib().set_option("wgrad_cfg", cfg)
            run_mfma_exact(dtype, case + (1,), f"{what} wgrad_cfg={cfg}", dets=(1,), fwd=False)


# ------------------------------------------------------------------------------------------------------------ refusals
def _small_valid_call(dtype=torch.float16):
    run_depthwise_exact(dtype, (2, 8, 7, 7, 3, 1, 1, 1))


def test_refusals_raise_and_leave_the_library_usable():
    o, E = ops(), lib().Sy11Error
    f16 = torch.float16
    x = View(2, 7, 7, 8, f16, src=torch.ones(2, 8, 7, 7))
    # depthwise with an f32 output
    with pytest.raises(E):
        o.conv2d_fwd(x.v, torch.ones(8, 3, 3, 1, dtype=f16, device=DEV), torch.zeros(2, 7, 7, 8, device=DEV), 3, 1, 1, 1, 8, out_f32=True)
    _small_valid_call()
    # depthwise 5x5: 25 taps, forward / input gradient / filter gradient
    w5 = torch.ones(8, 5, 5, 1, dtype=f16, device=DEV)
    y = View(2, 7, 7, 8, f16)
    with pytest.raises(E):
        o.conv2d_fwd(x.v, w5, y.v, 5, 1, 2, 1, 8)
    with pytest.raises(E):
        o.conv2d_dgrad(x.v, w5, y.v, (2, 7, 7, 8), 5, 1, 2, 1, 8)
    with pytest.raises(E):
        o.conv2d_wgrad(x.v, x.v, torch.zeros(8, 5, 5, 1, device=DEV), 5, 1, 2, 1, 8)
    _small_valid_call()
    # groups = C with N = 2C in f16: one channel per group is not a 16-byte vector
    with pytest.raises(E):
        o.conv2d_fwd(x.v, torch.ones(16, 3, 3, 1, dtype=f16, device=DEV), View(2, 7, 7, 16, f16).v, 3, 1, 1, 1, 8)
    _small_valid_call()
    # a tap offset d * (k - 1) = 120 does not fit the int8 tap table with its margin: 1x3 filter, dilation 60
    xw, yw = View(1, 2, 122, 8, f16, src=torch.ones(1, 8, 2, 122)), View(1, 2, 2, 8, f16, src=torch.ones(1, 8, 2, 2))
    assert R.out_hw(2, 122, (1, 3), 1, 0, 60) == (2, 2)
    w13 = torch.ones(8, 1, 3, 8, dtype=f16, device=DEV)
    with pytest.raises(E):
        o.conv2d_fwd(xw.v, w13, yw.v, (1, 3), 1, 0, 60)
    with pytest.raises(E):
        o.conv2d_dgrad(yw.v, w13, xw.v, (1, 2, 2, 8), (1, 3), 1, 0, 60)
    with pytest.raises(E):
        o.conv2d_wgrad(xw.v, yw.v, torch.zeros(8, 1, 3, 8, device=DEV), (1, 3), 1, 0, 60)
    _small_valid_call()
    run_mfma_exact(f16, (2, 32, 32, 9, 12, (1, 3), 1, 1, 1, 1), "dense after the refusals", dets=(1,))


# ------------------------------------------------------------------------------------------------------------ real-valued family
def close_to_scale(got, ref, dtype, what, mult):
    """The project's bar for an epilogue with a transcendental: tests/test_kernels_gpu.py `close`."""
    scale = max(ref.abs().max().item(), 1e-6)
    err = (got.double() - ref).abs().max().item()
    assert err <= R.TOL_SCALE[dtype] * mult * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e} ({dtype})"


def run_real(dtype, case10, family):
    o = ops()
    B, C, N, H, W, k, s, p, d, g = case10
    r = R.real_case(*case10, dtype=dtype)
    OH, OW = R.out_hw(H, W, k, s, p, d)
    depthwise = g == C and C == N
    xv, dyv = View(B, H, W, C, dtype, src=r["x"]), View(B, OH, OW, N, dtype, src=r["dy"])
    yv, dxv = View(B, OH, OW, N, dtype), View(B, H, W, C, dtype)
    wk = krsc(r["w"], dtype)
    bias = r["bias"].float().to(DEV)
    ratios = {}
    st = torch.zeros(2, N, device=DEV)
    o.conv2d_fwd(xv.v, wk, yv.v, k, s, p, d, g, stats=(st[0], st[1]))
    ratios["y"] = R.worst_ratio(yv.nchw(), r["y"], r["bound_y"])
    ratios["sum"] = R.worst_ratio(st[0].cpu(), r["y"].sum((0, 2, 3)), r["bound_sum"])
    ratios["sumsq"] = R.worst_ratio(st[1].cpu(), (r["y"] * r["y"]).sum((0, 2, 3)), r["bound_sumsq"])
    o.conv2d_fwd(xv.v, wk, yv.v, k, s, p, d, g, bias=bias)
    yb = r["y"] + r["bias"].view(1, -1, 1, 1)
    ratios["y+bias"] = R.worst_ratio(yv.nchw(), yb, r["bound_y_bias"])
    o.conv2d_fwd(xv.v, wk, yv.v, k, s, p, d, g, bias=bias, silu=True)
    y_silu = yv.nchw()
    y_shape = (B, OH, OW, N)
    w_dgrad = wk if depthwise else (o.weight_transpose(wk, groups=g) if g > 1 else o.weight_transpose(wk))
    o.conv2d_dgrad(dyv.v, w_dgrad, dxv.zero(), y_shape, k, s, p, d, g, accumulate=(not depthwise) and R.dgrad_has_holes(k, s, p, d))
    ratios["dx"] = R.worst_ratio(dxv.nchw(), r["dx"], r["bound_dx"])
    dw = torch.zeros(N, *wk.shape[1:], device=DEV)
    o.conv2d_wgrad(xv.v, dyv.v, dw, k, s, p, d, g)
    ratios["dw"] = R.worst_ratio(dw.permute(0, 3, 1, 2).cpu(), r["dw"], r["bound_dw"])
    print(f"\nREAL {family} {R.case_id(case10)} {str(dtype)[6:]} K={r['K']} M={r['M']}: worst err/bound " +
          " ".join(f"{n}={v:.3f}" for n, v in ratios.items()))
    for n, v in ratios.items():
        assert v <= 1.0, f"{family} {R.case_id(case10)} {dtype}: {n} error is {v:.3f} x its bound"
    close_to_scale(y_silu, torch.nn.functional.silu(yb), dtype, f"{family} bias + SiLU", mult=2)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("case", R.REAL_DW_CASES, ids=R.case_id)
def test_depthwise_real(case, dtype):
    B, C, H, W, k, s, p, d = case
    b = R.dw_branches(dtype, C, H, W, k, s, p, d)
    run_real(dtype, (B, C, C, H, W, k, s, p, d, C), f"depthwise[{b['fwd']}/{b['dgrad']}/{b['wgrad']}]")


@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("case", R.REAL_GROUPED_CASES, ids=R.case_id)
def test_grouped_real(case, dtype):
    run_real(dtype, case, "grouped")


@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("case", R.REAL_DENSE_CASES, ids=R.case_id)
def test_dense_real(case, dtype):
    run_real(dtype, case + (1,), "dense")
