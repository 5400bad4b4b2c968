"""The six kernels of the first layer (csrc/direct.hip: stem_fwd_kernel, stem_fwd_mma, stem_fwd_tile, stem_wgrad_kernel,
stem_wgrad_mma, stem_wgrad_tile) against the float64 reference, with proof of which one ran: after every call "stem_fwd_last" /
"stem_wgrad_last" must equal the restated dispatch of tests/_stem_ref.py (`stem_branches`) BEFORE anything is compared, and the last
test requires the kernels observed in the session to be exactly those that tests/test_stem_ref_cpu.py promises.

Exact family (integer operands, results BIT-EQUAL to float64, both reduction modes): y into a view whose neighbouring channels hold
a sentinel, statistics of the RAW convolution (before bias and activation) into (N,) and (8, N) rows, y + integer bias, dw after one
and two accumulating calls; dense operands, y / dy in 16-byte-aligned slices and dy in a misaligned slice; every column shift of
the tiled kernels with 16-byte loads and with element-wise fill, one-tile and ragged maps, the gather MFMA kernels (stride 3,
IW = 3), the padding guard (padding >= 2 outside the tiling: forward on the general kernel), every N template of the gather
kernels, and two sparse rows past the persistent workgroup caps.
Real family: y, y + bias, sum, sumsq, dw under the order-independent elementwise bounds of `R.real_case`; SiLU with and without bias
against float64 under the bar of tests/_kernel_ref.py (8 e_ref + u s); worst err / bound printed (run with -s).
stem_conv_fwd_bn: mean / rstd / scale / shift / running statistics against `R.bn_tail_ref` from the exact sums, one row per
forward kernel (fused tail in the MFMA kernels, the separate finalize kernel after the gather kernel).

Worst err / bound of the real family, MI355X, when the tests were written (y / y + bias / dw, then SiLU / SiLU + bias as err / bar; sum
and sumsq stay below 2e-4): tiled with 16-byte loads f16 0.977 / 0.983 / 1.4e-4, 0.56 / 0.59, bf16 0.991 / 0.990 / 1.6e-4, 0.57 / 0.55;
tiled with element-wise fill f16 0.975 / 0.979 / 3.0e-4, 0.56 / 0.54, bf16 0.988 / 0.986 / 2.7e-4, 0.55 / 0.56; gather MFMA f16 0.981 /
0.971 / 5.6e-4, 0.57 / 0.55, bf16 0.994 / 0.990 / 3.0e-4, 0.57 / 0.56; gather f16 0.969 / 0.966 / 7.0e-4, 0.59 / 0.57, bf16 0.991 / 0.992 /
4.3e-4, 0.55 / 0.52, f32 0.029 / 0.035 / 7.0e-4, 0.10 / 0.09.  The 16-bit y figures are the rounding of the stored output (the u_out
term is exactly half an ulp).  Nothing is tuned to these figures: the bounds come from the operation counts and from the
reference's own f32 error.
"""
import pytest
import torch

from tests import _conv_ref as R
from tests import _kernel_ref as K
from tests import _stem_ref as S
from tests.test_conv_variants_gpu import DEV, SENTINEL, View, check_bn_tail, krsc, lib, ops, options, same

pytestmark = pytest.mark.gpu

OBSERVED = set()         # (op, code, dtype, N template) of every checked call of this session


class TailView(View):
    """`View` whose buffer is followed by 64 more SENTINEL elements: a read or write a few channels past the last pixel stays inside
    the allocation and meets the sentinel."""

    def __init__(self, B, H, W, C, dtype, ld, off, src=None):
        n = B * H * W * ld
        self.flat = torch.full((n + 64,), SENTINEL, dtype=dtype, device=DEV)
        self.buf = self.flat[:n].view(B, H, W, ld)
        self.v = self.buf[..., off:off + C]
        self.off, self.C = off, C
        if src is not None:
            self.v.copy_(src.permute(0, 2, 3, 1).to(DEV, dtype))

    def assert_neighbours_untouched(self, what):
        super().assert_neighbours_untouched(what)
        assert (self.flat[self.buf.numel():] == SENTINEL).all(), f"{what}: wrote past its last pixel"


class Stem:
    """The device operands of one row and the three entry points; after each call the kernel that ran must be the one the mirror names."""

    def __init__(self, row, r):
        d = S.row_dict(row)
        self.row, self.d, self.want = row, d, S.row_branches(row)
        B, N, H, W, dt = d["B"], d["N"], d["H"], d["W"], d["dtype"]
        OH, OW = S.out_hw(H, W, d["s"], d["p"])
        n = B * 3 * H * W
        lead = 1 if d["mode"] == "exact-xoff" else 0
        self.xbuf = torch.full((n + 8,), SENTINEL, dtype=torch.float32, device=DEV)
        self.x = self.xbuf[lead:lead + n].view(B, 3, H, W)
        self.x.copy_(r["x"].to(DEV, torch.float32))
        assert self.x.is_contiguous() and (self.x.data_ptr() % 16 == 0) == (lead == 0)
        self.y = TailView(B, OH, OW, N, dt, d["y_ld"], S.slice_offset(d["y_ld"], N))
        self.dy = TailView(B, OH, OW, N, dt, d["dy_ld"], S.slice_offset(d["dy_ld"], N), src=r["dy"])
        self.wk = krsc(r["w"], dt)
        self.what = S.row_id(row)

    def _note(self, op, option):
        got = lib().get_option(option)
        assert got == self.want[op], f"{self.what}: {option} = {got}, the mirror names {self.want[op]}"
        OBSERVED.add((op, got, self.d["dtype"], S.n_class(self.d["N"])))

    def fwd(self, bias=None, stats=None, silu=False):
        self.y.flat.fill_(SENTINEL)
        ops().stem_conv_fwd(self.x, self.wk, self.y.v, self.d["s"], self.d["p"], bias=bias, stats=stats, silu=silu)
        self._note("fwd", "stem_fwd_last")
        self.y.assert_neighbours_untouched(f"{self.what} y")
        return self.y.nchw()

    def fwd_bn(self, stats, bn):
        self.y.flat.fill_(SENTINEL)
        ops().stem_conv_fwd_bn(self.x, self.wk, self.y.v, self.d["s"], self.d["p"], stats, bn)
        self._note("fwd", "stem_fwd_last")
        return self.y.nchw()

    def wgrad(self, dw):
        ops().stem_conv_wgrad(self.x, self.dy.v, dw, self.d["s"], self.d["p"])
        self._note("wgrad", "stem_wgrad_last")
        return dw.permute(0, 3, 1, 2)

    def new_dw(self):
        """A zeroed [N][3][3][3] filter gradient at the head of a buffer whose tail (the rows a 64-wide template would own) holds SENTINEL."""
        n = self.d["N"] * 27
        self.dwbuf = torch.full((n + 64 * 27,), SENTINEL, dtype=torch.float32, device=DEV)
        dw = self.dwbuf[:n].view(self.d["N"], 3, 3, 3)
        return dw.zero_()

    def inputs_untouched(self):
        assert (self.dwbuf[self.d["N"] * 27:] == SENTINEL).all(), f"{self.what}: wrote past dw"
        n = self.x.numel()
        lead = self.x.data_ptr() // 4 - self.xbuf.data_ptr() // 4
        assert (self.xbuf[:lead] == SENTINEL).all() and (self.xbuf[lead + n:] == SENTINEL).all(), f"{self.what}: wrote next to x"
        self.dy.assert_neighbours_untouched(f"{self.what} dy")


@pytest.mark.parametrize("row", S.EXACT_ROWS, ids=S.row_id)
def test_exact(row):
    r = S.exact(row)
    t = Stem(row, r)
    N, slots = t.d["N"], t.d["slots"]
    ref_sum, ref_sq = r["y"].sum((0, 2, 3)), (r["y"] * r["y"]).sum((0, 2, 3))
    bias = r["bias"].float().to(DEV)
    for det in (1, 0):
        what = f"{t.what} deterministic={det}"
        with options(deterministic=det):
            for shape in ((N,), (slots, N)):
                st = torch.zeros((2,) + shape, device=DEV)
                same(t.fwd(stats=(st[0], st[1])), r["y"], f"{what} y (stats {shape})")
                tot = st.double().cpu().reshape(2, -1, N).sum(1)
                same(tot[0], ref_sum, f"{what} sum {shape}")
                same(tot[1], ref_sq, f"{what} sumsq {shape}")
            same(t.fwd(), r["y"], f"{what} y")
            if t.d["bias"]:
                st = torch.zeros(2, N, device=DEV)
                same(t.fwd(bias=bias, stats=(st[0], st[1])), r["y"] + r["bias"].view(1, -1, 1, 1), f"{what} y + bias")
                same(st[0], ref_sum, f"{what} sum beside a bias: statistics are of the raw convolution")
                same(st[1], ref_sq, f"{what} sumsq beside a bias")
            dw = t.new_dw()
            for n in (1, 2):
                same(t.wgrad(dw), n * r["dw"], f"{what} dw after call {n}")
            t.inputs_untouched()
    t.inputs_untouched()


@pytest.mark.parametrize("name", S.BN_ROWS)
@pytest.mark.parametrize("running", [True, False], ids=["running", "norunning"])
def test_fwd_bn(name, running):
    row = S.find_row(name)
    r = S.exact(row)
    t = Stem(row, r)
    N, count = t.d["N"], r["y"].shape[0] * r["y"].shape[2] * r["y"].shape[3]
    gen = torch.Generator().manual_seed(7)
    gamma, beta = (torch.rand(N, generator=gen) + 0.5).to(DEV), (torch.randn(N, generator=gen) * 0.1).to(DEV)
    rm0, rv0 = ((torch.randn(N, generator=gen) * 0.3).to(DEV), (torch.rand(N, generator=gen) + 0.5).to(DEV)) if running else (None, None)
    eps, mom = 1e-3, 0.03
    for det in (1, 0):
        for shape in ((N,), (8, N)):
            rm, rv = (rm0.clone(), rv0.clone()) if running else (None, None)
            st, v = torch.zeros((2,) + shape, device=DEV), torch.full((4, N), float("nan"), device=DEV)
            ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
            what = f"fwd_bn {t.what} deterministic={det} stats {shape}"
            with options(deterministic=det):
                y = t.fwd_bn((st[0], st[1]), (count, gamma, beta, eps, mom, rm, rv, v[0], v[1], v[2], v[3], ticket))
            same(y, r["y"], f"{what} y")
            check_bn_tail(v, rm, rv, st, ticket, r, slice(None), count, gamma, beta, eps, mom, rm0, rv0, what)


@pytest.mark.parametrize("row", S.REAL_ROWS, ids=S.row_id)
def test_real(row):
    rr = S.real(row)
    t = Stem(row, rr)
    d = t.d
    N, dt = d["N"], d["dtype"]
    bias = rr["bias"].float().to(DEV)
    ratios = {}
    st = torch.zeros(2, N, device=DEV)
    ratios["y"] = R.worst_ratio(t.fwd(stats=(st[0], st[1])), rr["y"], rr["bound_y"])
    ratios["sum"] = R.worst_ratio(st[0].cpu(), rr["y"].sum((0, 2, 3)), rr["bound_sum"])
    ratios["sumsq"] = R.worst_ratio(st[1].cpu(), (rr["y"] * rr["y"]).sum((0, 2, 3)), rr["bound_sumsq"])
    ratios["y+bias"] = R.worst_ratio(t.fwd(bias=bias), rr["y"] + rr["bias"].view(1, -1, 1, 1), rr["bound_y_bias"])
    dw = t.new_dw()
    ratios["dw"] = R.worst_ratio(t.wgrad(dw).cpu(), rr["dw"], rr["bound_dw"])
    code = S.row_branches(row)
    print(f"\nREAL {t.what} fwd {code['fwd']} wgrad {code['wgrad']} K={rr['K']} M={rr['M']}: worst err/bound " +
          " ".join(f"{n}={v:.3g}" for n, v in ratios.items()))
    bars = K.Bars(f"stem {t.what} fwd {code['fwd']}")
    for with_bias in (False, True):           # without a bias the tiled kernel still leaves its plain store path: SiLU alone does that
        r64, r32 = S.silu_refs(rr, d["s"], d["p"], with_bias)
        bars.add("silu + bias" if with_bias else "silu", t.fwd(bias=bias if with_bias else None, silu=True), r64, r32, out_dtype=dt)
    for n, v in ratios.items():
        assert v <= 1.0, f"{t.what}: {n} error is {v:.3f} x its bound"
    bars.check()
    t.inputs_untouched()


def test_every_promised_kernel_ran():
    """Needs the whole file: the (op, kernel, dtype, N template) combinations that the rows above really launched, read back from
    the library, are exactly those that the CPU test of the table promises."""
    want = S.promised()
    assert OBSERVED == want, f"never ran: {sorted(map(str, want - OBSERVED))}; unexpected: {sorted(map(str, OBSERVED - want))}"
