"""GPU: every entry of csrc/fusion.hip on its own against a float64 CPU reference (tests/_kernel_ref.py holds the bar), in the
ordered and in the atomic reduction mode, at every legal lane width, on contiguous inputs and on channel slices of wider buffers.

References: the formulas of the header comment of fusion.hip, written in plain torch, with autograd for every backward quantity;
the gate formula and the composed chain are tied to oracle/yolo11_ref.py (`gct`, `fusion_eschannel`).  Exact quantities (channel
max, argmax, untouched memory) are compared for equality.

Measured bars (MI355X) are tabulated in DESIGN.md section 5, "kernel-level parity, measured".
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import yolo11_ref as R
from tests._kernel_ref import DEV, Bars, lib, nhwc_view, ops, outside_untouched, reduction_mode, rnd, rounded, same_bits, sum_bound  # noqa: F401

pytestmark = pytest.mark.gpu

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
SHAPES = [(1, 1, 1), (2, 3, 5), (3, 20, 20), (2, 37, 41), (2, 80, 80), (1, 130, 130)]     # 130^2 > 512 * 4 * 8: the gx = 512 cap at LP = 64
LANES = [(F32, c) for c in (4, 8, 16, 32, 64, 128, 256)] + [(d, c) for d in (F16, BF16) for c in (8, 16, 64, 128, 512)]
LANE_IDS = [f"{str(d)[6:]}-C{c}" for d, c in LANES]
SHAPE_IDS = ["x".join(map(str, s)) for s in SHAPES]
EPS = 1e-5


def _depth(HW, Cn, dtype):
    """Additions a term of fusion_stats' sq / fusion_bwd_reduce's dG passes through at most: a lane group owns every ppb-th pixel
    (all of them when one workgroup owns the image: ordered mode), then the ppb parked rows, then the add into the output."""
    ppb = 256 // (Cn // (16 // torch.empty((), dtype=dtype).element_size()))
    return -(-HW // ppb) + ppb + 1


def _sq_slice(B, Cn, n=3, i=1, init=0.0):
    buf = torch.full((B, n * Cn), init, dtype=F32, device=DEV)
    return buf, buf[:, i * Cn:(i + 1) * Cn]


# ------------------------------------------------------------------------------------------------ fusion_stats
def _stats_ref(x, dt):
    xd = x.to(dt)
    return xd.mean(-1), (xd * xd).sum((1, 2))


def _run_stats(x_cpu, dtype, strided, calls=1):
    B, H, W, Cn = x_cpu.shape
    xv, xbuf = nhwc_view(x_cpu, dtype, strided)
    mm = torch.full((B, H, W, 2), -7.0, dtype=F32, device=DEV)
    am = torch.full((B, H, W), -1, dtype=torch.int16, device=DEV)
    sqbuf, sq = _sq_slice(B, Cn)
    for _ in range(calls):
        ops().fusion_stats(xv, mm, am, sq)
    torch.cuda.synchronize()
    assert outside_untouched(xbuf, Cn)
    assert float(sqbuf[:, :Cn].abs().max()) == 0.0 and float(sqbuf[:, 2 * Cn:].abs().max()) == 0.0, "sq written outside its column slice"
    return mm.cpu(), am.cpu().to(torch.int32) & 0xFFFF, sq.cpu()


@pytest.mark.parametrize("strided", [False, True], ids=["contig", "slice"])
@pytest.mark.parametrize("lane", LANES, ids=LANE_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_fusion_stats(reduction_mode, shape, lane, strided):
    dtype, Cn = lane
    B, H, W = shape
    x = rounded(rnd(B, H, W, Cn, seed=11 + Cn + H), dtype)
    mx, ai = x.max(-1)
    assert np.array_equal(ai.numpy(), np.argmax(x.numpy(), -1)), "the CPU reference's tie rule is not 'first index'"
    mm, am, sq = _run_stats(x, dtype, strided, calls=2)
    assert same_bits(mm[..., 1], mx), "channel max is not bit-exact"
    assert torch.equal(am, ai.to(torch.int32)), f"argmax differs at {int((am != ai).sum())} pixels"
    b = Bars(f"fusion_stats[{reduction_mode}]")
    (m64, s64), (m32, s32) = _stats_ref(x, torch.float64), _stats_ref(x, F32)
    b.add("mean", mm[..., 0], m64, m32)
    # measured at 1x130x130 C256 f32, ordered: 64 x e_ref (4225 sequential adds per accumulator against torch's cascade)
    b.add("sq(2 calls)", sq, 2 * s64, 2 * s32, extra=sum_bound(_depth(H * W, Cn, dtype) + 1, 2 * s64.max()))
    b.check()


@pytest.mark.parametrize("lane", [(F32, 16), (F32, 128), (F32, 256), (F16, 128), (BF16, 512)], ids=["f32-C16", "f32-C128", "f32-C256", "f16-C128", "bf16-C512"])
def test_fusion_stats_ties_first_index_wins(reduction_mode, lane):
    """Values from 7 levels: the channel maximum is shared by several channels in most pixels, inside one lane's vector and
    across the lanes of the LP-wide shuffle.  The first index has to win, as in torch.max on the CPU."""
    dtype, Cn = lane
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-3, 4, (2, 37, 41, Cn), generator=g).float() / 4
    mx, ai = x.max(-1)
    tied = ((x == mx[..., None]).sum(-1) > 1).float().mean().item()
    assert tied >= 0.5, f"only {tied:.2f} of the pixels have a tied maximum: the case would be vacuous"
    assert np.array_equal(ai.numpy(), np.argmax(x.numpy(), -1))
    mm, am, sq = _run_stats(x, dtype, strided=True)
    assert same_bits(mm[..., 1], mx)
    assert torch.equal(am, ai.to(torch.int32)), f"argmax differs at {int((am != ai).sum())} of {ai.numel()} pixels"
    b = Bars(f"fusion_stats.ties[{reduction_mode}]")
    (m64, s64), (m32, s32) = _stats_ref(x, torch.float64), _stats_ref(x, F32)
    b.add("mean", mm[..., 0], m64, m32)
    b.add("sq", sq, s64, s32, extra=sum_bound(_depth(37 * 41, Cn, dtype), s64.max()))
    b.check()


# ------------------------------------------------------------------------------------------------ SAB map
SAB_SHAPES = SHAPES + [(2, 1, 7), (2, 9, 1), (1, 16, 16), (5, 2, 2)]


def _ring(B, H, W):
    m = torch.zeros(B, H, W, dtype=torch.bool)
    m[:, 0], m[:, -1], m[:, :, 0], m[:, :, -1] = True, True, True, True
    return m


def _sab_ref(mm, w, dS, dw0, dt):
    mm_, w_ = mm.to(dt).clone().requires_grad_(True), w.to(dt).clone().requires_grad_(True)
    S = torch.sigmoid(F.conv2d(mm_.permute(0, 3, 1, 2), w_, None, 1, 1))[:, 0]
    dmm, dw = torch.autograd.grad((S * dS.to(dt)).sum(), (mm_, w_))
    return S.detach(), dmm, dw0.to(dt) + dw.permute(0, 2, 3, 1).reshape(-1)


@pytest.mark.parametrize("shape", SAB_SHAPES, ids=["x".join(map(str, s)) for s in SAB_SHAPES])
def test_sab_map_fwd_bwd(reduction_mode, shape):
    B, H, W = shape
    mm, w, dS, dw0 = rnd(B, H, W, 2, seed=1, scale=2.0), rnd(1, 2, 3, 3, seed=2, scale=0.7), rnd(B, H, W, seed=3), rnd(18, seed=4, scale=3.0)
    o = ops()
    w18 = o.filter_krsc(w.to(DEV)).reshape(-1).contiguous()
    mm_d, S = mm.to(DEV), torch.full((B, H, W), -7.0, dtype=F32, device=DEV)
    o.sab_map_fwd(mm_d, w18, S)
    dmm, dw = torch.full((B, H, W, 2), -7.0, dtype=F32, device=DEV), dw0.to(DEV)
    o.sab_map_bwd(dS.to(DEV), S, mm_d, w18, dmm, dw)
    torch.cuda.synchronize()
    S64, dmm64, dw64 = _sab_ref(mm, w, dS, dw0, torch.float64)
    S32, dmm32, dw32 = _sab_ref(mm, w, dS, dw0, F32)
    ring = _ring(B, H, W)
    b = Bars(f"sab_map[{reduction_mode}] {B}x{H}x{W}")
    b.add("S", S, S64, S32)
    b.add("S.border", S.cpu()[ring], S64[ring], S32[ring])          # a tap that crosses a row or image boundary shows up here
    b.add("dmm", dmm, dmm64, dmm32)
    b.add("dmm.border", dmm.cpu()[ring], dmm64[ring], dmm32[ring])
    if (~ring).any():
        b.add("dmm.interior", dmm.cpu()[~ring], dmm64[~ring], dmm32[~ring])
    b.add("dw(+dw0)", dw, dw64, dw32)
    b.check()


# ------------------------------------------------------------------------------------------------ GCT gate
def _gate(sq, alpha, gamma, beta, eps=EPS):
    """The gate of fusion.hip's header comment as a function of sq = sum_hw a^2."""
    e = (sq + eps).sqrt() * alpha
    return 1.0 + torch.tanh(e * (gamma / (e.pow(2).mean(1, keepdim=True) + eps).sqrt()) + beta)


def _gct_ref(sq, alpha, gamma, beta, dG, acc, dt):
    v = [t.to(dt).clone().requires_grad_(True) for t in (sq, alpha, gamma, beta)]
    G = _gate(*v)
    dsq, da, dg, db = torch.autograd.grad((G * dG.to(dt)).sum(), v)
    return G.detach(), 2.0 * dsq, acc[0].to(dt) + da, acc[1].to(dt) + dg, acc[2].to(dt) + db        # dx = x * q  <=>  q = 2 dL/dsq


def test_gate_formula_is_the_oracles_gct():
    """CPU part: _gate(sum_hw x^2) * x is oracle.yolo11_ref.gct(x) in float64."""
    x = rnd(3, 24, 5, 4, seed=1).double()
    a, g, bt = (rnd(1, 24, 1, 1, seed=s).double() + o for s, o in ((2, 1.0), (3, 0.0), (4, 0.0)))
    got = x * _gate(x.pow(2).sum((2, 3)), a.view(1, -1), g.view(1, -1), bt.view(1, -1)).view(3, 24, 1, 1)
    ref = R.gct({"p.alpha": a, "p.gamma": g, "p.beta": bt}, "p.", x, eps=EPS)
    assert (got - ref).abs().max().item() <= 1e-13 * ref.abs().max().item()


@pytest.mark.parametrize("zero_channels", [False, True], ids=["sq>0", "sq=0"])
@pytest.mark.parametrize("B", [1, 2, 7])
@pytest.mark.parametrize("Ct", [8, 255, 256, 257, 384, 1536])
def test_gct_gate_fwd_bwd(reduction_mode, Ct, B, zero_channels):
    """``sq=0``: every 5th channel of every image is all-zero, root = sqrt(eps), q = de * alpha / root is ~300 x the others."""
    sq = (rnd(B, Ct, seed=1).abs() + 0.05) * 400.0
    if zero_channels:
        sq[:, ::5] = 0.0
    alpha, gamma, beta = 1.0 + rnd(1, Ct, seed=2, scale=0.3), rnd(1, Ct, seed=3, scale=0.6), rnd(1, Ct, seed=4, scale=0.4)
    dG = rnd(B, Ct, seed=5)
    acc = [rnd(1, Ct, seed=6 + i, scale=2.0) for i in range(3)]
    o = ops()
    d = lambda t: t.reshape(-1).contiguous().to(DEV)                   # noqa: E731
    sq_d, a_d, g_d, b_d = sq.to(DEV), d(alpha), d(gamma), d(beta)
    G, q = torch.full((B, Ct), -7.0, dtype=F32, device=DEV), torch.full((B, Ct), -7.0, dtype=F32, device=DEV)
    da, dg, db = (d(t) for t in acc)
    o.gct_gate_fwd(sq_d, a_d, g_d, b_d, EPS, G)
    o.gct_gate_bwd(sq_d, a_d, g_d, b_d, EPS, dG.to(DEV), q, da, dg, db)
    torch.cuda.synchronize()
    r64, r32 = _gct_ref(sq, alpha, gamma, beta, dG, acc, torch.float64), _gct_ref(sq, alpha, gamma, beta, dG, acc, F32)
    b = Bars(f"gct_gate[{reduction_mode}] B{B} Ct{Ct} {'sq=0' if zero_channels else ''}")
    for name, got, i in (("G", G, 0), ("q", q, 1), ("dalpha", da.view(1, -1), 2), ("dgamma", dg.view(1, -1), 3), ("dbeta", db.view(1, -1), 4)):
        b.add(name, got, r64[i], r32[i])
    b.check()


# ------------------------------------------------------------------------------------------------ combine / reduce / apply, G and S free
def _xs(n, B, H, W, Cn, dtype, seed):
    return [rounded(rnd(B, H, W, Cn, seed=seed + i), dtype) for i in range(n)]


def _combine_ref(xs, G, Ss, dt):
    Cn = xs[0].shape[-1]
    return sum(x.to(dt) * (G.to(dt)[:, None, None, i * Cn:(i + 1) * Cn] + S.to(dt)[..., None]) for i, (x, S) in enumerate(zip(xs, Ss)))


CRA_CASES = [(2, (2, 3, 5), F32, 4), (3, (3, 20, 20), F32, 64), (2, (2, 37, 41), F32, 256), (3, (2, 37, 41), F16, 128), (2, (1, 1, 1), BF16, 8),
             (3, (2, 80, 80), BF16, 512), (2, (2, 80, 80), F16, 16), (3, (1, 130, 130), F32, 256), (3, (2, 37, 41), F32, 32)]


@pytest.mark.parametrize("strided", [False, True], ids=["contig", "slice"])
@pytest.mark.parametrize("case", CRA_CASES, ids=[f"n{n}-{'x'.join(map(str, s))}-{str(d)[6:]}-C{c}" for n, s, d, c in CRA_CASES])
def test_fusion_combine_reduce_apply(reduction_mode, case, strided):
    """out, dG (accumulated into a non-zero slice), dS, and dx (plain, and accumulated into a non-zero dx) with G, S, q, dmm and
    the argmax as FREE inputs: autograd of  sum(out * dout) + sum(q / 2 * x^2) + sum(dmm0 * mean_c x) + sum(dmm1 * x[argmax])."""
    n, (B, H, W), dtype, Cn = case
    o = ops()
    xs = _xs(n, B, H, W, Cn, dtype, seed=20)
    G, q = 1.0 + rnd(B, n * Cn, seed=30, scale=0.9), rnd(B, n * Cn, seed=31, scale=0.5)
    Ss = [rnd(B, H, W, seed=40 + i).abs() for i in range(n)]
    dout = rounded(rnd(B, H, W, Cn, seed=50), dtype)
    dmm = [rnd(B, H, W, 2, seed=60 + i) for i in range(n)]
    g = torch.Generator().manual_seed(70)
    am = [torch.randint(0, Cn, (B, H, W), generator=g) for _ in range(n)]
    dG0 = rnd(B, n * Cn, seed=80, scale=5.0)
    dx0 = [rounded(rnd(B, H, W, Cn, seed=90 + i, scale=2.0), dtype) for i in range(n)]

    xv = [nhwc_view(x, dtype, strided) for x in xs]
    dov, dobuf = nhwc_view(dout, dtype, strided)
    S_d = [S.to(DEV) for S in Ss]
    G_d, q_d = G.to(DEV), q.to(DEV)
    out, outbuf = nhwc_view(torch.zeros(B, H, W, Cn), dtype, strided)
    o.fusion_combine([v for v, _ in xv], S_d, G_d, out)
    dG_d = dG0.to(DEV)
    dS = [torch.full((B, H, W), -7.0, dtype=F32, device=DEV) for _ in range(n)]
    dx, dxa = [], []
    for i in range(n):
        o.fusion_bwd_reduce(dov, xv[i][0], dG_d[:, i * Cn:(i + 1) * Cn], dS[i])
    for i in range(n):
        am_d = am[i].to(torch.int16).to(DEV)
        sl = slice(i * Cn, (i + 1) * Cn)
        a, abuf = nhwc_view(torch.zeros(B, H, W, Cn), dtype, strided)
        o.fusion_bwd_apply(dov, xv[i][0], G_d[:, sl], q_d[:, sl], S_d[i], dmm[i].to(DEV), am_d, a, False)
        c, cbuf = nhwc_view(dx0[i], dtype, strided)
        o.fusion_bwd_apply(dov, xv[i][0], G_d[:, sl], q_d[:, sl], S_d[i], dmm[i].to(DEV), am_d, c, True)
        dx.append((a, abuf))
        dxa.append((c, cbuf))
    torch.cuda.synchronize()
    for _, buf in xv + [(None, dobuf), (None, outbuf)] + dx + dxa:
        assert outside_untouched(buf, Cn), "a kernel wrote outside its channel slice"

    def ref(dt):
        x_ = [x.to(dt).clone().requires_grad_(True) for x in xs]
        G_ = G.to(dt).clone().requires_grad_(True)
        S_ = [S.to(dt).clone().requires_grad_(True) for S in Ss]
        y = _combine_ref(x_, G_, S_, dt)
        loss = (y * dout.to(dt)).sum()
        for i in range(n):
            loss = loss + (q.to(dt)[:, None, None, i * Cn:(i + 1) * Cn] / 2 * x_[i] ** 2).sum() + (dmm[i][..., 0].to(dt) * x_[i].mean(-1)).sum() \
                + (dmm[i][..., 1].to(dt) * x_[i].gather(-1, am[i][..., None])[..., 0]).sum()
        gr = torch.autograd.grad(loss, [G_] + S_ + x_)
        return y.detach(), dG0.to(dt) + gr[0], gr[1:1 + n], gr[1 + n:]

    r64, r32 = ref(torch.float64), ref(F32)
    b = Bars(f"fusion c/r/a[{reduction_mode}] n{n} {B}x{H}x{W}x{Cn} {dtype}")
    b.add("out", out.float(), r64[0], r32[0], dtype)
    absG = torch.cat([(x.double() * dout.double()).abs().sum((1, 2)) for x in xs], 1).max() + dG0.abs().max()
    b.add("dG(+dG0)", dG_d, r64[1], r32[1], extra=sum_bound(_depth(H * W, Cn, dtype), absG))
    for i in range(n):
        b.add(f"dS{i}", dS[i], r64[2][i], r32[2][i])
        b.add(f"dx{i}", dx[i][0].float(), r64[3][i], r32[3][i], dtype)
        b.add(f"dx{i}(+dx0)", dxa[i][0].float(), dx0[i].double() + r64[3][i], dx0[i] + r32[3][i], dtype)
    b.check()


# ------------------------------------------------------------------------------------------------ the composed chain
def _chain_gpu(xs_v, w, alpha, gamma, beta, dout_v, dtype, acc_into):
    """The launches of Fusion._run and of its backward closure (nn/modules/conv.py), in their order."""
    o = ops()
    n = len(xs_v)
    B, H, W, Cn = xs_v[0].shape
    f32 = dict(dtype=F32, device=DEV)
    sq = torch.zeros((B, n * Cn), **f32)
    mm = [torch.empty((B, H, W, 2), **f32) for _ in range(n)]
    am = [torch.empty((B, H, W), dtype=torch.int16, device=DEV) for _ in range(n)]
    S = [torch.empty((B, H, W), **f32) for _ in range(n)]
    w18 = o.filter_krsc(w.to(DEV)).float().reshape(-1)
    for i, a in enumerate(xs_v):
        o.fusion_stats(a, mm[i], am[i], sq[:, i * Cn:(i + 1) * Cn])
        o.sab_map_fwd(mm[i], w18, S[i])
    G = torch.empty((B, n * Cn), **f32)
    a_d, g_d, b_d = (t.reshape(-1).to(DEV) for t in (alpha, gamma, beta))
    o.gct_gate_fwd(sq, a_d, g_d, b_d, EPS, G)
    out = torch.empty((B, H, W, Cn), dtype=dtype, device=DEV)
    o.fusion_combine(xs_v, S, G, out)
    dG = torch.zeros((B, n * Cn), **f32)
    dS = [torch.empty((B, H, W), **f32) for _ in range(n)]
    dmm = [torch.empty((B, H, W, 2), **f32) for _ in range(n)]
    dw18 = torch.zeros(18, **f32)
    for i, a in enumerate(xs_v):
        o.fusion_bwd_reduce(dout_v, a, dG[:, i * Cn:(i + 1) * Cn], dS[i])
        o.sab_map_bwd(dS[i], S[i], mm[i], w18, dmm[i], dw18)
    q = torch.empty((B, n * Cn), **f32)
    pg = [torch.zeros(n * Cn, **f32) for _ in range(3)]
    o.gct_gate_bwd(sq, a_d, g_d, b_d, EPS, dG, q, pg[0], pg[1], pg[2])
    for i, a in enumerate(xs_v):
        o.fusion_bwd_apply(dout_v, a, G[:, i * Cn:(i + 1) * Cn], q[:, i * Cn:(i + 1) * Cn], S[i], dmm[i], am[i], acc_into[i], True)
    torch.cuda.synchronize()
    return out, dw18, pg


def _chain_ref(xs, w, alpha, gamma, beta, dout, dx0, dt):
    n = len(xs)
    x_ = [x.to(dt).permute(0, 3, 1, 2).clone().requires_grad_(True) for x in xs]
    key = "f.gsc2." if n == 2 else "f.gsc3."
    sd = {"f.sab.cv1.weight": w.to(dt).clone().requires_grad_(True), key + "alpha": alpha.to(dt).view(1, -1, 1, 1).clone().requires_grad_(True),
          key + "gamma": gamma.to(dt).view(1, -1, 1, 1).clone().requires_grad_(True), key + "beta": beta.to(dt).view(1, -1, 1, 1).clone().requires_grad_(True)}
    y = R.fusion_eschannel(sd, "f.", x_)
    gr = torch.autograd.grad((y * dout.to(dt).permute(0, 3, 1, 2)).sum(), x_ + list(sd.values()))
    dxs = [d0.to(dt) + g.permute(0, 2, 3, 1) for d0, g in zip(dx0, gr[:n])]
    return y.detach().permute(0, 2, 3, 1), dxs, gr[n].permute(0, 2, 3, 1).reshape(-1), [g.reshape(-1) for g in gr[n + 1:]]


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("n,shape", [(3, (2, 37, 41)), (2, (2, 37, 41)), (3, (2, 80, 80))], ids=["n3-2x37x41", "n2-2x37x41", "n3-2x80x80"])
def test_fusion_chain_vs_oracle_autograd(reduction_mode, n, shape, dtype):
    """Forward and backward exactly as Fusion._run launches them at C = 128, against autograd of oracle.yolo11_ref.fusion_eschannel:
    out, dx_i (accumulated into a non-zero channel slice), d sab.cv1.weight, d alpha / gamma / beta."""
    B, H, W = shape
    Cn = 128
    xs = _xs(n, B, H, W, Cn, dtype, seed=100)
    w = rnd(1, 2, 3, 3, seed=110, scale=0.7)
    alpha, gamma, beta = 1.0 + rnd(n * Cn, seed=111, scale=0.3), rnd(n * Cn, seed=112, scale=0.6), rnd(n * Cn, seed=113, scale=0.4)
    dout = rounded(rnd(B, H, W, Cn, seed=114), dtype)
    dx0 = [rounded(rnd(B, H, W, Cn, seed=120 + i), dtype) for i in range(n)]
    xv = [nhwc_view(x, dtype, True)[0] for x in xs]
    acc = [nhwc_view(d0, dtype, True) for d0 in dx0]
    out, dw18, pg = _chain_gpu(xv, w, alpha, gamma, beta, nhwc_view(dout, dtype, False)[0], dtype, [a for a, _ in acc])
    for _, buf in acc:
        assert outside_untouched(buf, Cn)
    r64, r32 = _chain_ref(xs, w, alpha, gamma, beta, dout, dx0, torch.float64), _chain_ref(xs, w, alpha, gamma, beta, dout, dx0, F32)
    b = Bars(f"fusion chain[{reduction_mode}] n{n} {B}x{H}x{W}x{Cn} {dtype}")
    b.add("out", out.float(), r64[0], r32[0], dtype)
    for i in range(n):
        b.add(f"dx{i}(+dx0)", acc[i][0].float(), r64[1][i], r32[1][i], dtype)
    b.add("d sab.cv1.weight", dw18, r64[2], r32[2])
    for name, got, i in (("dalpha", pg[0], 0), ("dgamma", pg[1], 1), ("dbeta", pg[2], 2)):
        b.add(name, got, r64[3][i], r32[3][i])
    b.check()


# ------------------------------------------------------------------------------------------------ argument checks
def _call_all(x, dx, Cn):
    """Every entry that takes an NHWC view, on sentinel-filled outputs; returns the outputs so the caller can see nothing ran."""
    o = ops()
    B, H, W, _ = x.shape
    f32 = dict(dtype=F32, device=DEV)
    mm, am, sq = torch.full((B, H, W, 2), -7.0, **f32), torch.full((B, H, W), -1, dtype=torch.int16, device=DEV), torch.full((B, Cn), -7.0, **f32)
    S, G = torch.zeros((B, H, W), **f32), torch.zeros((B, 2 * Cn), **f32)
    dS = torch.full((B, H, W), -7.0, **f32)
    Err = lib().Sy11Error
    with pytest.raises(Err):
        o.fusion_stats(x, mm, am, sq)
    with pytest.raises(Err):
        o.fusion_combine([x, x], [S, S], G, dx)
    with pytest.raises(Err):
        o.fusion_bwd_reduce(x, x, sq, dS)
    with pytest.raises(Err):
        o.fusion_bwd_apply(x, x, G[:, :Cn], G[:, :Cn], S, mm, am, dx, False)
    torch.cuda.synchronize()
    for t, v in ((mm, -7.0), (am, -1), (sq, -7.0), (dS, -7.0), (dx, 3.0)):
        assert bool((t.float() == v).all()), "a rejected call launched a kernel"


@pytest.mark.parametrize("dtype,Cn", [(F32, 6), (F16, 12), (F16, 384), (F32, 48), (F32, 512), (BF16, 1024)],
                         ids=["f32-C6", "f16-C12", "f16-C384", "f32-C48", "f32-C512", "bf16-C1024"])
def test_illegal_channel_counts_are_rejected(dtype, Cn):
    """C not a multiple of the 16-byte vector; C / vec not a power of two (384 in f16 = 48 lanes); more than 64 lanes."""
    x = torch.ones((1, 2, 3, Cn), dtype=dtype, device=DEV)
    _call_all(x, torch.full((1, 2, 3, Cn), 3.0, dtype=dtype, device=DEV), Cn)


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_misaligned_views_are_rejected(dtype):
    """A channel slice that starts one element into the buffer (not 16-byte addressable), and a pixel stride that is not a
    whole number of vectors."""
    Cn = 64
    vec = 16 // torch.empty((), dtype=dtype).element_size()
    wide = torch.ones((1, 2, 3, Cn + 2 * vec), dtype=dtype, device=DEV)
    odd = torch.ones((1, 2, 3, Cn + vec + 1), dtype=dtype, device=DEV)
    for x in (wide[..., 1:1 + Cn], odd[..., :Cn]):
        _call_all(x, torch.full((1, 2, 3, Cn), 3.0, dtype=dtype, device=DEV), Cn)
    good = torch.ones((1, 2, 3, Cn), dtype=dtype, device=DEV)
    dxw = torch.full((1, 2, 3, Cn + 2 * vec), 3.0, dtype=dtype, device=DEV)
    S, G = torch.zeros((1, 2, 3), device=DEV), torch.zeros((1, 2 * Cn), device=DEV)
    with pytest.raises(lib().Sy11Error):
        ops().fusion_combine([good, good], [S, S], G, dxw[..., 1:1 + Cn])
    torch.cuda.synchronize()
    assert bool((dxw == 3.0).all())
