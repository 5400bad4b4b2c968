"""CPU: the float64 reference of the BatchNorm kernels (tests/_bn_ref.py) against float64 autograd of
F.batch_norm(training=True) -> F.silu -> + res, and its edges (a constant channel, count = 1, a negative variance before the clamp)
against the closed form.  tests/test_bn_kernels_gpu.py compares the kernels with this reference."""
import pytest
import torch
import torch.nn.functional as F

from tests import _bn_ref as R

F64 = torch.float64
EPS, MOM = 1e-3, 0.03
REL = 1e-12


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def _inputs(B, H, W, C, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g, dtype=F64) * 2 - 1
    y = 2 * r(C) + (0.2 + 0.9 * (r(C) + 1)) * r(B, H, W, C)
    dz = 0.5 * r(C) + r(B, H, W, C)
    gamma = 1 + 0.5 * r(C)
    gamma[0], gamma[C // 2] = -0.7, 0.0
    return y, dz, r(B, H, W, C), gamma, 0.3 * r(C), 0.1 * r(C), 1 + 0.2 * r(C).abs()


def _chain(y, dz, res, gamma, beta, rm, rv, silu, slots):
    """finalize -> act_fwd -> bwd_sums -> bwd_apply in float64, the sums handed on as `slots` rows"""
    C = y.shape[-1]
    M = y.numel() // C
    y2 = y.reshape(-1, C)
    part = torch.linspace(0.5, 1.5, slots, dtype=F64)[:, None]
    part = part / part.sum()
    mean, rstd, scale, shift, rm2, rv2 = R.finalize(M, part * y2.sum(0), part * (y2 * y2).sum(0), gamma, beta, EPS, MOM, rm, rv, F64)
    z = R.act_fwd(y, scale, shift, silu, res, F64)
    sg, sgx = R.bwd_sums(y, dz, mean, rstd, scale, shift, silu, F64)
    dy, dgamma, dbeta = R.bwd_apply(y, dz, mean, rstd, scale, shift, gamma, silu, part * sg, part * sgx, M, F64)
    return dict(z=z, dy=dy, dgamma=dgamma, dbeta=dbeta, rm=rm2, rv=rv2, mean=mean, rstd=rstd, scale=scale, shift=shift)


@pytest.mark.parametrize("slots", [1, 5])
@pytest.mark.parametrize("silu", [True, False], ids=["silu", "linear"])
@pytest.mark.parametrize("shape", [(2, 5, 7, 6), (3, 9, 4, 17), (1, 1, 2, 3)], ids=lambda s: "x".join(map(str, s)))
def test_reference_matches_float64_autograd(shape, silu, slots):
    B, H, W, C = shape
    y, dz, res, gamma, beta, rm, rv = _inputs(B, H, W, C, seed=3 + C)
    got = _chain(y, dz, res, gamma, beta, rm, rv, silu, slots)
    nchw = lambda t: t.permute(0, 3, 1, 2)
    ya, ra = nchw(y).clone().requires_grad_(True), nchw(res).clone().requires_grad_(True)
    ga, ba = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rma, rva = rm.clone(), rv.clone()
    mom, eps = R.f32_value(MOM), R.f32_value(EPS)          # the kernel's `float` arguments
    u = F.batch_norm(ya, rma, rva, ga, ba, True, mom, eps)
    z = (F.silu(u) if silu else u) + ra
    (z * nchw(dz)).sum().backward()
    nhwc = lambda t: t.permute(0, 2, 3, 1)
    assert _rel(got["z"], nhwc(z.detach())) <= REL
    assert _rel(got["dy"], nhwc(ya.grad)) <= REL
    assert _rel(got["dgamma"], ga.grad) <= REL
    assert _rel(got["dbeta"], ba.grad) <= REL
    assert torch.equal(nhwc(ra.grad), dz), "the residual operand's gradient is dz itself"
    assert _rel(got["rm"], rma) <= REL
    assert _rel(got["rv"], rva) <= REL


@pytest.mark.parametrize("silu", [True, False], ids=["silu", "linear"])
def test_constant_channel_closed_form(silu):
    """y = c in one channel: mean = c, var = 0, rstd = 1 / sqrt(eps), xhat = 0, z = act(beta), dy = gamma * rstd * (g - mean(g))."""
    y, dz, res, gamma, beta, rm, rv = _inputs(2, 4, 5, 4, seed=9)
    c = 1.625
    y[..., 1] = c
    got = _chain(y, dz, None, gamma, beta, rm, rv, silu, 3)
    eps, mom = R.f32_value(EPS), R.f32_value(MOM)
    rs = eps ** -0.5
    assert got["mean"][1].item() == c
    assert abs(got["rstd"][1].item() - rs) <= REL * rs
    assert abs(got["shift"][1].item() - (beta[1].item() - c * gamma[1].item() * rs)) <= 1e-12 * abs(c * gamma[1].item() * rs)
    assert abs(got["rv"][1].item() - (1 - mom) * rv[1].item()) <= REL
    act = (lambda t: t * torch.sigmoid(t)) if silu else (lambda t: t)
    ub = torch.full((), c, dtype=F64) * got["scale"][1] + got["shift"][1]
    assert (got["z"][..., 1] - act(ub)).abs().max().item() == 0.0
    assert abs(ub.item() - beta[1].item()) <= 1e-12 * abs(c * gamma[1].item() * rs)
    g = dz[..., 1] * (R.dsilu(ub) if silu else 1.0)
    want = gamma[1] * rs * (g - g.mean())
    assert _rel(got["dy"][..., 1], want) <= REL
    assert abs(got["dgamma"][1].item()) <= REL * g.abs().sum().item()


def test_count_one_and_negative_variance():
    """One pixel: var = 0, the unbiased factor is 1 (not 1 / 0), dy = 0.  Sums whose E[x^2] - mean^2 is below zero: clamped."""
    C = 3
    y = torch.tensor([[[[0.75, -1.5, 2.0]]]], dtype=F64)
    dz = torch.tensor([[[[0.5, -0.25, 1.0]]]], dtype=F64)
    gamma, beta = torch.tensor([1.5, -0.5, 0.0], dtype=F64), torch.tensor([0.1, 0.2, 0.3], dtype=F64)
    rm, rv = torch.zeros(C, dtype=F64), torch.ones(C, dtype=F64)
    got = _chain(y, dz, None, gamma, beta, rm, rv, True, 1)
    eps, mom = R.f32_value(EPS), R.f32_value(MOM)
    assert torch.equal(got["mean"], y.reshape(-1))
    assert torch.allclose(got["rstd"], torch.full((C,), eps ** -0.5, dtype=F64), rtol=REL, atol=0)
    assert torch.allclose(got["rv"], torch.full((C,), 1 - mom, dtype=F64), rtol=REL, atol=0)
    assert torch.allclose(got["rm"], mom * y.reshape(-1), rtol=REL, atol=0)
    assert got["dy"].abs().max().item() <= 1e-13
    assert bool(torch.isfinite(got["rv"]).all())
    # sum = 3, sum of squares a little under 9 at count 1, and over 4 pixels: var < 0 before the clamp
    for count, s1, s2 in ((1, 3.0, 8.9999), (4, 12.0, 35.9996)):
        one = lambda v: torch.tensor([v], dtype=F64)
        mean, rstd, scale, shift, rm2, rv2 = R.finalize(count, one(s1), one(s2), one(2.0), one(0.5), EPS, MOM, one(0.0), one(1.0), F64)
        assert mean.item() == 3.0 and abs(rstd.item() - eps ** -0.5) <= REL * eps ** -0.5
        assert abs(rv2.item() - (1 - mom)) <= REL
        m32 = R.finalize(count, one(s1), one(s2), one(2.0), one(0.5), EPS, MOM, one(0.0), one(1.0), torch.float32)
        assert all(t.dtype == torch.float32 for t in m32)
        assert m32[1].item() == rstd.float().item() and m32[0].item() == 3.0


def test_float32_variant_rounds_mean_and_rstd_once():
    """dt = float32: mean and rstd are the float64 results rounded once; scale and shift are f32 products of the rounded values."""
    y, dz, res, gamma, beta, rm, rv = _inputs(2, 6, 5, 9, seed=21)
    y2 = y.float().reshape(-1, 9)
    ssum, ssq = torch.stack((y2.sum(0), 0 * y2.sum(0))), torch.stack(((y2 * y2).sum(0), 0 * y2.sum(0)))
    a64 = R.finalize(60, ssum, ssq, gamma.float(), beta.float(), EPS, MOM, rm.float(), rv.float(), F64)
    a32 = R.finalize(60, ssum, ssq, gamma.float(), beta.float(), EPS, MOM, rm.float(), rv.float(), torch.float32)
    assert torch.equal(a32[0], a64[0].float()) and torch.equal(a32[1], a64[1].float())
    assert torch.equal(a32[2], gamma.float() * a32[1])
    assert torch.equal(a32[3], beta.float() - a32[0] * a32[2])
    for v32, v64 in zip(a32, a64):
        assert _rel(v32.double(), v64) <= 4 * 2.0 ** -24
