"""Plain-torch CPU reference of the four BatchNorm kernels of csrc/elementwise.hip (sy11_bn_finalize, sy11_bn_act_fwd,
sy11_bn_act_bwd_reduce, sy11_bn_act_bwd_apply[_res]): the formulas of include/sy11.h, one function per kernel.  Not a test module.

Every function takes inputs that are ALREADY rounded to the kernel's storage dtype (activations) or to f32 (per-channel vectors,
slot rows) and evaluates the formula in the compute dtype ``dt``.  The parity tests call each once with torch.float64 (``r64``) and
once with torch.float32 (``r32``); tests/_kernel_ref.py derives the bar from the difference of the two.  Activations are NHWC,
shape (..., C); per-channel vectors are [C]; slot rows are [slots, C] (a [C] vector counts as one slot).
"""
import torch

F32, F64 = torch.float32, torch.float64


def f32_value(v):
    """A Python float as the kernel receives it through a `float` argument."""
    return float(torch.tensor(float(v), dtype=F32))


def _rows(t):
    return t.reshape(1, -1) if t.dim() == 1 else t


def silu(u):
    return u * torch.sigmoid(u)


def dsilu(u):
    """d/du silu(u) = s + u * s * (1 - s),  s = sigmoid(u)"""
    s = torch.sigmoid(u)
    return s * (1 + u * (1 - s))


def finalize(count, ssum, ssq, gamma, beta, eps, momentum, running_mean, running_var, dt=F64):
    """-> mean, rstd, scale, shift, new running_mean, new running_var (the last two None without running statistics).

    The kernel folds the slot rows and divides in double and rounds mean and rstd ONCE, so with dt = float32 mean and rstd are the
    float64 values rounded to f32; scale, shift and the running statistics then repeat the kernel's f32 steps from those rounded
    values.  With dt = float64 nothing is rounded.  eps and momentum are taken at their f32 values (they are `float` arguments).
    The clamp var < 0 -> 0 and the unbiased factor count / (count - 1) (1 when count = 1) are part of the formula."""
    count, eps, momentum = float(count), f32_value(eps), f32_value(momentum)
    s1, s2 = _rows(ssum).to(F64).sum(0), _rows(ssq).to(F64).sum(0)
    mu = s1 / count
    var = (s2 / count - mu * mu).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    unbiased = var * (count / (count - 1.0)) if count > 1 else var
    if dt == F64:
        g, b = gamma.to(F64), beta.to(F64)
        scale = g * rstd
        shift = b - mu * scale
        if running_mean is None:
            return mu, rstd, scale, shift, None, None
        rm = (1.0 - momentum) * running_mean.to(F64) + momentum * mu
        rv = (1.0 - momentum) * running_var.to(F64) + momentum * unbiased
        return mu, rstd, scale, shift, rm, rv
    assert dt == F32
    mu32, rstd32 = mu.to(F32), rstd.to(F32)
    g, b = gamma.to(F32), beta.to(F32)
    scale = g * rstd32
    shift = b - mu32 * scale
    if running_mean is None:
        return mu32, rstd32, scale, shift, None, None
    m = torch.tensor(momentum, dtype=F32)
    keep = torch.tensor(1.0, dtype=F32) - m
    rm = keep * running_mean.to(F32) + m * mu32
    rv = keep * running_var.to(F32) + m * unbiased.to(F32)
    return mu32, rstd32, scale, shift, rm, rv


def act_fwd(y, scale, shift, silu_on, res, dt=F64):
    """z = act(y * scale[c] + shift[c]) (+ res)"""
    u = y.to(dt) * scale.to(dt) + shift.to(dt)
    z = silu(u) if silu_on else u
    return z if res is None else z + res.to(dt)


def _g_xhat(y, dz, mean, rstd, scale, shift, silu_on, dt):
    yd = y.to(dt)
    g = dz.to(dt)
    if silu_on:
        g = g * dsilu(yd * scale.to(dt) + shift.to(dt))
    return g, (yd - mean.to(dt)) * rstd.to(dt)


def bwd_terms(y, dz, mean, rstd, scale, shift, silu_on, dt=F64):
    """The summands of bwd_sums: g = dz * act'(y * scale + shift) and g * xhat, xhat = (y - mean) * rstd."""
    g, xh = _g_xhat(y, dz, mean, rstd, scale, shift, silu_on, dt)
    return g, g * xh


def bwd_sums(y, dz, mean, rstd, scale, shift, silu_on, dt=F64):
    """-> sum_g[c] = sum over pixels of g, sum_gx[c] = sum over pixels of g * xhat"""
    g, gx = bwd_terms(y, dz, mean, rstd, scale, shift, silu_on, dt)
    C = g.shape[-1]
    return g.reshape(-1, C).sum(0), gx.reshape(-1, C).sum(0)


def bwd_apply(y, dz, mean, rstd, scale, shift, gamma, silu_on, sum_g_slots, sum_gx_slots, M, dt=F64):
    """-> dy = gamma * rstd * (g - sum_g / M - xhat * sum_gx / M), and the increments of dgamma (= sum_gx) and dbeta (= sum_g).
    sum_g / sum_gx are the totals of the slot rows GIVEN, not recomputed sums: the fold of the rows is part of the formula."""
    tg, tgx = _rows(sum_g_slots).to(dt).sum(0), _rows(sum_gx_slots).to(dt).sum(0)
    g, xh = _g_xhat(y, dz, mean, rstd, scale, shift, silu_on, dt)
    dy = (gamma.to(dt) * rstd.to(dt)) * (g - tg / M - xh * (tgx / M))
    return dy, tgx, tg
