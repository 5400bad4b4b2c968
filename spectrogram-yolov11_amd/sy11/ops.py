"""Tensor-level wrappers over the C-ABI (sy11._lib): build descriptors from torch tensors, pass raw device
pointers + the current HIP stream.  torch is plumbing only (memory, streams); every computation is a libsy11 kernel.

An NHWC *view* is a torch tensor of shape (B, H, W, C) whose strides are (H*W*ld, W*ld, ld, 1): a channel slice
``buf[..., a:b]`` of a contiguous NHWC buffer qualifies (ld = buf.shape[-1]) — concat by pointer.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import EPI_ACCUM, EPI_OUT_F32, EPI_SILU, BnTail, ConvDesc, OptDesc, call

_DT = {torch.float32: _lib.F32, torch.float16: _lib.F16, torch.bfloat16: _lib.BF16}


def dt_code(t: torch.dtype) -> int:
    try:
        return _DT[t]
    except KeyError:
        raise _lib.Sy11Error(f"unsupported dtype {t}") from None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.Sy11Error("sy11 ops need tensors on the MI355X (cuda) device; there is no CPU path")


def view_ld(t: torch.Tensor) -> int:
    """Pixel stride of an NHWC view; validates the stride pattern."""
    if t.dim() != 4:
        raise _lib.Sy11Error(f"expected a 4-d NHWC view, got shape {tuple(t.shape)}")
    B, H, W, Cn = t.shape
    ld = t.stride(2) if W > 1 else (t.stride(1) // max(W, 1) if H > 1 else max(t.stride(0) // max(H * W, 1), Cn))
    ok = (Cn == 1 or t.stride(3) == 1) and (W == 1 or t.stride(2) == ld) and (H == 1 or t.stride(1) == W * ld) \
        and (B == 1 or t.stride(0) == H * W * ld) and ld >= Cn
    if not ok:
        raise _lib.Sy11Error(f"not an NHWC view: shape {tuple(t.shape)} strides {t.stride()}")
    return ld


def nhwc_empty(B, H, W, Cn, dtype, device):
    return torch.empty((B, H, W, Cn), dtype=dtype, device=device)


def dgrad_leaves_holes(k, s, p, d=1) -> bool:
    """True when some input pixels receive no tap at all (stride > reach, or stride and dilation sharing a factor):
    sy11_conv2d_dgrad then needs a zeroed dx and SY11_EPI_ACCUM."""
    return any(all((ph + p - r * d) % s for r in range(k)) for ph in range(s))


def conv_out_hw(H, W, k, s, p, d=1):
    return (H + 2 * p - d * (k - 1) - 1) // s + 1, (W + 2 * p - d * (k - 1) - 1) // s + 1


def _desc(x_shape, x_ld, y_shape, y_ld, dtype, k, s, p, d, groups, flags, slots=1):
    B, IH, IW, Cn = x_shape
    _, OH, OW, N = y_shape
    kh, kw = (k, k) if isinstance(k, int) else k
    if _lib.PROFILE is not None:     # algorithmic FLOPs of this conv problem (same for fwd / dgrad / wgrad)
        _lib.PROFILE_META = {"flops": 2.0 * B * OH * OW * N * (Cn // groups) * kh * kw, "groups": groups,
                             "bytes": (B * IH * IW * Cn + B * OH * OW * N + N * (Cn // groups) * kh * kw)
                             * torch.empty((), dtype=dtype).element_size(),
                             "desc": f"B{B} {IH}x{IW}x{Cn}->{OH}x{OW}x{N} k{kh} s{s} g{groups}"}
    return ConvDesc(dt_code(dtype), B, IH, IW, Cn, x_ld, OH, OW, N, y_ld, kh, kw, s, s, p, p, d, d, groups, flags, slots)


def filter_krsc(w: torch.Tensor) -> torch.Tensor:
    """OIHW parameter -> memory [O][KH][KW][I].  Free when the parameter is kept in channels_last format."""
    v = w.permute(0, 2, 3, 1)
    return v if v.is_contiguous() else v.contiguous()


def conv2d_fwd(x, w_krsc, y, k, s=1, p=0, d=1, groups=1, bias=None, stats=None, silu=False, out_f32=False):
    """x, y: NHWC views; w_krsc: contiguous [N][KH][KW][C/groups]; stats: (sum, sumsq), each f32 [N] or [slots][N],
    accumulated into."""
    _need_gpu(x, w_krsc, y, bias)
    flags = (EPI_SILU if silu else 0) | (EPI_OUT_F32 if out_f32 else 0)
    slots = stats[0].shape[0] if (stats and stats[0].dim() == 2) else 1
    dsc = _desc(x.shape, view_ld(x), y.shape, view_ld(y), x.dtype, k, s, p, d, groups, flags, slots)
    call("sy11_conv2d_fwd", C.byref(dsc), _p(x), _p(w_krsc), _p(bias), _p(y), _p(stats[0]) if stats else None,
         _p(stats[1]) if stats else None, _stream())
    return y


def _bn_tail(count, gamma, beta, eps, momentum, running_mean, running_var, mean, rstd, scale, shift, ticket):
    return BnTail(_p(gamma), _p(beta), _p(running_mean), _p(running_var), _p(mean), _p(rstd), _p(scale), _p(shift), _p(ticket),
                  float(eps), float(momentum), float(count))


def conv2d_fwd_bn(x, w_krsc, y, k, s, p, d, groups, stats, bn):
    """Train-mode Conv.forward up to the BN statistics: conv + per-channel sum/sumsq + (in the kernel tail) mean / rstd /
    scale / shift / running-stat update.  ``bn`` = (count, gamma, beta, eps, momentum, running_mean, running_var, mean, rstd,
    scale, shift, ticket) with ``ticket`` a zeroed 4-byte-per-group buffer."""
    _need_gpu(x, w_krsc, y)
    slots = stats[0].shape[0] if stats[0].dim() == 2 else 1
    dsc = _desc(x.shape, view_ld(x), y.shape, view_ld(y), x.dtype, k, s, p, d, groups, 0, slots)
    tail = _bn_tail(*bn)
    call("sy11_conv2d_fwd_bn", C.byref(dsc), _p(x), _p(w_krsc), _p(y), _p(stats[0]), _p(stats[1]), C.byref(tail), _stream())
    return y


def stem_conv_fwd_bn(x_nchw, w_krsc, y, s, p, stats, bn):
    _need_gpu(x_nchw, w_krsc, y)
    if x_nchw.dtype != torch.float32 or not x_nchw.is_contiguous() or x_nchw.shape[1] != 3:
        raise _lib.Sy11Error("stem_conv_fwd_bn: x must be a contiguous NCHW f32 image with 3 channels")
    B, _, IH, IW = x_nchw.shape
    slots = stats[0].shape[0] if stats[0].dim() == 2 else 1
    dsc = _desc((B, IH, IW, 3), 3, y.shape, view_ld(y), y.dtype, 3, s, p, 1, 1, 0, slots)
    tail = _bn_tail(*bn)
    call("sy11_stem_conv_fwd_bn", C.byref(dsc), _p(x_nchw), _p(w_krsc), _p(y), _p(stats[0]), _p(stats[1]), C.byref(tail), _stream())
    return y


def weight_transpose(w_krsc: torch.Tensor, groups: int = 1) -> torch.Tensor:
    """dgrad filter: [C][KH][KW][N] for a dense conv; [groups][C/g][KH][KW][N/g] for a grouped one (each group's block
    transposed on its own — the layout sy11_conv2d_dgrad documents)."""
    N, KH, KW, Cn = w_krsc.shape
    if groups > 1:
        ng = N // groups
        wt = torch.empty((groups, Cn, KH, KW, ng), dtype=w_krsc.dtype, device=w_krsc.device)
        for g in range(groups):
            call("sy11_weight_transpose", dt_code(w_krsc.dtype), ng, KH * KW, Cn, _p(w_krsc[g * ng:(g + 1) * ng]), _p(wt[g]), _stream())
        return wt
    wt = torch.empty((Cn, KH, KW, N), dtype=w_krsc.dtype, device=w_krsc.device)
    call("sy11_weight_transpose", dt_code(w_krsc.dtype), N, KH * KW, Cn, _p(w_krsc), _p(wt), _stream())
    return wt


def conv2d_dgrad(dy, w_or_wt, dx, y_shape, k, s=1, p=0, d=1, groups=1, accumulate=False):
    """dx (NHWC view of the conv INPUT shape) = conv^T(dy).  groups==1: pass the tap-transposed filter."""
    _need_gpu(dy, w_or_wt, dx)
    dsc = _desc(dx.shape, view_ld(dx), y_shape, y_shape[-1], dy.dtype, k, s, p, d, groups, EPI_ACCUM if accumulate else 0)
    call("sy11_conv2d_dgrad", C.byref(dsc), _p(dy), view_ld(dy), _p(w_or_wt), _p(dx), _stream())
    return dx


def conv2d_wgrad(x, dy, dw_f32, k, s=1, p=0, d=1, groups=1):
    """dw_f32 ([N][KH][KW][C/groups], f32) += x (*) dy."""
    _need_gpu(x, dy, dw_f32)
    if dw_f32.dtype != torch.float32 or not dw_f32.is_contiguous():
        raise _lib.Sy11Error("conv2d_wgrad: dw must be a contiguous f32 tensor")
    dsc = _desc(x.shape, view_ld(x), dy.shape, view_ld(dy), x.dtype, k, s, p, d, groups, 0)
    call("sy11_conv2d_wgrad", C.byref(dsc), _p(x), _p(dy), view_ld(dy), _p(dw_f32), _stream())
    return dw_f32


def conv2d_dgrad_wgrad_1x1(dy, x, wt, dx, dw_f32, accumulate=False):
    """Dense 1x1 / stride-1 layer: dx (NHWC view, the shape of x) = dy * w [+ dx] AND dw_f32 ([N][1][1][C], f32) += dy^T * x in one
    launch that reads dy once (sy11_conv2d_dgrad_wgrad_1x1).  dy, x, dx: 16-bit NHWC views of the same B, H, W; wt: the
    tap-transposed filter [C][1][1][N] of weight_transpose."""
    _need_gpu(dy, x, wt, dx, dw_f32)
    B, H, W, N = dy.shape
    Cn = x.shape[3]
    if tuple(x.shape[:3]) != (B, H, W) or tuple(dx.shape) != tuple(x.shape) or x.dtype != dy.dtype or dx.dtype != dy.dtype or wt.dtype != dy.dtype:
        raise _lib.Sy11Error(f"conv2d_dgrad_wgrad_1x1: dy {tuple(dy.shape)} {dy.dtype}, x {tuple(x.shape)} {x.dtype}, dx {tuple(dx.shape)} {dx.dtype} "
                             f"do not belong to one 1x1 stride-1 layer")
    if dw_f32.dtype != torch.float32 or not dw_f32.is_contiguous() or dw_f32.numel() != N * Cn:
        raise _lib.Sy11Error("conv2d_dgrad_wgrad_1x1: dw must be a contiguous f32 tensor of N * C elements")
    if not wt.is_contiguous() or wt.numel() != N * Cn:
        raise _lib.Sy11Error("conv2d_dgrad_wgrad_1x1: wt must be the contiguous [C][1][1][N] filter of weight_transpose")
    M = B * H * W
    if _lib.PROFILE is not None:     # both GEMMs; dy, x and dx once each, the filter read and its gradient written
        es = dy.element_size()
        _lib.PROFILE_META = {"flops": 4.0 * M * N * Cn, "groups": 1, "bytes": (M * N + 2 * M * Cn + 2 * N * Cn) * es,
                             "desc": f"B{B} {H}x{W}x{Cn}->{H}x{W}x{N} k1 s1 g1 dgrad+wgrad"}
    call("sy11_conv2d_dgrad_wgrad_1x1", dt_code(dy.dtype), M, Cn, N, _p(dy), view_ld(dy), _p(x), view_ld(x), _p(wt), _p(dx), view_ld(dx),
         1 if accumulate else 0, _p(dw_f32), _stream())
    return dx


def dgrad_wgrad_1x1_plan(Cn, N, lds_bytes=160 * 1024):
    """The tile choice of conv2d_dgrad_wgrad_1x1 (sy11_dgrad_wgrad_1x1_plan, host arithmetic): (np, cp, cb, blocks)."""
    v = [C.c_int32() for _ in range(4)]
    _lib.check(_lib.load().sy11_dgrad_wgrad_1x1_plan(int(Cn), int(N), int(lds_bytes), *[C.byref(e) for e in v]), "sy11_dgrad_wgrad_1x1_plan")
    return tuple(int(e.value) for e in v)


def conv2d_wgrad_group(problems, target_workgroups=0):
    """Several dense 16-bit filter gradients in one launch (sy11_conv2d_wgrad_group): ``problems`` is a sequence of
    (x, dy, dw_f32, k, s, p, d), each exactly conv2d_wgrad(x, dy, dw_f32, k, s, p, d).  A list longer than WGRAD_GROUP_MAX goes out
    as several launches.  ``target_workgroups``: workgroups per launch, 0 = one resident round of the chip."""
    problems = list(problems)
    if not problems:
        raise _lib.Sy11Error("conv2d_wgrad_group: empty problem list")
    dt = problems[0][0].dtype
    for at in range(0, len(problems), _lib.WGRAD_GROUP_MAX):
        part = problems[at:at + _lib.WGRAD_GROUP_MAX]
        arr = (_lib.WgradProblem * len(part))()
        flops = nbytes = 0.0
        for i, (x, dy, dw, k, s, p, d) in enumerate(part):
            _need_gpu(x, dy, dw)
            if dw.dtype != torch.float32 or not dw.is_contiguous():
                raise _lib.Sy11Error("conv2d_wgrad_group: dw must be a contiguous f32 tensor")
            if x.dtype != dt or dy.dtype != dt:
                raise _lib.Sy11Error("conv2d_wgrad_group: every problem of a group has the same dtype")
            arr[i].desc = _desc(x.shape, view_ld(x), dy.shape, view_ld(dy), x.dtype, k, s, p, d, 1, 0)
            arr[i].x, arr[i].dy, arr[i].dw, arr[i].dy_ld = x.data_ptr(), dy.data_ptr(), dw.data_ptr(), view_ld(dy)
            if _lib.PROFILE is not None:
                flops += _lib.PROFILE_META["flops"]
                nbytes += _lib.PROFILE_META["bytes"]
        if _lib.PROFILE is not None:
            _lib.PROFILE_META = {"flops": flops, "groups": 1, "bytes": nbytes, "desc": f"group of {len(part)}"}
        call("sy11_conv2d_wgrad_group", dt_code(dt), len(part), arr, int(target_workgroups), _stream())


def wgrad_group_plan(M, N, K, target_workgroups):
    """The work split of one grouped launch (sy11_wgrad_group_plan, host arithmetic): (pix_per_split[count], wg_start[count + 1])."""
    n = len(M)
    arr = lambda v: (C.c_int32 * max(len(v), 1))(*[int(e) for e in v])
    pps, start = (C.c_int32 * max(n, 1))(), (C.c_int32 * (n + 1))()
    _lib.check(_lib.load().sy11_wgrad_group_plan(n, arr(M), arr(N), arr(K), int(target_workgroups), pps, start), "sy11_wgrad_group_plan")
    return list(pps)[:n], list(start)


def stem_conv_fwd(x_nchw, w_krsc, y, s=2, p=1, bias=None, stats=None, silu=False):
    _need_gpu(x_nchw, w_krsc, y)
    if x_nchw.dtype != torch.float32 or not x_nchw.is_contiguous() or x_nchw.shape[1] != 3:
        raise _lib.Sy11Error("stem_conv_fwd: x must be a contiguous NCHW f32 image with 3 channels")
    B, _, IH, IW = x_nchw.shape
    slots = stats[0].shape[0] if (stats and stats[0].dim() == 2) else 1
    dsc = _desc((B, IH, IW, 3), 3, y.shape, view_ld(y), y.dtype, 3, s, p, 1, 1, EPI_SILU if silu else 0, slots)
    call("sy11_stem_conv_fwd", C.byref(dsc), _p(x_nchw), _p(w_krsc), _p(bias), _p(y), _p(stats[0]) if stats else None,
         _p(stats[1]) if stats else None, _stream())
    return y


def stem_conv_wgrad(x_nchw, dy, dw_f32, s=2, p=1):
    _need_gpu(x_nchw, dy, dw_f32)
    B, _, IH, IW = x_nchw.shape
    dsc = _desc((B, IH, IW, 3), 3, dy.shape, view_ld(dy), dy.dtype, 3, s, p, 1, 1, 0)
    call("sy11_stem_conv_wgrad", C.byref(dsc), _p(x_nchw), _p(dy), view_ld(dy), _p(dw_f32), _stream())
    return dw_f32


def _mc(t):
    B, H, W, Cn = t.shape
    return B * H * W, Cn


def bn_finalize(count, ssum, ssq, gamma, beta, eps, momentum, running_mean, running_var, mean, rstd, scale, shift):
    slots = ssum.shape[0] if ssum.dim() == 2 else 1
    if _lib.PROFILE is not None:
        _lib.PROFILE_META = {"flops": 0.0, "bytes": float(gamma.numel() * 4 * (2 * slots + 8)), "desc": f"bn_finalize {gamma.numel()}"}
    call("sy11_bn_finalize", gamma.numel(), slots, float(count), _p(ssum), _p(ssq), _p(gamma), _p(beta), eps, momentum,
         _p(running_mean), _p(running_var), _p(mean), _p(rstd), _p(scale), _p(shift), _stream())


def _stream_meta(what, M, Cn, *tensors):
    """Algorithmic bytes of a streaming pass (bench.py's roofline leg): every operand read or written once."""
    if _lib.PROFILE is not None:
        _lib.PROFILE_META = {"flops": 0.0, "bytes": float(sum(M * Cn * t.element_size() for t in tensors if t is not None)),
                             "desc": f"{what} {M}x{Cn}"}


def bn_act_fwd(y, scale, shift, z, silu=True, res=None):
    _need_gpu(y, z, res)
    M, Cn = _mc(y)
    _stream_meta("bn_act_fwd", M, Cn, y, z, res)
    call("sy11_bn_act_fwd", dt_code(y.dtype), M, Cn, _p(y), view_ld(y), _p(scale), _p(shift), int(silu), _p(res),
         view_ld(res) if res is not None else 0, _p(z), view_ld(z), _stream())
    return z


def bn_act_bwd_reduce(y, dz, mean, rstd, scale, shift, silu, sum_g, sum_gx):
    M, Cn = _mc(y)
    _stream_meta("bn_bwd_reduce", M, Cn, y, dz)
    slots = sum_g.shape[0] if sum_g.dim() == 2 else 1
    call("sy11_bn_act_bwd_reduce", dt_code(y.dtype), M, Cn, _p(y), view_ld(y), _p(dz), view_ld(dz), _p(mean), _p(rstd),
         _p(scale), _p(shift), int(silu), _p(sum_g), _p(sum_gx), slots, _stream())


def bn_act_bwd_apply(y, dz, mean, rstd, scale, shift, gamma, silu, sum_g, sum_gx, dy, dgamma, dbeta, res_grad=None, res_accumulate=False):
    """``res_grad``: gradient buffer of a residual operand of the layer's output (same pixels, own stride): (= | +=) dz in the same pass."""
    M, Cn = _mc(y)
    _stream_meta("bn_bwd_apply", M, Cn, y, dz, dy)
    slots = sum_g.shape[0] if sum_g.dim() == 2 else 1
    if res_grad is None:
        call("sy11_bn_act_bwd_apply", dt_code(y.dtype), M, Cn, _p(y), view_ld(y), _p(dz), view_ld(dz), _p(mean), _p(rstd),
             _p(scale), _p(shift), _p(gamma), int(silu), _p(sum_g), _p(sum_gx), slots, _p(dy), view_ld(dy), _p(dgamma),
             _p(dbeta), _stream())
        return
    if res_grad.dtype != y.dtype or tuple(res_grad.shape) != tuple(y.shape):
        raise _lib.Sy11Error("bn_act_bwd_apply: the residual gradient must have the layer's shape and dtype")
    call("sy11_bn_act_bwd_apply_res", dt_code(y.dtype), M, Cn, _p(y), view_ld(y), _p(dz), view_ld(dz), _p(mean), _p(rstd),
         _p(scale), _p(shift), _p(gamma), int(silu), _p(sum_g), _p(sum_gx), slots, _p(dy), view_ld(dy), _p(dgamma),
         _p(dbeta), _p(res_grad), view_ld(res_grad), int(bool(res_accumulate)), _stream())


def bias_grad_cast(dz, dy, dbias=None, partials=None):
    """dz: f32 NHWC view (B,H,W,N); dy: contiguous (B,H,W,npad) of the compute dtype, npad >= N (pad channels zeroed);
    dbias: f32 [N] accumulated into.  One launch (two with ``partials``, a [rows][N] scratch selecting the ordered reduction)."""
    _need_gpu(dz, dy, dbias, partials)
    M, N = _mc(dz)
    if dz.dtype != torch.float32 or not dy.is_contiguous() or tuple(dy.shape[:3]) != tuple(dz.shape[:3]) or dy.shape[3] < N:
        raise _lib.Sy11Error("bias_grad_cast: dz must be f32, dy contiguous with the same pixels and >= N channels")
    call("sy11_bias_grad_cast", dt_code(dy.dtype), M, N, dy.shape[3], _p(dz), view_ld(dz), _p(dy), _p(dbias), _p(partials),
         partials.shape[0] if partials is not None else 0, _stream())
    return dy


def copy2d(src, dst, accumulate=False):
    _need_gpu(src, dst)
    M, Cn = _mc(src)
    if tuple(dst.shape) != tuple(src.shape) or dst.dtype != src.dtype:
        raise _lib.Sy11Error(f"copy2d: shape/dtype mismatch {tuple(src.shape)} vs {tuple(dst.shape)}")
    call("sy11_copy2d", dt_code(src.dtype), M, Cn, _p(src), view_ld(src), _p(dst), view_ld(dst), int(accumulate), _stream())
    return dst


def upsample2x_fwd(x, y):
    B, H, W, Cn = x.shape
    call("sy11_upsample2x_fwd", dt_code(x.dtype), B, H, W, Cn, _p(x), view_ld(x), _p(y), view_ld(y), _stream())
    return y


def upsample2x_bwd(dy, dx, accumulate=False):
    B, H, W, Cn = dx.shape
    call("sy11_upsample2x_bwd", dt_code(dx.dtype), B, H, W, Cn, _p(dy), view_ld(dy), _p(dx), view_ld(dx), int(accumulate),
         _stream())
    return dx


def maxpool5_fwd(x, y, idx):
    B, H, W, Cn = x.shape
    call("sy11_maxpool5_fwd", dt_code(x.dtype), B, H, W, Cn, _p(x), view_ld(x), _p(y), view_ld(y), _p(idx), _stream())
    return y


def maxpool5_bwd(dy, idx, dx, accumulate=False):
    B, H, W, Cn = dx.shape
    call("sy11_maxpool5_bwd", dt_code(dx.dtype), B, H, W, Cn, _p(dy), view_ld(dy), _p(idx), _p(dx), view_ld(dx),
         int(accumulate), _stream())
    return dx


def attention_fwd(qkv, heads, kd, hd, o, p):
    B, H, W, _ = qkv.shape
    call("sy11_attention_fwd", dt_code(qkv.dtype), B, H * W, heads, kd, hd, _p(qkv), view_ld(qkv), _p(o), view_ld(o), _p(p),
         _stream())
    return o


def attention_bwd(qkv, heads, kd, hd, p, d_o, dqkv, ws=None, o=None):
    """``o``: the forward output (optional) — with it the 16-bit MFMA path takes softmax's row sums as dO . o and reads P once."""
    B, H, W, _ = qkv.shape
    if ws is None:                                   # caller-owned scratch, sized by the library's own query
        ws = torch.empty(_lib.load().sy11_attention_workspace_bytes(B, H * W, heads) // 4, dtype=torch.float32, device=qkv.device)
    if o is None:
        call("sy11_attention_bwd", dt_code(qkv.dtype), B, H * W, heads, kd, hd, _p(qkv), view_ld(qkv), _p(p), _p(d_o),
             view_ld(d_o), _p(dqkv), view_ld(dqkv), _p(ws), _stream())
    else:
        call("sy11_attention_bwd_o", dt_code(qkv.dtype), B, H * W, heads, kd, hd, _p(qkv), view_ld(qkv), _p(p), _p(o), view_ld(o), _p(d_o),
             view_ld(d_o), _p(dqkv), view_ld(dqkv), _p(ws), _stream())
    return dqkv


def detect_decode(maps, strides, nc):
    """maps: list of contiguous NHWC f32 (B, H, W, 64+nc) -> (B, 4+nc, A) f32."""
    _need_gpu(*maps)
    nl = len(maps)
    B = maps[0].shape[0]
    for m in maps:
        if m.dtype != torch.float32 or not m.is_contiguous() or m.shape[-1] != 64 + nc:
            raise _lib.Sy11Error("detect_decode: maps must be contiguous NHWC f32 with 64+nc channels")
    A = sum(m.shape[1] * m.shape[2] for m in maps)
    out = torch.empty((B, 4 + nc, A), dtype=torch.float32, device=maps[0].device)
    ptrs = (C.c_void_p * nl)(*[m.data_ptr() for m in maps])
    hs = (C.c_int32 * nl)(*[m.shape[1] for m in maps])
    ws = (C.c_int32 * nl)(*[m.shape[2] for m in maps])
    st = (C.c_float * nl)(*[float(s) for s in strides])
    call("sy11_detect_decode", B, nc, nl, C.cast(ptrs, C.c_void_p), C.cast(hs, C.c_void_p), C.cast(ws, C.c_void_p),
         C.cast(st, C.c_void_p), _p(out), _stream())
    return out


def nms_sorted(boxes_sorted: torch.Tensor, iou_thres: float) -> torch.Tensor:
    """boxes sorted by (score desc, index asc), (n,4) f32 contiguous -> bool keep mask (n,)."""
    _need_gpu(boxes_sorted)
    n = boxes_sorted.shape[0]
    keep = torch.zeros((n,), dtype=torch.uint8, device=boxes_sorted.device)
    if n == 0:
        return keep.bool()
    b = boxes_sorted.contiguous().float()
    ws = torch.empty((_lib.load().sy11_nms_workspace_bytes(n) // 8,), dtype=torch.int64, device=b.device)
    call("sy11_nms_sorted", n, _p(b), float(iou_thres), _p(ws), _p(keep), _stream())
    return keep.bool()


def nms_sorted_batched(boxes_sorted: torch.Tensor, counts, iou_thres: float, max_keep: int, chunk_bytes: int = 2 << 30) -> torch.Tensor:
    """Greedy NMS of several images in one go: image i owns counts[i] consecutive rows of ``boxes_sorted`` ((total, 4) f32, each
    image's rows in score-descending order).  -> bool keep mask (total,), at most ``max_keep`` survivors per image.  The bit
    matrices of a launch are bounded by ``chunk_bytes`` (images are processed in as many launches as that takes)."""
    _need_gpu(boxes_sorted)
    total = boxes_sorted.shape[0]
    keep = torch.empty((total,), dtype=torch.uint8, device=boxes_sorted.device)
    if total == 0:
        return keep.bool()
    b = boxes_sorted.contiguous().float()
    lib = _lib.load()
    counts = [int(c) for c in counts]
    need = [c * ((c + 63) // 64) * 8 for c in counts]
    lo, row = 0, 0
    while lo < len(counts):
        hi, size = lo, 0
        while hi < len(counts) and (hi == lo or size + need[hi] <= chunk_bytes):
            size += need[hi]
            hi += 1
        n_rows = sum(counts[lo:hi])
        if n_rows:
            arr = (C.c_int32 * (hi - lo))(*counts[lo:hi])
            ws = torch.empty((max(size // 8, 1),), dtype=torch.int64, device=b.device)
            call("sy11_nms_sorted_batched", hi - lo, C.cast(arr, C.c_void_p), _p(b[row:row + n_rows]), float(iou_thres), int(max_keep), _p(ws),
                 _p(keep[row:row + n_rows]), _stream())
        row += n_rows
        lo = hi
    return keep.bool()


def nms_candidates(pred: torch.Tensor, nc: int, conf_thres: float, multi_label: bool, segment_by_class: bool = False, max_per_image: int = None,
                   class_ok: torch.Tensor = None):
    """Candidates of non_max_suppression from the (B, 4 + nc + nm, A) f32 prediction tensor, in the reference's order (image, anchor,
    class).  -> (key int64 (n,), anchor int32 (n,), class int32 (n,)) on the device, the per-image counts as a host list, and whether
    the keys are segmented by class: key = segment << 32 | ~bits(score), segment = image, or image * nc + class when
    ``segment_by_class`` is asked for AND no image has more than ``max_per_image`` candidates (the caller's `max_nms` cut is per image
    and by score, so it needs the image-wide order) AND the device flag ``class_ok`` (read with the counts) is non-zero.
    One host synchronisation (the counts)."""
    _need_gpu(pred)
    if pred.dtype != torch.float32 or not pred.is_contiguous():
        raise _lib.Sy11Error("nms_candidates: prediction must be a contiguous f32 (B, D, A) tensor")
    B, D, A = pred.shape
    nblk = (A + 255) // 256
    cnt = torch.empty((B, nblk), dtype=torch.int32, device=pred.device)
    call("sy11_nms_candidates", B, D, A, nc, float(conf_thres), 1 if multi_label else 0, 0, _p(pred), None, _p(cnt), None, None, None, _stream())
    incl = torch.cumsum(cnt.view(-1), 0, dtype=torch.int32)
    off = (incl - cnt.view(-1)).contiguous()
    per_image = cnt.sum(1, dtype=torch.int64)
    if class_ok is not None:
        per_image = torch.cat((per_image, class_ok.reshape(1).to(torch.int64)))
    per_image = per_image.tolist()                             # the one host read: sizes the outputs, and the caller's segment list
    ok = bool(per_image.pop()) if class_ok is not None else True
    total = sum(per_image)
    by_class = bool(segment_by_class) and ok and not (max_per_image is not None and per_image and max(per_image) > max_per_image)
    flags = (1 if multi_label else 0, 1 if by_class else 0)
    key = torch.empty((total,), dtype=torch.int64, device=pred.device)
    anchor = torch.empty((total,), dtype=torch.int32, device=pred.device)
    cls = torch.empty((total,), dtype=torch.int32, device=pred.device)
    if total:
        call("sy11_nms_candidates", B, D, A, nc, float(conf_thres), *flags, _p(pred), _p(off), None, _p(key), _p(anchor), _p(cls), _stream())
    return key, anchor, cls, per_image, by_class


def nms_sorted_segments(boxes_sorted: torch.Tensor, seg_of_row: torch.Tensor, nseg: int, iou_thres: float, max_keep: int) -> torch.Tensor:
    """Greedy NMS of ``nseg`` segments at once; ``seg_of_row`` (int64, non-decreasing) names the segment of every row of
    ``boxes_sorted`` ((n, 4) f32, a segment's rows in score-descending order).  -> bool keep mask (n,), at most ``max_keep``
    survivors per segment.  One host read (the longest segment and the workspace size)."""
    _need_gpu(boxes_sorted, seg_of_row)
    n = boxes_sorted.shape[0]
    keep = torch.zeros((n,), dtype=torch.uint8, device=boxes_sorted.device)
    if n == 0:
        return keep.bool()
    cnt = torch.bincount(seg_of_row, minlength=nseg)
    nw = (cnt + 63) // 64
    words = cnt * nw
    ws_end = torch.cumsum(words, 0)
    max_n, total_words = (int(v) for v in torch.stack((cnt.max(), ws_end[-1])).tolist())
    start = torch.zeros((nseg + 1,), dtype=torch.int32, device=boxes_sorted.device)
    start[1:] = torch.cumsum(cnt, 0)
    ws = (ws_end - words).contiguous()
    work = torch.empty((max(total_words, 1),), dtype=torch.int64, device=boxes_sorted.device)
    call("sy11_nms_sorted_segments", nseg, _p(start), _p(ws), max_n, _p(boxes_sorted.contiguous().float()), float(iou_thres), int(max_keep),
         _p(work), _p(keep), _stream())
    return keep.bool()


def stft_logmel(iq, window, mel_start, mel_w, n_fft, hop, n_frames, n_mel):
    """iq: (B, L) complex64 -> (db (B, frames, n_mel) f32, minmax (B, 2) f32)."""
    _need_gpu(iq, window, mel_start, mel_w)
    if iq.dtype != torch.complex64 or not iq.is_contiguous():
        raise _lib.Sy11Error("stft_logmel: iq must be contiguous complex64")
    # the tables go down as raw pointers: another dtype or a strided view would be reinterpreted, not converted
    if window.dtype != torch.float32 or tuple(window.shape) != (n_fft,) or not window.is_contiguous():
        raise _lib.Sy11Error(f"stft_logmel: `window` must be a contiguous f32 vector of n_fft = {n_fft} taps, got {window.dtype} {tuple(window.shape)}")
    if mel_start.dtype != torch.int32 or tuple(mel_start.shape) != (n_mel,) or not mel_start.is_contiguous():
        raise _lib.Sy11Error(f"stft_logmel: `mel_start` must be a contiguous int32 vector of n_mel = {n_mel} bins, got {mel_start.dtype} "
                             f"{tuple(mel_start.shape)}")
    if mel_w.dtype != torch.float32 or mel_w.dim() != 2 or mel_w.shape[0] != n_mel or mel_w.shape[1] < 1 or not mel_w.is_contiguous():
        raise _lib.Sy11Error(f"stft_logmel: `mel_w` must be a contiguous f32 (n_mel = {n_mel}, taps) matrix, got {mel_w.dtype} {tuple(mel_w.shape)}")
    B, L = iq.shape
    db = torch.empty((B, n_frames, n_mel), dtype=torch.float32, device=iq.device)
    mm = torch.empty((B, 2), dtype=torch.float32, device=iq.device)
    call("sy11_stft_minmax_init", B, _p(mm), _stream())
    call("sy11_stft_logmel", B, L, n_fft, hop, n_frames, n_mel, C.c_void_p(torch.view_as_real(iq).data_ptr()), _p(window),
         _p(mel_start), _p(mel_w), mel_w.shape[1], _p(db), _p(mm), _stream())
    return db, mm


def stft_normalize(db, mm, out=None):
    B, n_frames, n_mel = db.shape
    if out is not None and (tuple(out.shape) != (B, 3, n_mel, n_frames) or out.dtype != torch.float32 or not out.is_contiguous()
                            or out.device != db.device):
        raise _lib.Sy11Error("stft_normalize: `out` must be a contiguous f32 (B, 3, n_mel, n_frames) tensor on the same device")
    img = out if out is not None else torch.empty((B, 3, n_mel, n_frames), dtype=torch.float32, device=db.device)
    call("sy11_stft_normalize", B, n_mel, n_frames, _p(db), _p(mm), _p(img), _stream())
    return img


def stft_windows(db_strip, start, n_frames, out=None):
    """Windows of ``n_frames`` frames cut from one dB strip: ``db_strip`` (F, n_mel) f32 (``stft_logmel(...)[0][0]`` of one
    run of consecutive frames), ``start`` (W,) int32 on the device, relative to the strip's first frame ->
    (img (W, 3, n_mel, n_frames) f32 in [0, 1], minmax (W, 2) over exactly each window's rectangle)."""
    _need_gpu(db_strip, start)
    if db_strip.dim() != 2 or db_strip.dtype != torch.float32 or not db_strip.is_contiguous():
        raise _lib.Sy11Error("stft_windows: the strip must be a contiguous f32 (F, n_mel) tensor")
    if start.dtype != torch.int32 or start.dim() != 1 or not start.is_contiguous() or start.numel() == 0:
        raise _lib.Sy11Error("stft_windows: `start` must be a non-empty contiguous int32 vector")
    F, n_mel = db_strip.shape
    W = start.numel()
    if out is not None and (tuple(out.shape) != (W, 3, n_mel, n_frames) or out.dtype != torch.float32 or not out.is_contiguous()
                            or out.device != db_strip.device):
        raise _lib.Sy11Error("stft_windows: `out` must be a contiguous f32 (W, 3, n_mel, n_frames) tensor on the same device")
    img = out if out is not None else torch.empty((W, 3, n_mel, n_frames), dtype=torch.float32, device=db_strip.device)
    mm = torch.empty((W, 2), dtype=torch.float32, device=db_strip.device)
    fmm = torch.empty((F, 2), dtype=torch.float32, device=db_strip.device)
    call("sy11_stft_windows", F, n_mel, int(n_frames), W, _p(start), _p(db_strip), _p(mm), _p(fmm), _p(img), _stream())
    return img, mm


IQ_RECIPE = np.dtype([("dphi", "<u4"), ("phi0", "<u4"), ("gain", "<f4"), ("sigma", "<f4"), ("seed", "<u8"), ("src2", "<u8"), ("off2", "<i8"),
                      ("dphi2", "<u4"), ("phi02", "<u4"), ("gain2", "<f4"), ("flags", "<u4")])          # sy11_iq_recipe, 56 bytes


def iq_recipes(B):
    """B identity rows of the kernel's recipe table (gain 1, everything else off) as a numpy record array."""
    rec = np.zeros(B, dtype=IQ_RECIPE)
    rec["gain"], rec["gain2"] = 1.0, 1.0
    return rec


def iq_gather_augment(srcs, offs, L, rec=None, partners=None, out=None):
    """One launch: window ``b`` = ``L`` samples of ``srcs[b]`` (a 1-D contiguous complex64 device tensor: a resident capture or a
    staged copy) from sample ``offs[b]`` (may be odd), through row ``b`` of ``rec`` (``iq_recipes``; None = plain gather) ->
    (B, L) complex64.  ``partners[b]``: the capture row b's ``off2`` / ``dphi2`` / ``phi02`` / ``gain2`` refer to, or None (no mix; the
    ``src2`` field is filled in here).  Both windows are bounds-checked against their tensors before anything is launched; the two
    tables and the recipes travel to the device as ONE small copy."""
    B = len(srcs)
    if B == 0 or len(offs) != B or (partners is not None and len(partners) != B) or (rec is not None and (rec.dtype != IQ_RECIPE or rec.shape != (B,))):
        raise _lib.Sy11Error("iq_gather_augment: need one source, one offset, one recipe row (and one partner or None) per batch row")
    _need_gpu(*srcs)
    rec = iq_recipes(B) if rec is None else rec.copy()
    L = int(L)
    table = np.empty(B * (16 + IQ_RECIPE.itemsize), dtype=np.uint8)
    ptr, off = table[:8 * B].view(np.uint64), table[8 * B:16 * B].view(np.int64)
    for b in range(B):
        for what, t, o in (("source", srcs[b], int(offs[b])), ("partner", None if partners is None else partners[b], int(rec["off2"][b]))):
            if t is None:
                continue
            if t.dtype != torch.complex64 or t.dim() != 1 or not t.is_contiguous() or not t.is_cuda:
                raise _lib.Sy11Error(f"iq_gather_augment: {what} {b} must be a 1-D contiguous complex64 device tensor")
            if o < 0 or o + L > t.shape[0]:
                raise _lib.Sy11Error(f"iq_gather_augment: {what} {b}: samples [{o}, {o + L}) leave the capture ({t.shape[0]} samples)")
        ptr[b], off[b] = srcs[b].data_ptr(), int(offs[b])
        rec["src2"][b] = 0 if partners is None or partners[b] is None else partners[b].data_ptr()
    table[16 * B:] = rec.view(np.uint8)
    dev = srcs[0].device
    if out is not None and (tuple(out.shape) != (B, L) or out.dtype != torch.complex64 or not out.is_contiguous() or out.device != dev):
        raise _lib.Sy11Error("iq_gather_augment: `out` must be a contiguous complex64 (B, L) tensor on the sources' device")
    y = out if out is not None else torch.empty((B, L), dtype=torch.complex64, device=dev)
    t = torch.from_numpy(table).to(dev)
    base = t.data_ptr()
    call("sy11_iq_gather_augment", B, L, C.c_void_p(base), C.c_void_p(base + 8 * B), C.c_void_p(base + 16 * B),
         C.c_void_p(torch.view_as_real(y).data_ptr()), _stream())
    t.record_stream(torch.cuda.current_stream(dev))
    return y


def iq_resample(x, plan, n0, m0, M, out=None, n_total=None):
    """One launch of the DDC (sy11_iq_resample): outputs ``[m0, m0 + M)`` of the capture resampled / retuned by ``plan``
    (``sy11.data.resample.plan_resample``) -> (M,) complex64.  ``x``: 1-D contiguous complex64 device tensor holding the capture's
    samples ``[n0, n0 + len(x))`` (its base may be an odd sample of a larger tensor); ``n_total``: the capture's length (None: ``x`` is
    the whole capture and ``n0`` must be 0).  ``x`` must cover ``plan.support(m0, m0 + M)`` clipped to the capture — samples
    outside the capture are zeros, samples inside it are never assumed.  ``plan.identity`` returns the outputs' samples untouched."""
    _need_gpu(x, out)
    n0, m0, M = int(n0), int(m0), int(M)
    if x.dtype != torch.complex64 or x.dim() != 1 or not x.is_contiguous() or x.shape[0] == 0:
        raise _lib.Sy11Error("iq_resample: x must be a non-empty 1-D contiguous complex64 device tensor")
    n_in = x.shape[0]
    if n_total is None:
        if n0 != 0:
            raise _lib.Sy11Error("iq_resample: n0 != 0 needs the capture's length (n_total)")
        n_total = n_in
    n_total = int(n_total)
    if n0 < 0 or n0 + n_in > n_total:
        raise _lib.Sy11Error(f"iq_resample: samples [{n0}, {n0 + n_in}) leave the capture ({n_total} samples)")
    if M <= 0 or m0 < 0 or m0 + M > plan.n_out(n_total):
        raise _lib.Sy11Error(f"iq_resample: outputs [{m0}, {m0 + M}) are not among the capture's {plan.n_out(n_total)}")
    if M >= 2 ** 31 or n_in >= 2 ** 31:
        raise _lib.Sy11Error(f"iq_resample: M = {M} and n_in = {n_in} must stay below 2^31 per call")
    a, b = plan.support(m0, m0 + M)
    a, b = max(a, 0), min(b, n_total)
    if a < n0 or b > n0 + n_in:
        raise _lib.Sy11Error(f"iq_resample: outputs [{m0}, {m0 + M}) read samples [{a}, {b}); x holds [{n0}, {n0 + n_in})")
    if out is not None and (tuple(out.shape) != (M,) or out.dtype != torch.complex64 or not out.is_contiguous() or out.device != x.device):
        raise _lib.Sy11Error("iq_resample: `out` must be a contiguous complex64 (M,) tensor on x's device")
    if plan.identity:
        y = x[m0 - n0:m0 - n0 + M]
        return y if out is None else out.copy_(y)
    y = out if out is not None else torch.empty((M,), dtype=torch.complex64, device=x.device)
    call("sy11_iq_resample", plan.P, plan.Q, plan.T, plan.c, _p(plan.taps_on(x.device)), n0, n_in, C.c_void_p(torch.view_as_real(x).data_ptr()),
         plan.dphi, m0, M, C.c_void_p(torch.view_as_real(y).data_ptr()), _stream())
    return y


def iq_channelize(x, plan, n0, m0, M, out=None, n_total=None):
    """One launch of the polyphase filter bank (sy11_iq_channelize): time steps ``[m0, m0 + M)`` of every channel of the capture
    under ``plan`` (``sy11.data.channelize.plan_channels``) -> (K, M) complex64, channel-major.  ``x``, ``n0`` and ``n_total`` as in
    ``iq_resample``: ``x`` holds the capture's samples ``[n0, n0 + len(x))`` (its base may be an odd sample of a larger tensor) and
    must cover ``plan.support(m0, m0 + M)`` clipped to the capture; samples outside the capture are zeros."""
    _need_gpu(x, out)
    n0, m0, M = int(n0), int(m0), int(M)
    if x.dtype != torch.complex64 or x.dim() != 1 or not x.is_contiguous() or x.shape[0] == 0:
        raise _lib.Sy11Error("iq_channelize: x must be a non-empty 1-D contiguous complex64 device tensor")
    n_in = x.shape[0]
    if n_total is None:
        if n0 != 0:
            raise _lib.Sy11Error("iq_channelize: n0 != 0 needs the capture's length (n_total)")
        n_total = n_in
    n_total = int(n_total)
    if n0 < 0 or n0 + n_in > n_total:
        raise _lib.Sy11Error(f"iq_channelize: samples [{n0}, {n0 + n_in}) leave the capture ({n_total} samples)")
    if M <= 0 or m0 < 0 or m0 + M > plan.n_out(n_total):
        raise _lib.Sy11Error(f"iq_channelize: time steps [{m0}, {m0 + M}) are not among the capture's {plan.n_out(n_total)}")
    if M >= 2 ** 31 or n_in >= 2 ** 31:
        raise _lib.Sy11Error(f"iq_channelize: M = {M} and n_in = {n_in} must stay below 2^31 per call")
    a, b = plan.support(m0, m0 + M)
    a, b = max(a, 0), min(b, n_total)
    if a < n0 or b > n0 + n_in:
        raise _lib.Sy11Error(f"iq_channelize: time steps [{m0}, {m0 + M}) read samples [{a}, {b}); x holds [{n0}, {n0 + n_in})")
    if out is not None and (tuple(out.shape) != (plan.K, M) or out.dtype != torch.complex64 or not out.is_contiguous() or out.device != x.device):
        raise _lib.Sy11Error("iq_channelize: `out` must be a contiguous complex64 (K, M) tensor on x's device")
    y = out if out is not None else torch.empty((plan.K, M), dtype=torch.complex64, device=x.device)
    taps, twiddle = plan.on(x.device)
    call("sy11_iq_channelize", plan.K, plan.D, plan.N, plan.c, _p(taps), C.c_void_p(torch.view_as_real(twiddle).data_ptr()), n0, n_in,
         C.c_void_p(torch.view_as_real(x).data_ptr()), m0, M, M, C.c_void_p(torch.view_as_real(y).data_ptr()), _stream())
    return y


def iq_extract(x, n0, n_total, segments, taps, out):
    """One launch of the extraction kernel (sy11_iq_extract): every segment of ``segments`` — ``sy11.data.extract.SEGMENT`` records
    (m0, out_off, M, log2d, dphi): the outputs ``[m0, m0 + M)`` on the grid of decimation ``D = 2^log2d`` (output m = capture sample
    m D), mixed by ``dphi``, low-passed and decimated — is written to ``out[out_off : out_off + M]``.  ``x``, ``n0`` and ``n_total`` as in
    ``iq_resample``: ``x`` holds the capture's samples ``[n0, n0 + len(x))`` (its base may be an odd sample of a larger tensor) and must
    cover every segment's support clipped to the capture; samples outside the capture are zeros.  ``taps``: the device buffer of
    ``sy11.data.extract.taps_on``; ``out``: 1-D contiguous complex64 on x's device.  Each output is, bit for bit, what ``iq_resample``
    gives with ``plan_resample(fs, fs / D, shift)``.  -> ``out``."""
    from .data.extract import MAX_LOG2D, SEGMENT, taps_offset
    _need_gpu(x, taps, out)
    n0, n_total = int(n0), int(n_total)
    if x.dtype != torch.complex64 or x.dim() != 1 or not x.is_contiguous() or x.shape[0] == 0:
        raise _lib.Sy11Error("iq_extract: x must be a non-empty 1-D contiguous complex64 device tensor")
    n_in = x.shape[0]
    if n0 < 0 or n0 + n_in > n_total:
        raise _lib.Sy11Error(f"iq_extract: samples [{n0}, {n0 + n_in}) leave the capture ({n_total} samples)")
    if out.dtype != torch.complex64 or out.dim() != 1 or not out.is_contiguous() or out.device != x.device or out.shape[0] == 0:
        raise _lib.Sy11Error("iq_extract: `out` must be a non-empty 1-D contiguous complex64 tensor on x's device")
    if taps.dtype != torch.float32 or taps.dim() != 1 or not taps.is_contiguous() or taps.device != x.device \
            or taps.shape[0] != taps_offset(MAX_LOG2D + 1):
        raise _lib.Sy11Error(f"iq_extract: `taps` must be the {taps_offset(MAX_LOG2D + 1)}-float table of sy11.data.extract.taps_on on x's device")
    seg = np.ascontiguousarray(segments)
    if seg.dtype != SEGMENT or seg.ndim != 1 or seg.shape[0] == 0:
        raise _lib.Sy11Error("iq_extract: `segments` must be a non-empty 1-D array of sy11.data.extract.SEGMENT records")
    l, M, m0, off = seg["log2d"].astype(np.int64), seg["M"].astype(np.int64), seg["m0"], seg["out_off"]
    if (l < 0).any() or (l > MAX_LOG2D).any():
        raise _lib.Sy11Error(f"iq_extract: log2 D must lie in [0, {MAX_LOG2D}]")
    D = np.int64(1) << l
    if (M <= 0).any() or (m0 < 0).any() or (m0 >= 2 ** 48).any() or ((m0 + M - 1) * D >= n_total).any():
        k = int(np.flatnonzero((M <= 0) | (m0 < 0) | (m0 >= 2 ** 48) | ((m0 + M - 1) * D >= n_total))[0])
        raise _lib.Sy11Error(f"iq_extract: segment {k}: outputs [{int(m0[k])}, {int(m0[k] + M[k])}) at D = {int(D[k])} are not on the capture's "
                             f"{n_total} samples")
    if (off < 0).any() or (off + M > out.shape[0]).any():
        k = int(np.flatnonzero((off < 0) | (off + M > out.shape[0]))[0])
        raise _lib.Sy11Error(f"iq_extract: segment {k} writes [{int(off[k])}, {int(off[k] + M[k])}) of an output of {out.shape[0]} samples")
    a = np.where(l == 0, m0, np.maximum((m0 - 16) * D, 0))
    b = np.where(l == 0, m0 + M, np.minimum((m0 + M + 15) * D + 1, n_total))
    if (a < n0).any() or (b > n0 + n_in).any():
        k = int(np.flatnonzero((a < n0) | (b > n0 + n_in))[0])
        raise _lib.Sy11Error(f"iq_extract: segment {k} reads samples [{int(a[k])}, {int(b[k])}); x holds [{n0}, {n0 + n_in})")
    lib = _lib.load()
    tile = np.array([lib.sy11_iq_extract_tile(k) for k in range(MAX_LOG2D + 1)], dtype=np.int64)[l]
    count = -(-M // tile)                                      # the tile map: one (segment, first output) pair per workgroup
    n_tile = int(count.sum())
    if n_in >= 2 ** 31 or out.shape[0] >= 2 ** 31 or n_tile >= 2 ** 31 or seg.shape[0] >= 2 ** 31:
        raise _lib.Sy11Error(f"iq_extract: n_in = {n_in}, len(out) = {out.shape[0]} and the {n_tile} tiles must stay below 2^31 per call")
    tiles = np.empty((n_tile, 2), dtype=np.int32)
    tiles[:, 0] = np.repeat(np.arange(seg.shape[0]), count)
    tiles[:, 1] = (np.arange(n_tile) - np.repeat(np.cumsum(count) - count, count)) * np.repeat(tile, count)
    table = np.concatenate((seg.view(np.uint8), tiles.reshape(-1).view(np.uint8)))
    t = torch.from_numpy(table).to(x.device)
    call("sy11_iq_extract", seg.shape[0], C.c_void_p(table.ctypes.data), C.c_void_p(t.data_ptr()), n_tile,
         C.c_void_p(table.ctypes.data + seg.nbytes), C.c_void_p(t.data_ptr() + seg.nbytes), _p(taps), n_total, n0, n_in,
         C.c_void_p(torch.view_as_real(x).data_ptr()), out.shape[0], C.c_void_p(torch.view_as_real(out).data_ptr()), _stream())
    t.record_stream(torch.cuda.current_stream(x.device))
    return out


def iq_psd(x, n0, n_total, n_fft, items, window, twiddle, nw2, partial, env=None):
    """One launch of the Welch kernel (sy11_iq_psd): every item of ``items`` — ``sy11.data.measure.ITEM`` records (j0, env_off, nf, row,
    k_lo, k_hi): the frames ``[j0, j0 + nf)`` of one box, all of one group of ``sy11_iq_psd_group()`` frames — writes the sum of its
    frames' ``|X_j[k]|^2`` to row ``row`` of ``partial`` (rows, n_fft) f32 and, with ``env`` (1-D f32), the in-box power of each frame to
    ``env[env_off + (j - j0)]``.  ``x``, ``n0`` and ``n_total`` as in ``iq_extract``; frame j is the capture's samples
    ``[j n_fft / 2, j n_fft / 2 + n_fft)``.  ``window`` (n_fft,) f32, ``twiddle`` (n_fft / 2,) complex128 and ``nw2`` come from
    ``sy11.data.measure.tables_on``.  A refused call raises ``Sy11Error`` and writes nothing.  -> ``partial``."""
    from .data.measure import ITEM, N_FFT
    _need_gpu(x, window, twiddle, partial, env)
    n0, n_total, n_fft = int(n0), int(n_total), int(n_fft)
    if n_fft not in N_FFT:
        raise _lib.Sy11Error(f"iq_psd: n_fft must be one of {N_FFT}, got {n_fft}")
    if x.dtype != torch.complex64 or x.dim() != 1 or not x.is_contiguous() or x.shape[0] == 0:
        raise _lib.Sy11Error("iq_psd: x must be a non-empty 1-D contiguous complex64 device tensor")
    n_in = x.shape[0]
    if n0 < 0 or n0 + n_in > n_total:
        raise _lib.Sy11Error(f"iq_psd: samples [{n0}, {n0 + n_in}) leave the capture ({n_total} samples)")
    if partial.dtype != torch.float32 or partial.dim() != 2 or partial.shape[1] != n_fft or partial.shape[0] == 0 or not partial.is_contiguous() \
            or partial.device != x.device:
        raise _lib.Sy11Error(f"iq_psd: `partial` must be a non-empty contiguous (rows, {n_fft}) float32 tensor on x's device")
    if env is not None and (env.dtype != torch.float32 or env.dim() != 1 or env.shape[0] == 0 or not env.is_contiguous() or env.device != x.device):
        raise _lib.Sy11Error("iq_psd: `env` must be None or a non-empty 1-D contiguous float32 tensor on x's device")
    if window.dtype != torch.float32 or window.shape != (n_fft,) or not window.is_contiguous() or window.device != x.device \
            or twiddle.dtype != torch.complex128 or twiddle.shape != (n_fft // 2,) or not twiddle.is_contiguous() or twiddle.device != x.device:
        raise _lib.Sy11Error(f"iq_psd: `window` / `twiddle` must be the ({n_fft},) float32 and ({n_fft // 2},) complex128 tables on x's device")
    it = np.ascontiguousarray(items)
    if it.dtype != ITEM or it.ndim != 1 or it.shape[0] == 0:
        raise _lib.Sy11Error("iq_psd: `items` must be a non-empty 1-D array of sy11.data.measure.ITEM records")
    G, H = _lib.load().sy11_iq_psd_group(), n_fft // 2
    j0, nf, row = it["j0"], it["nf"].astype(np.int64), it["row"].astype(np.int64)
    bad = (nf < 1) | (nf > G) | (j0 < 0) | (j0 >= 2 ** 48) | (j0 // G != (j0 + nf - 1) // G)
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise _lib.Sy11Error(f"iq_psd: item {k}: frames [{int(j0[k])}, {int(j0[k] + nf[k])}) are not 1 .. {G} frames of one group")
    a, b = j0 * H, (j0 + nf - 1) * H + n_fft
    bad = (a < n0) | (b > n0 + n_in)
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise _lib.Sy11Error(f"iq_psd: item {k} reads samples [{int(a[k])}, {int(b[k])}); x holds [{n0}, {n0 + n_in})")
    bad = (row < 0) | (row >= partial.shape[0])
    if bad.any() or np.unique(row).shape[0] != row.shape[0]:
        k = int(np.flatnonzero(bad)[0]) if bad.any() else int(np.flatnonzero(np.bincount(row)[row] > 1)[0])
        raise _lib.Sy11Error(f"iq_psd: item {k} writes row {int(row[k])} of a partial table of {partial.shape[0]} rows (a row takes one item)")
    bad = (it["k_lo"] < -H) | (it["k_lo"] > it["k_hi"]) | (it["k_hi"] >= H)
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise _lib.Sy11Error(f"iq_psd: item {k}: bins [{int(it['k_lo'][k])}, {int(it['k_hi'][k])}] are not in [{-H}, {H})")
    if env is not None:
        bad = (it["env_off"] < 0) | (it["env_off"] + nf > env.shape[0])
        if bad.any():
            k = int(np.flatnonzero(bad)[0])
            raise _lib.Sy11Error(f"iq_psd: item {k} writes [{int(it['env_off'][k])}, {int(it['env_off'][k] + nf[k])}) of an envelope of "
                                 f"{env.shape[0]} values")
    if n_in >= 2 ** 31 or it.shape[0] >= 2 ** 31 or partial.shape[0] >= 2 ** 31:
        raise _lib.Sy11Error(f"iq_psd: n_in = {n_in}, the {it.shape[0]} items and the {partial.shape[0]} rows must stay below 2^31 per call")
    t = torch.from_numpy(it.view(np.uint8)).to(x.device)
    call("sy11_iq_psd", n_fft, it.shape[0], C.c_void_p(it.ctypes.data), C.c_void_p(t.data_ptr()), _p(window),
         C.c_void_p(torch.view_as_real(twiddle).data_ptr()), float(nw2), n_total, n0, n_in, C.c_void_p(torch.view_as_real(x).data_ptr()),
         partial.shape[0], _p(partial), 0 if env is None else env.shape[0], _p(env), _stream())
    t.record_stream(torch.cuda.current_stream(x.device))
    return partial


def psd_measure(partial, boxes, frac_lo, frac_hi):
    """The reduction of a measurement (sy11_psd_measure), one launch: ``partial`` (rows, n_fft) f32 as ``iq_psd`` filled it, ``boxes`` —
    ``sy11.data.measure.BOX`` records (row0, n_rows, k_lo, k_hi, s_lo, s_hi, noise_l, scale, corr) -> ``(psd, out_f, out_i)``: (k, n_fft)
    float64 in signed-bin order, (k, 4) float64 [p_in, noise_median, sum_c, sum_kc] and (k, 4) int32 [k_dn, k_up, n_in, n_noise], on the
    device; float64 throughout, in the orders of include/sy11.h.  A refused call raises ``Sy11Error`` and writes nothing."""
    from .data.measure import BOX, N_FFT
    _need_gpu(partial)
    if partial.dtype != torch.float32 or partial.dim() != 2 or partial.shape[1] not in N_FFT or partial.shape[0] == 0 or not partial.is_contiguous():
        raise _lib.Sy11Error(f"psd_measure: `partial` must be a non-empty contiguous (rows, n_fft) float32 device tensor, n_fft one of {N_FFT}")
    n_fft, H = partial.shape[1], partial.shape[1] // 2
    bx = np.ascontiguousarray(boxes)
    if bx.dtype != BOX or bx.ndim != 1 or bx.shape[0] == 0 or bx.shape[0] >= 2 ** 31:
        raise _lib.Sy11Error("psd_measure: `boxes` must be a non-empty 1-D array of sy11.data.measure.BOX records")
    frac_lo, frac_hi = float(frac_lo), float(frac_hi)
    if not 0.0 <= frac_lo <= frac_hi <= 1.0:
        raise _lib.Sy11Error(f"psd_measure: need 0 <= frac_lo <= frac_hi <= 1, got {frac_lo!r} / {frac_hi!r}")
    bad = (bx["n_rows"] < 1) | (bx["row0"] < 0) | (bx["row0"] + bx["n_rows"] > partial.shape[0])
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise _lib.Sy11Error(f"psd_measure: box {k} sums rows [{int(bx['row0'][k])}, {int(bx['row0'][k]) + int(bx['n_rows'][k])}) of a partial table "
                             f"of {partial.shape[0]} rows")
    bad = (bx["s_lo"] < -H) | (bx["s_lo"] > bx["k_lo"]) | (bx["k_lo"] > bx["k_hi"]) | (bx["k_hi"] > bx["s_hi"]) | (bx["s_hi"] >= H) \
        | (bx["noise_l"] < 0) | (bx["noise_l"] > H)
    if bad.any():
        raise _lib.Sy11Error(f"psd_measure: box {int(np.flatnonzero(bad)[0])}: need -N/2 <= s_lo <= k_lo <= k_hi <= s_hi < N/2 and 0 <= noise_l <= N/2")
    if not (np.isfinite(bx["scale"]).all() and np.isfinite(bx["corr"]).all() and (bx["scale"] > 0).all() and (bx["corr"] > 0).all()):
        raise _lib.Sy11Error("psd_measure: scale and corr must be positive and finite")
    dev, k = partial.device, bx.shape[0]
    psd = torch.empty((k, n_fft), dtype=torch.float64, device=dev)
    out_f = torch.empty((k, 4), dtype=torch.float64, device=dev)
    out_i = torch.empty((k, 4), dtype=torch.int32, device=dev)
    t = torch.from_numpy(bx.view(np.uint8)).to(dev)
    call("sy11_psd_measure", n_fft, k, C.c_void_p(bx.ctypes.data), C.c_void_p(t.data_ptr()), frac_lo, frac_hi, partial.shape[0], _p(partial),
         _p(psd), _p(out_f), _p(out_i), _stream())
    t.record_stream(torch.cuda.current_stream(dev))
    return psd, out_f, out_i


def iq_cyclo(x, n_fft, items, window, twiddle, partial, mom):
    """One launch of the characterisation kernel (sy11_iq_cyclo): every item of ``items`` — ``sy11.data.characterize.ITEM`` records (off, len,
    j0, nf, row, last): the frames ``[j0, j0 + nf)`` of the clip ``x[off : off + len]``, all of one group of ``sy11_iq_cyclo_group()`` frames
    — writes the sums of its frames' ``|FFT(w y_q)[k]|^2``, y = |x|^2, x^2, x^4, to ``partial[row]`` (rows, 3, n_fft) f32 and the sums of x^2
    (re, im), |x|^2 and |x|^4 over the samples it owns to ``mom[row]`` (rows, 4) f64.  ``x``: the packed clips (``Extraction.packed``),
    1-D contiguous complex64; a clip may start at an odd sample.  ``window`` / ``twiddle``: ``sy11.data.measure.tables_on``.  A refused call
    raises ``Sy11Error`` and writes nothing.  -> ``(partial, mom)``."""
    from .data.characterize import ITEM
    from .data.measure import N_FFT
    _need_gpu(x, window, twiddle, partial, mom)
    n_fft = int(n_fft)
    if n_fft not in N_FFT:
        raise _lib.Sy11Error(f"iq_cyclo: n_fft must be one of {N_FFT}, got {n_fft}")
    if x.dtype != torch.complex64 or x.dim() != 1 or not x.is_contiguous() or x.shape[0] == 0:
        raise _lib.Sy11Error("iq_cyclo: x must be a non-empty 1-D contiguous complex64 device tensor")
    n_in = x.shape[0]
    if partial.dtype != torch.float32 or partial.dim() != 3 or tuple(partial.shape[1:]) != (3, n_fft) or partial.shape[0] == 0 \
            or not partial.is_contiguous() or partial.device != x.device:
        raise _lib.Sy11Error(f"iq_cyclo: `partial` must be a non-empty contiguous (rows, 3, {n_fft}) float32 tensor on x's device")
    if mom.dtype != torch.float64 or tuple(mom.shape) != (partial.shape[0], 4) or not mom.is_contiguous() or mom.device != x.device:
        raise _lib.Sy11Error(f"iq_cyclo: `mom` must be a contiguous ({partial.shape[0]}, 4) float64 tensor on x's device")
    if window.dtype != torch.float32 or window.shape != (n_fft,) or not window.is_contiguous() or window.device != x.device \
            or twiddle.dtype != torch.complex128 or twiddle.shape != (n_fft // 2,) or not twiddle.is_contiguous() or twiddle.device != x.device:
        raise _lib.Sy11Error(f"iq_cyclo: `window` / `twiddle` must be the ({n_fft},) float32 and ({n_fft // 2},) complex128 tables on x's device")
    if x.data_ptr() % 8 or window.data_ptr() % 4 or twiddle.data_ptr() % 16 or partial.data_ptr() % 4 or mom.data_ptr() % 8:
        raise _lib.Sy11Error("iq_cyclo: x / mom must be 8-byte aligned, the twiddle table 16-byte, partial / window 4-byte")
    it = np.ascontiguousarray(items)
    if it.dtype != ITEM or it.ndim != 1 or it.shape[0] == 0:
        raise _lib.Sy11Error("iq_cyclo: `items` must be a non-empty 1-D array of sy11.data.characterize.ITEM records")
    if n_in >= 2 ** 31 or it.shape[0] >= 2 ** 31 or partial.shape[0] >= 2 ** 31:
        raise _lib.Sy11Error(f"iq_cyclo: len(x) = {n_in}, the {it.shape[0]} items and the {partial.shape[0]} rows must stay below 2^31 per call")
    G, H = _lib.load().sy11_iq_cyclo_group(), n_fft // 2
    off, ln, j0, nf, row = it["off"], it["len"], it["j0"].astype(np.int64), it["nf"].astype(np.int64), it["row"].astype(np.int64)
    bad = (off < 0) | (ln < n_fft) | (ln > n_in) | (off > n_in - ln)
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise _lib.Sy11Error(f"iq_cyclo: item {k}: the clip [{int(off[k])}, {int(off[k] + ln[k])}) is shorter than a frame or leaves the {n_in} "
                             f"packed samples")
    bad = (nf < 1) | (nf > G) | (j0 < 0) | (j0 // G != (j0 + nf - 1) // G)
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise _lib.Sy11Error(f"iq_cyclo: item {k}: frames [{int(j0[k])}, {int(j0[k] + nf[k])}) are not 1 .. {G} frames of one group")
    J = (ln - n_fft) // H + 1
    bad = j0 + nf > J
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise _lib.Sy11Error(f"iq_cyclo: item {k}: frames [{int(j0[k])}, {int(j0[k] + nf[k])}) leave the clip's {int(J[k])} frames")
    bad = (it["last"] != (j0 + nf == J))
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise _lib.Sy11Error(f"iq_cyclo: item {k}: last = {int(it['last'][k])}, but its frames end at {int(j0[k] + nf[k])} of the clip's {int(J[k])}")
    bad = (row < 0) | (row >= partial.shape[0])
    if bad.any() or np.unique(row).shape[0] != row.shape[0]:
        k = int(np.flatnonzero(bad)[0]) if bad.any() else int(np.flatnonzero(np.bincount(row)[row] > 1)[0])
        raise _lib.Sy11Error(f"iq_cyclo: item {k} writes row {int(row[k])} of a partial table of {partial.shape[0]} rows (a row takes one item)")
    t = torch.from_numpy(it.view(np.uint8)).to(x.device)
    call("sy11_iq_cyclo", n_fft, it.shape[0], C.c_void_p(it.ctypes.data), C.c_void_p(t.data_ptr()), _p(window),
         C.c_void_p(torch.view_as_real(twiddle).data_ptr()), n_in, C.c_void_p(torch.view_as_real(x).data_ptr()), partial.shape[0], _p(partial),
         _p(mom), _stream())
    t.record_stream(torch.cuda.current_stream(x.device))
    return partial, mom


CYCLO_OUT = 22                                                 # float64 per clip that sy11_cyclo_peaks writes (include/sy11.h)


def cyclo_peaks(partial, mom, rows, n_clip, spectra=None, out=None):
    """The reduction of a characterisation (sy11_cyclo_peaks), one launch: ``partial`` (rows, 3, n_fft) f32 and ``mom`` (rows, 4) f64 as
    ``iq_cyclo`` filled them, ``rows`` — ``sy11.data.characterize.ROW`` records (row0, n_rows, clip, k_min, reserved, scale), one per clip to
    reduce -> ``(spectra, out)``: (n_clip, 3, n_fft) float64 in signed-bin order and (n_clip, 22) float64 in the layout of include/sy11.h,
    on the device.  Given ``spectra`` / ``out`` are written in the rows that ``rows`` names and left alone elsewhere; fresh ones are filled
    with NaN first.  A refused call raises ``Sy11Error`` and writes nothing."""
    from .data.characterize import ROW
    from .data.measure import N_FFT
    _need_gpu(partial, mom, spectra, out)
    if partial.dtype != torch.float32 or partial.dim() != 3 or partial.shape[1] != 3 or partial.shape[2] not in N_FFT or partial.shape[0] == 0 \
            or not partial.is_contiguous():
        raise _lib.Sy11Error(f"cyclo_peaks: `partial` must be a non-empty contiguous (rows, 3, n_fft) float32 device tensor, n_fft one of {N_FFT}")
    n_fft, H, dev = partial.shape[2], partial.shape[2] // 2, partial.device
    if mom.dtype != torch.float64 or tuple(mom.shape) != (partial.shape[0], 4) or not mom.is_contiguous() or mom.device != dev:
        raise _lib.Sy11Error(f"cyclo_peaks: `mom` must be a contiguous ({partial.shape[0]}, 4) float64 tensor on partial's device")
    r = np.ascontiguousarray(rows)
    n_clip = int(n_clip)
    if r.dtype != ROW or r.ndim != 1 or r.shape[0] == 0 or r.shape[0] >= 2 ** 29 or not 0 < n_clip < 2 ** 31:
        raise _lib.Sy11Error("cyclo_peaks: `rows` must be a non-empty 1-D array of sy11.data.characterize.ROW records (below 2^29) and n_clip positive")
    for name, v, shape in (("spectra", spectra, (n_clip, 3, n_fft)), ("out", out, (n_clip, CYCLO_OUT))):
        if v is not None and (v.dtype != torch.float64 or tuple(v.shape) != shape or not v.is_contiguous() or v.device != dev):
            raise _lib.Sy11Error(f"cyclo_peaks: `{name}` must be None or a contiguous {shape} float64 tensor on partial's device")
    bad = (r["n_rows"] < 1) | (r["row0"] < 0) | (r["row0"] + r["n_rows"] > partial.shape[0])
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise _lib.Sy11Error(f"cyclo_peaks: clip {k} sums rows [{int(r['row0'][k])}, {int(r['row0'][k]) + int(r['n_rows'][k])}) of a partial table "
                             f"of {partial.shape[0]} rows")
    clip = r["clip"].astype(np.int64)
    bad = (clip < 0) | (clip >= n_clip)
    if bad.any() or np.unique(clip).shape[0] != clip.shape[0]:
        k = int(np.flatnonzero(bad)[0]) if bad.any() else int(np.flatnonzero(np.bincount(clip)[clip] > 1)[0])
        raise _lib.Sy11Error(f"cyclo_peaks: clip {k} writes output row {int(clip[k])} of {n_clip} (an output row takes one entry)")
    bad = (r["k_min"] < 1) | (r["k_min"] > H - 1)
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise _lib.Sy11Error(f"cyclo_peaks: clip {k}: the search range [{int(r['k_min'][k])}, {H - 1}] is empty or holds DC")
    if not (np.isfinite(r["scale"]).all() and (r["scale"] > 0).all()):
        raise _lib.Sy11Error("cyclo_peaks: scale must be positive and finite")
    if spectra is None:
        spectra = torch.full((n_clip, 3, n_fft), float("nan"), dtype=torch.float64, device=dev)
    if out is None:
        out = torch.full((n_clip, CYCLO_OUT), float("nan"), dtype=torch.float64, device=dev)
    t = torch.from_numpy(r.view(np.uint8)).to(dev)
    call("sy11_cyclo_peaks", n_fft, r.shape[0], C.c_void_p(r.ctypes.data), C.c_void_p(t.data_ptr()), partial.shape[0], _p(partial), _p(mom),
         n_clip, _p(spectra), _p(out), _stream())
    t.record_stream(torch.cuda.current_stream(dev))
    return spectra, out


def _first(bad):
    return int(np.flatnonzero(bad)[0])


def _one_item_per_row(what, row, n_rows):
    """Raise unless every entry of ``row`` is a row of the table and named once."""
    bad = (row < 0) | (row >= n_rows)
    if bad.any() or np.unique(row).shape[0] != row.shape[0]:
        k = _first(bad) if bad.any() else _first(np.bincount(row)[row] > 1)
        raise _lib.Sy11Error(f"{what}: item {k} writes row {int(row[k])} of a table of {n_rows} rows (a row takes one item)")


def _packed_c64(what, name, v, like=None):
    if v.dtype != torch.complex64 or v.dim() != 1 or not v.is_contiguous() or v.shape[0] == 0 or v.shape[0] >= 2 ** 31 or v.data_ptr() % 8 \
            or (like is not None and (v.device != like.device or v.shape != like.shape or v.data_ptr() == like.data_ptr())):
        raise _lib.Sy11Error(f"{what}: `{name}` must be a non-empty 1-D contiguous 8-byte aligned complex64 device tensor below 2^31"
                             + ("" if like is None else " of the input's length, on its device, and not the input itself"))


def _row_table(what, name, v, dev):
    if v.dtype != torch.float64 or v.dim() != 2 or v.shape[1] != 3 or v.shape[0] == 0 or v.shape[0] >= 2 ** 31 or not v.is_contiguous() or v.device != dev \
            or v.data_ptr() % 8:
        raise _lib.Sy11Error(f"{what}: `{name}` must be a non-empty contiguous (rows, 3) float64 tensor on the input's device")


def iq_demod_filter(x, items, taps, y, rows):
    """Launch 1 of the demodulation (sy11_iq_demod_filter): every item of ``items`` — ``sy11.data.demodulate.ITEM`` records (off, len, n0, tap_off,
    wc, ws, cnt, hw, n_taps, row, first, last): the tile ``[n0, n0 + cnt)`` of the usable span ``[hw, len - hw)`` of the clip ``x[off : off + len]`` —
    de-rotates by ``wc``, filters with ``taps[tap_off : tap_off + n_taps]`` into ``y`` (packed like ``x``) and writes the timing partials at ``ws`` to
    ``rows[row]`` (rows, 3) f64.  ``x``: the packed clips, 1-D contiguous complex64; a clip may start at an odd sample.  A refused call raises
    ``Sy11Error`` and writes nothing.  -> ``(y, rows)``."""
    from .data.demodulate import ITEM, MAX_TAPS
    what = "iq_demod_filter"
    _need_gpu(x, taps, y, rows)
    _packed_c64(what, "x", x)
    _packed_c64(what, "y", y, x)
    _row_table(what, "rows", rows, x.device)
    if taps.dtype != torch.float32 or taps.dim() != 1 or taps.shape[0] == 0 or taps.shape[0] >= 2 ** 31 or not taps.is_contiguous() or taps.device != x.device \
            or taps.data_ptr() % 4:
        raise _lib.Sy11Error(f"{what}: `taps` must be a non-empty 1-D contiguous float32 tensor on x's device")
    it = np.ascontiguousarray(items)
    if it.dtype != ITEM or it.ndim != 1 or it.shape[0] == 0 or it.shape[0] >= 2 ** 31:
        raise _lib.Sy11Error(f"{what}: `items` must be a non-empty 1-D array of sy11.data.demodulate.ITEM records")
    T, n_in, n_tap = _lib.load().sy11_iq_demod_tile(), x.shape[0], taps.shape[0]
    off, ln, n0, tap_off = it["off"], it["len"], it["n0"], it["tap_off"]
    cnt, hw, n_taps, row = (it[k].astype(np.int64) for k in ("cnt", "hw", "n_taps", "row"))
    bad = (off < 0) | (ln < 1) | (ln > n_in) | (off > n_in - ln)
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: item {k}: the clip [{int(off[k])}, {int(off[k] + ln[k])}) leaves the {n_in} packed samples")
    bad = (hw < 1) | (n_taps != 2 * hw + 1) | (n_taps > MAX_TAPS)
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: item {k}: {int(n_taps[k])} taps for a half width of {int(hw[k])} (odd, 2 hw + 1, at most {MAX_TAPS})")
    bad = (tap_off < 0) | (tap_off > n_tap - n_taps)
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: item {k}: taps [{int(tap_off[k])}, {int(tap_off[k] + n_taps[k])}) leave the {n_tap} packed taps")
    bad = (n0 < hw) | ((n0 - hw) % T != 0) | (cnt < 1) | (cnt > T) | (n0 > ln - hw - cnt)
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: item {k}: samples [{int(n0[k])}, {int(n0[k] + cnt[k])}) are not a tile of the usable span [{int(hw[k])}, {int(ln[k] - hw[k])})")
    bad = it["first"] != (n0 == hw)
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: item {k}: first = {int(it['first'][k])}, but it starts at {int(n0[k])} of the usable span from {int(hw[k])}")
    is_last = n0 + cnt == ln - hw
    bad = (it["last"] != is_last) | (~is_last & (cnt != T))
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: item {k}: last = {int(it['last'][k])} with {int(cnt[k])} samples, but it ends at {int(n0[k] + cnt[k])} of the usable span "
                             f"to {int(ln[k] - hw[k])}")
    _one_item_per_row(what, row, rows.shape[0])
    t = torch.from_numpy(it.view(np.uint8)).to(x.device)
    call("sy11_iq_demod_filter", it.shape[0], C.c_void_p(it.ctypes.data), C.c_void_p(t.data_ptr()), n_tap, _p(taps), n_in,
         C.c_void_p(torch.view_as_real(x).data_ptr()), C.c_void_p(torch.view_as_real(y).data_ptr()), rows.shape[0], _p(rows), _stream())
    t.record_stream(torch.cuda.current_stream(x.device))
    return y, rows


def demod_symbols(y, items, sym, rows):
    """Launch 2 of the demodulation (sy11_demod_symbols): every item of ``items`` — ``sy11.data.demodulate.BLOCK`` records (off, len, t0, step,
    sym_off, n, order, row, reserved): ``n`` (1 .. 256) symbols of the clip ``y[off : off + len]`` at the Q32.32 positions ``t0 + i step`` — writes the
    cubic interpolation of ``y`` at every position to ``sym[sym_off + i]`` and the sums of ``s^order`` (negated at order 4) and ``|s|^2`` to
    ``rows[row]`` (rows, 3) f64.  A refused call raises ``Sy11Error`` and writes nothing.  -> ``(sym, rows)``."""
    from .data.demodulate import BLOCK
    what = "demod_symbols"
    _need_gpu(y, sym, rows)
    _packed_c64(what, "y", y)
    _packed_c64(what, "sym", sym)
    if sym.device != y.device:
        raise _lib.Sy11Error(f"{what}: `sym` must be on y's device")
    _row_table(what, "rows", rows, y.device)
    it = np.ascontiguousarray(items)
    if it.dtype != BLOCK or it.ndim != 1 or it.shape[0] == 0 or it.shape[0] >= 2 ** 31:
        raise _lib.Sy11Error(f"{what}: `items` must be a non-empty 1-D array of sy11.data.demodulate.BLOCK records")
    n_in, n_sym = y.shape[0], sym.shape[0]
    off, ln, t0, step, sym_off = it["off"], it["len"], it["t0"], it["step"], it["sym_off"]
    n, order, row = (it[k].astype(np.int64) for k in ("n", "order", "row"))
    bad = (off < 0) | (ln < 4) | (ln > n_in) | (off > n_in - ln)
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: item {k}: the clip [{int(off[k])}, {int(off[k] + ln[k])}) leaves the {n_in} packed samples")
    bad = (n < 1) | (n > 256) | (sym_off < 0) | (sym_off > n_sym - n)
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: item {k}: symbols [{int(sym_off[k])}, {int(sym_off[k] + n[k])}) are not 1 .. 256 of the {n_sym} packed symbols")
    bad = (step < 2 ** 32) | (step > 2 ** 40) | (t0 < 2 ** 32) | (t0 >= ln * 2 ** 32)
    bad = bad | (((t0 + (n - 1) * np.where(bad, 0, step)) >> 32) > ln - 3)
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: item {k}: positions from {int(t0[k])} in steps of {int(step[k])} (Q32.32) leave [1, {int(ln[k]) - 3}]")
    bad = (order != 2) & (order != 4)
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: item {k}: order {int(order[k])} is not 2 or 4")
    _one_item_per_row(what, row, rows.shape[0])
    t = torch.from_numpy(it.view(np.uint8)).to(y.device)
    call("sy11_demod_symbols", it.shape[0], C.c_void_p(it.ctypes.data), C.c_void_p(t.data_ptr()), n_in, C.c_void_p(torch.view_as_real(y).data_ptr()),
         n_sym, C.c_void_p(torch.view_as_real(sym).data_ptr()), rows.shape[0], _p(rows), _stream())
    t.record_stream(torch.cuda.current_stream(y.device))
    return sym, rows


def demod_decide(sym, items, theta, r, d, rows):
    """Launch 3 of the demodulation (sy11_demod_decide): every item of ``items`` — ``sy11.data.demodulate.DEC`` records (sym_off, n_sym, row0, nb, b,
    block, order): block ``b`` of the ``nb`` blocks of ``block`` symbols of the clip ``sym[sym_off : sym_off + n_sym]`` — turns its symbols back by the
    phase interpolated from ``theta[row0 : row0 + nb]`` (float64, one per block, on the device) into ``r``, writes the decisions to ``d`` (uint8) and
    the sums of ``|r|^2``, ``Re(r conj(point(d)))`` and the count to ``rows[row0 + b]`` (rows, 3) f64.  A refused call raises ``Sy11Error`` and writes
    nothing.  -> ``(r, d, rows)``."""
    from .data.demodulate import DEC
    what = "demod_decide"
    _need_gpu(sym, theta, r, d, rows)
    _packed_c64(what, "sym", sym)
    _packed_c64(what, "r", r, sym)
    _row_table(what, "rows", rows, sym.device)
    if theta.dtype != torch.float64 or tuple(theta.shape) != (rows.shape[0],) or not theta.is_contiguous() or theta.device != sym.device or theta.data_ptr() % 8:
        raise _lib.Sy11Error(f"{what}: `theta` must be a contiguous ({rows.shape[0]},) float64 tensor on sym's device")
    if d.dtype != torch.uint8 or tuple(d.shape) != tuple(sym.shape) or not d.is_contiguous() or d.device != sym.device:
        raise _lib.Sy11Error(f"{what}: `d` must be a contiguous ({sym.shape[0]},) uint8 tensor on sym's device")
    it = np.ascontiguousarray(items)
    if it.dtype != DEC or it.ndim != 1 or it.shape[0] == 0 or it.shape[0] >= 2 ** 31:
        raise _lib.Sy11Error(f"{what}: `items` must be a non-empty 1-D array of sy11.data.demodulate.DEC records")
    n_sym, n_rows = sym.shape[0], rows.shape[0]
    sym_off, ns, row0 = it["sym_off"], it["n_sym"], it["row0"]
    nb, b, block, order = (it[k].astype(np.int64) for k in ("nb", "b", "block", "order"))
    bad = (ns < 1) | (sym_off < 0) | (sym_off > n_sym - ns)
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: item {k}: symbols [{int(sym_off[k])}, {int(sym_off[k] + ns[k])}) leave the {n_sym} packed symbols")
    bad = (block < 8) | (block > 256) | (nb < 1) | (b < 0) | (b >= nb)
    bad = bad | (nb != (ns + np.where(bad, 1, block) - 1) // np.where(bad, 1, block))
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: item {k}: block {int(b[k])} of {int(nb[k])} blocks of {int(block[k])} does not fit {int(ns[k])} symbols")
    bad = (row0 < 0) | (row0 > n_rows - nb)
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: item {k}: rows [{int(row0[k])}, {int(row0[k] + nb[k])}) leave a table of {n_rows} rows")
    bad = (order != 2) & (order != 4)
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: item {k}: order {int(order[k])} is not 2 or 4")
    _one_item_per_row(what, row0 + b, n_rows)
    t = torch.from_numpy(it.view(np.uint8)).to(sym.device)
    call("sy11_demod_decide", it.shape[0], C.c_void_p(it.ctypes.data), C.c_void_p(t.data_ptr()), n_sym, C.c_void_p(torch.view_as_real(sym).data_ptr()),
         n_rows, _p(theta), C.c_void_p(torch.view_as_real(r).data_ptr()), _p(d), _p(rows), _stream())
    t.record_stream(torch.cuda.current_stream(sym.device))
    return r, d, rows


def _packed_f32(what, name, v, dev, n=None):
    if v.dtype != torch.float32 or v.dim() != 1 or not v.is_contiguous() or v.shape[0] == 0 or v.shape[0] >= 2 ** 31 or v.data_ptr() % 4 or v.device != dev \
            or (n is not None and v.shape[0] != n):
        raise _lib.Sy11Error(f"{what}: `{name}` must be a non-empty 1-D contiguous float32 tensor below 2^31 on the input's device" + ("" if n is None else f" of {n} entries"))


def _rows_of(what, name, v, dev, width):
    if v.dtype != torch.float64 or v.dim() != 2 or v.shape[1] != width or v.shape[0] == 0 or v.shape[0] >= 2 ** 31 or not v.is_contiguous() or v.device != dev \
            or v.data_ptr() % 8:
        raise _lib.Sy11Error(f"{what}: `{name}` must be a non-empty contiguous (rows, {width}) float64 tensor on the input's device")


def iq_fsk_filter(x, items, taps, y, rows):
    """Launch 1 of the frequency-keyed demodulation (sy11_iq_fsk_filter): every item of ``items`` — ``sy11.data.demodulate_fsk.ITEM`` records (off, len,
    n0, tap_off, wc, ws, cnt, hw, n_taps, row, first, last): the tile ``[n0, n0 + cnt)`` of the usable span ``[hw + 1, len - hw)`` of the clip
    ``x[off : off + len]`` — takes the discriminator of its samples (turned back by ``wc``), filters it with ``taps[tap_off : tap_off + n_taps]`` into ``y``
    (float32, packed like ``x``) and writes the eight sums at ``ws`` to ``rows[row]`` (rows, 8) f64.  ``x``: the packed clips, 1-D contiguous complex64; a
    clip may start at an odd sample.  A refused call raises ``Sy11Error`` and writes nothing.  -> ``(y, rows)``."""
    from .data.demodulate import MAX_TAPS
    from .data.demodulate_fsk import ITEM
    what = "iq_fsk_filter"
    _need_gpu(x, taps, y, rows)
    _packed_c64(what, "x", x)
    _packed_f32(what, "y", y, x.device, x.shape[0])
    _rows_of(what, "rows", rows, x.device, 8)
    if taps.dtype != torch.float32 or taps.dim() != 1 or taps.shape[0] == 0 or taps.shape[0] >= 2 ** 31 or not taps.is_contiguous() or taps.device != x.device \
            or taps.data_ptr() % 4:
        raise _lib.Sy11Error(f"{what}: `taps` must be a non-empty 1-D contiguous float32 tensor on x's device")
    it = np.ascontiguousarray(items)
    if it.dtype != ITEM or it.ndim != 1 or it.shape[0] == 0 or it.shape[0] >= 2 ** 31:
        raise _lib.Sy11Error(f"{what}: `items` must be a non-empty 1-D array of sy11.data.demodulate_fsk.ITEM records")
    T, n_in, n_tap = _lib.load().sy11_iq_demod_tile(), x.shape[0], taps.shape[0]
    off, ln, n0, tap_off = it["off"], it["len"], it["n0"], it["tap_off"]
    cnt, hw, n_taps, row = (it[k].astype(np.int64) for k in ("cnt", "hw", "n_taps", "row"))
    bad = (off < 0) | (ln < 1) | (ln > n_in) | (off > n_in - ln)
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: item {k}: the clip [{int(off[k])}, {int(off[k] + ln[k])}) leaves the {n_in} packed samples")
    bad = (hw < 1) | (n_taps != 2 * hw + 1) | (n_taps > MAX_TAPS)
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: item {k}: {int(n_taps[k])} taps for a half width of {int(hw[k])} (odd, 2 hw + 1, at most {MAX_TAPS})")
    bad = (tap_off < 0) | (tap_off > n_tap - n_taps)
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: item {k}: taps [{int(tap_off[k])}, {int(tap_off[k] + n_taps[k])}) leave the {n_tap} packed taps")
    bad = (n0 < hw + 1) | ((n0 - hw - 1) % T != 0) | (cnt < 1) | (cnt > T) | (n0 > ln - hw - cnt)
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: item {k}: samples [{int(n0[k])}, {int(n0[k] + cnt[k])}) are not a tile of the usable span [{int(hw[k]) + 1}, {int(ln[k] - hw[k])})")
    bad = it["first"] != (n0 == hw + 1)
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: item {k}: first = {int(it['first'][k])}, but it starts at {int(n0[k])} of the usable span from {int(hw[k]) + 1}")
    is_last = n0 + cnt == ln - hw
    bad = (it["last"] != is_last) | (~is_last & (cnt != T))
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: item {k}: last = {int(it['last'][k])} with {int(cnt[k])} samples, but it ends at {int(n0[k] + cnt[k])} of the usable span "
                             f"to {int(ln[k] - hw[k])}")
    _one_item_per_row(what, row, rows.shape[0])
    t = torch.from_numpy(it.view(np.uint8)).to(x.device)
    call("sy11_iq_fsk_filter", it.shape[0], C.c_void_p(it.ctypes.data), C.c_void_p(t.data_ptr()), n_tap, _p(taps), n_in,
         C.c_void_p(torch.view_as_real(x).data_ptr()), _p(y), rows.shape[0], _p(rows), _stream())
    t.record_stream(torch.cuda.current_stream(x.device))
    return y, rows


def fsk_symbols(y, items, sym, rows):
    """Launch 2 of the frequency-keyed demodulation (sy11_fsk_symbols): every item of ``items`` — ``sy11.data.demodulate_fsk.BLOCK`` records (off, len, t0,
    step, sym_off, m, n, row): ``n`` (1 .. 256) symbols of the clip ``y[off : off + len]`` at the Q32.32 positions ``t0 + i step`` — writes the cubic
    interpolation of ``y`` (float32) at every position to ``sym[sym_off + i]`` (float32) and the count and sum of the symbols at or above ``m``, the sum
    of those below and the sum of squares to ``rows[row]`` (rows, 4) f64.  A refused call raises ``Sy11Error`` and writes nothing.  -> ``(sym, rows)``."""
    from .data.demodulate_fsk import BLOCK
    what = "fsk_symbols"
    _need_gpu(y, sym, rows)
    _packed_f32(what, "y", y, y.device)
    _packed_f32(what, "sym", sym, y.device)
    _rows_of(what, "rows", rows, y.device, 4)
    if sym.data_ptr() == y.data_ptr():
        raise _lib.Sy11Error(f"{what}: `sym` may not be y")
    it = np.ascontiguousarray(items)
    if it.dtype != BLOCK or it.ndim != 1 or it.shape[0] == 0 or it.shape[0] >= 2 ** 31:
        raise _lib.Sy11Error(f"{what}: `items` must be a non-empty 1-D array of sy11.data.demodulate_fsk.BLOCK records")
    n_in, n_sym = y.shape[0], sym.shape[0]
    off, ln, t0, step, sym_off = it["off"], it["len"], it["t0"], it["step"], it["sym_off"]
    n, row = (it[k].astype(np.int64) for k in ("n", "row"))
    bad = (off < 0) | (ln < 4) | (ln > n_in) | (off > n_in - ln)
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: item {k}: the clip [{int(off[k])}, {int(off[k] + ln[k])}) leaves the {n_in} packed samples")
    bad = (n < 1) | (n > 256) | (sym_off < 0) | (sym_off > n_sym - n)
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: item {k}: symbols [{int(sym_off[k])}, {int(sym_off[k] + n[k])}) are not 1 .. 256 of the {n_sym} packed symbols")
    bad = (step < 2 ** 32) | (step > 2 ** 40) | (t0 < 2 ** 32) | (t0 >= ln * 2 ** 32)
    bad = bad | (((t0 + (n - 1) * np.where(bad, 0, step)) >> 32) > ln - 3)
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: item {k}: positions from {int(t0[k])} in steps of {int(step[k])} (Q32.32) leave [1, {int(ln[k]) - 3}]")
    bad = ~np.isfinite(it["m"])
    if bad.any():
        raise _lib.Sy11Error(f"{what}: item {_first(bad)}: the mean m is not finite")
    _one_item_per_row(what, row, rows.shape[0])
    t = torch.from_numpy(it.view(np.uint8)).to(y.device)
    call("sy11_fsk_symbols", it.shape[0], C.c_void_p(it.ctypes.data), C.c_void_p(t.data_ptr()), n_in, _p(y), n_sym, _p(sym), rows.shape[0], _p(rows), _stream())
    t.record_stream(torch.cuda.current_stream(y.device))
    return sym, rows


def fsk_decide(sym, items, r, d, rows):
    """Launch 3 of the frequency-keyed demodulation (sy11_fsk_decide): every item of ``items`` — ``sy11.data.demodulate_fsk.DEC`` records (sym_off, f0, dev,
    n, row): ``n`` (1 .. 256) symbols from ``sym[sym_off]`` (float32) — writes ``(s - f0) / dev`` to ``r`` (complex64 of ``sym``'s length, the imaginary part
    zero), the decisions ``r < 0`` to ``d`` (uint8) and the sums of ``r^2``, ``|r|`` and the count to ``rows[row]`` (rows, 3) f64.  A refused call raises
    ``Sy11Error`` and writes nothing.  -> ``(r, d, rows)``."""
    from .data.demodulate_fsk import DEC
    what = "fsk_decide"
    _need_gpu(sym, r, d, rows)
    _packed_f32(what, "sym", sym, sym.device)
    _packed_c64(what, "r", r)
    if r.device != sym.device or r.shape != sym.shape:
        raise _lib.Sy11Error(f"{what}: `r` must be a ({sym.shape[0]},) complex64 tensor on sym's device")
    _row_table(what, "rows", rows, sym.device)
    if d.dtype != torch.uint8 or tuple(d.shape) != tuple(sym.shape) or not d.is_contiguous() or d.device != sym.device:
        raise _lib.Sy11Error(f"{what}: `d` must be a contiguous ({sym.shape[0]},) uint8 tensor on sym's device")
    it = np.ascontiguousarray(items)
    if it.dtype != DEC or it.ndim != 1 or it.shape[0] == 0 or it.shape[0] >= 2 ** 31:
        raise _lib.Sy11Error(f"{what}: `items` must be a non-empty 1-D array of sy11.data.demodulate_fsk.DEC records")
    n_sym, n_rows = sym.shape[0], rows.shape[0]
    sym_off, f0, dv = it["sym_off"], it["f0"], it["dev"]
    n, row = (it[k].astype(np.int64) for k in ("n", "row"))
    bad = (n < 1) | (n > 256) | (sym_off < 0) | (sym_off > n_sym - n)
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: item {k}: symbols [{int(sym_off[k])}, {int(sym_off[k] + n[k])}) are not 1 .. 256 of the {n_sym} packed symbols")
    bad = ~(np.isfinite(f0) & np.isfinite(dv) & (dv > 0))
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: item {k}: f0 = {float(f0[k])}, dev = {float(dv[k])}: both must be finite and dev positive")
    _one_item_per_row(what, row, n_rows)
    t = torch.from_numpy(it.view(np.uint8)).to(sym.device)
    call("sy11_fsk_decide", it.shape[0], C.c_void_p(it.ctypes.data), C.c_void_p(t.data_ptr()), n_sym, _p(sym), C.c_void_p(torch.view_as_real(r).data_ptr()),
         _p(d), n_rows, _p(rows), _stream())
    t.record_stream(torch.cuda.current_stream(sym.device))
    return r, d, rows


def _records(what, name, v, dtype):
    """``v`` as a non-empty contiguous 1-D array of ``dtype`` records; a ``ValueError`` otherwise."""
    it = np.ascontiguousarray(v)
    if it.dtype != dtype or it.ndim != 1 or it.shape[0] == 0 or it.shape[0] >= 2 ** 31:
        raise ValueError(f"{what}: `{name}` must be a non-empty 1-D array of sy11.data.demodulate_ofdm records {tuple(dtype.names)}")
    return it


def _flat(what, name, v, dtype, dev, like=None):
    if v.dtype != dtype or v.dim() != 1 or not v.is_contiguous() or v.shape[0] == 0 or v.shape[0] >= 2 ** 31 or v.device != dev or v.data_ptr() % 8 \
            or (like is not None and v.shape != like.shape):
        raise _lib.Sy11Error(f"{what}: `{name}` must be a non-empty 1-D contiguous 8-byte aligned {dtype} tensor below 2^31 on the input's device"
                             + ("" if like is None else f" of {like.shape[0]} entries"))


def iq_ofdm_fold(x, items, out):
    """Launch 1 of the OFDM demodulation (sy11_iq_ofdm_fold): every item of ``items`` — ``sy11.data.demodulate_ofdm.FOLD`` records (off, len, out_off, n_fft, S, r0, cnt_r, m0,
    cnt_m): the residues ``[r0, r0 + cnt_r)`` of the period ``S`` and the periods ``[m0, m0 + cnt_m)`` of the clip ``x[off : off + len]`` — writes per residue the sums of
    ``x[n + n_fft] conj(x[n])`` (Re, Im) and of the mean energy of the two samples to ``out[out_off + r - r0]`` (triples, 3) f64.  ``x``: the packed clips, 1-D contiguous
    complex64.  A table that is not one of ``FOLD`` records is a ``ValueError``; a call the library refuses raises ``Sy11Error`` and writes nothing.  -> ``out``."""
    from .data.demodulate_ofdm import FOLD
    what = "iq_ofdm_fold"
    _need_gpu(x, out)
    _packed_c64(what, "x", x)
    _rows_of(what, "out", out, x.device, 3)
    it = _records(what, "items", items, FOLD)
    t = torch.from_numpy(it.view(np.uint8)).to(x.device)
    call("sy11_iq_ofdm_fold", it.shape[0], C.c_void_p(it.ctypes.data), C.c_void_p(t.data_ptr()), x.shape[0], C.c_void_p(torch.view_as_real(x).data_ptr()), out.shape[0],
         _p(out), _stream())
    t.record_stream(torch.cuda.current_stream(x.device))
    return out


def ofdm_fft(x, items, bins, twiddle, yc, pilots, power):
    """Launch 2 of the OFDM demodulation (sy11_ofdm_fft): every item of ``items`` — ``sy11.data.demodulate_ofdm.FFT`` records (off, len, start, w, yc_off, pil_off, pow_off, n_fft,
    S, a, nf, bin_off, n_used, n_pil): ``nf`` (1 .. 1024 / n_fft) OFDM symbols of the clip ``x[off : off + len]``, the first FFT window at ``start`` — turns the samples back by
    ``w``, transforms them, turns carrier k by ``e^{2 pi i k a / n_fft}`` and writes, per OFDM symbol, the carriers ``bins[bin_off : bin_off + n_used]`` (``BIN`` records: k, pil) to
    ``yc`` (complex64), the pilots times their values to ``pilots`` (complex128) and the power of the used carriers to ``power`` (float64).  ``twiddle``: (512, 2) float64,
    ``e^{-2 pi i m / 1024}``.  A table that is not one of its records is a ``ValueError``; a call the library refuses raises ``Sy11Error`` and writes nothing.  -> the device copy of
    ``bins``."""
    from .data.demodulate_ofdm import BIN, FFT
    what = "ofdm_fft"
    _need_gpu(x, twiddle, yc, pilots, power)
    _packed_c64(what, "x", x)
    dev = x.device
    _flat(what, "yc", yc, torch.complex64, dev)
    _flat(what, "pilots", pilots, torch.complex128, dev)
    _flat(what, "power", power, torch.float64, dev)
    if twiddle.dtype != torch.float64 or tuple(twiddle.shape) != (512, 2) or not twiddle.is_contiguous() or twiddle.device != dev or twiddle.data_ptr() % 16 or pilots.data_ptr() % 16:
        raise _lib.Sy11Error(f"{what}: `twiddle` must be a contiguous (512, 2) float64 tensor on the input's device; it and `pilots` 16-byte aligned")
    it, bn = _records(what, "items", items, FFT), _records(what, "bins", bins, BIN)
    t, b = torch.from_numpy(it.view(np.uint8)).to(dev), torch.from_numpy(bn.view(np.uint8)).to(dev)
    call("sy11_ofdm_fft", it.shape[0], C.c_void_p(it.ctypes.data), C.c_void_p(t.data_ptr()), bn.shape[0], C.c_void_p(bn.ctypes.data), C.c_void_p(b.data_ptr()), _p(twiddle),
         x.shape[0], C.c_void_p(torch.view_as_real(x).data_ptr()), yc.shape[0], C.c_void_p(torch.view_as_real(yc).data_ptr()), pilots.shape[0],
         C.c_void_p(torch.view_as_real(pilots).data_ptr()), power.shape[0], _p(power), _stream())
    for v in (t, b):
        v.record_stream(torch.cuda.current_stream(dev))
    return b


def ofdm_decide(yc, items, cars, r, d, rows):
    """Launch 3 of the OFDM demodulation (sy11_ofdm_decide): every item of ``items`` — ``sy11.data.demodulate_ofdm.DEC`` records (yc_off, sym_off, rho_r, rho_i, car_off, n_data,
    n_used, order, row): one OFDM symbol, its ``n_used`` carrier values from ``yc[yc_off]`` — writes ``(yc[yc_off + idx] rho) tau`` for the data carriers
    ``cars[car_off : car_off + n_data]`` (``CAR`` records: idx, tr, ti) to ``r[sym_off ..]`` (complex64), the decisions at ``order`` to ``d`` (uint8) and the sums of ``|r|^2``,
    ``Re(r conj(point(d)))`` and the count to ``rows[row]`` (rows, 3) f64.  A table that is not one of its records is a ``ValueError``; a call the library refuses (a turn that is
    not finite among them) raises ``Sy11Error`` and writes nothing.  -> the device copy of ``cars``."""
    from .data.demodulate_ofdm import CAR, DEC
    what = "ofdm_decide"
    _need_gpu(yc, r, d, rows)
    dev = yc.device
    _flat(what, "yc", yc, torch.complex64, dev)
    _flat(what, "r", r, torch.complex64, dev)
    if d.dtype != torch.uint8 or tuple(d.shape) != tuple(r.shape) or not d.is_contiguous() or d.device != dev:
        raise _lib.Sy11Error(f"{what}: `d` must be a contiguous ({r.shape[0]},) uint8 tensor on yc's device")
    _row_table(what, "rows", rows, dev)
    if r.data_ptr() == yc.data_ptr():
        raise _lib.Sy11Error(f"{what}: `r` may not be yc")
    it, cr = _records(what, "items", items, DEC), _records(what, "cars", cars, CAR)
    t, c = torch.from_numpy(it.view(np.uint8)).to(dev), torch.from_numpy(cr.view(np.uint8)).to(dev)
    call("sy11_ofdm_decide", it.shape[0], C.c_void_p(it.ctypes.data), C.c_void_p(t.data_ptr()), cr.shape[0], C.c_void_p(cr.ctypes.data), C.c_void_p(c.data_ptr()), yc.shape[0],
         C.c_void_p(torch.view_as_real(yc).data_ptr()), r.shape[0], C.c_void_p(torch.view_as_real(r).data_ptr()), _p(d), rows.shape[0], _p(rows), _stream())
    for v in (t, c):
        v.record_stream(torch.cuda.current_stream(dev))
    return c


def _u8_vector(what, name, v, dev, n=None, exc=_lib.Sy11Error):
    if v.dtype != torch.uint8 or v.dim() != 1 or v.shape[0] == 0 or v.shape[0] >= 2 ** 31 or not v.is_contiguous() or v.device != dev \
            or (n is not None and v.shape[0] != n):
        raise exc(f"{what}: `{name}` must be a non-empty 1-D contiguous uint8 tensor on the symbols' device" + ("" if n is None else f" of {n} entries"))


def _sync_items(what, items, n_sym, n_word, n_pos):
    """The checks ``sync_correlate`` and ``sync_peaks`` share (the library repeats them) -> the contiguous ``ITEM`` table."""
    from .data.frames import ITEM, L_MAX, L_MIN
    it = np.ascontiguousarray(items)
    if it.dtype != ITEM or it.ndim != 1 or it.shape[0] == 0 or it.shape[0] >= 2 ** 31:
        raise _lib.Sy11Error(f"{what}: `items` must be a non-empty 1-D array of sy11.data.frames.ITEM records")
    T = _lib.load().sy11_sync_tile()
    sym_off, ns, word_off, pos_off, p0 = it["sym_off"], it["n_sym"], it["word_off"], it["pos_off"], it["p0"]
    cnt, L, order = (it[k].astype(np.int64) for k in ("cnt", "L", "order"))
    bad = (order != 2) & (order != 4)
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: item {k}: order {int(order[k])} is not 2 or 4")
    bad = (sym_off < 0) | (ns < 1) | (ns > n_sym) | (sym_off > n_sym - ns)
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: item {k}: the clip [{int(sym_off[k])}, {int(sym_off[k] + ns[k])}) leaves the {n_sym} packed symbols")
    bad = (L < L_MIN) | (L > L_MAX) | (L > ns)
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: item {k}: a word of {int(L[k])} symbols is not {L_MIN} .. {L_MAX} of a clip of {int(ns[k])}")
    bad = (word_off < 0) | (word_off > n_word - L)
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: item {k}: the word [{int(word_off[k])}, {int(word_off[k] + L[k])}) leaves the {n_word} packed word symbols")
    P = ns - L + 1
    bad = (p0 < 0) | (p0 % T != 0) | (cnt < 1) | (cnt > T) | (p0 > P - cnt) | ((cnt != T) & (p0 + cnt != P))
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: item {k}: positions [{int(p0[k])}, {int(p0[k] + cnt[k])}) are not a tile of [0, {int(P[k])})")
    bad = (pos_off < 0) | (pos_off > n_pos - P)
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: item {k}: positions [{int(pos_off[k])}, {int(pos_off[k] + P[k])}) leave the {n_pos} packed positions")
    a = pos_off + p0
    o = np.argsort(a, kind="stable")
    bad = (a + cnt)[o][:-1] > a[o][1:]
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: item {int(o[k + 1])} writes position {int(a[o][k + 1])}, which item {int(o[k])} of this call writes")
    return it


def sync_correlate(sym, items, words, rho2, q):
    """Launch 1 of the frame search (sy11_sync_correlate): every item of ``items`` — ``sy11.data.frames.ITEM`` records (sym_off, n_sym, word_off, pos_off,
    p0, cnt, L, order, reserved): the positions ``[p0, p0 + cnt)`` of the ``n_sym - L + 1`` of the clip ``sym[sym_off : sym_off + n_sym]`` against the word
    ``words[word_off : word_off + L]`` (uint8 decisions) — writes the squared normalised correlation to ``rho2[pos_off + p]`` (float64) and the rotation to
    ``q[pos_off + p]`` (uint8).  ``sym``: the packed corrected symbols, 1-D contiguous complex64.  A refused call raises ``Sy11Error`` and writes
    nothing.  -> ``(rho2, q)``."""
    what = "sync_correlate"
    _need_gpu(sym, words, rho2, q)
    _packed_c64(what, "sym", sym)
    _u8_vector(what, "words", words, sym.device)
    if rho2.dtype != torch.float64 or rho2.dim() != 1 or rho2.shape[0] == 0 or rho2.shape[0] >= 2 ** 31 or not rho2.is_contiguous() or rho2.device != sym.device \
            or rho2.data_ptr() % 8:
        raise _lib.Sy11Error(f"{what}: `rho2` must be a non-empty 1-D contiguous float64 tensor on the symbols' device")
    _u8_vector(what, "q", q, sym.device, rho2.shape[0])
    it = _sync_items(what, items, sym.shape[0], words.shape[0], rho2.shape[0])
    t = torch.from_numpy(it.view(np.uint8)).to(sym.device)
    call("sy11_sync_correlate", it.shape[0], C.c_void_p(it.ctypes.data), C.c_void_p(t.data_ptr()), words.shape[0], _p(words), sym.shape[0],
         C.c_void_p(torch.view_as_real(sym).data_ptr()), rho2.shape[0], _p(rho2), _p(q), _stream())
    t.record_stream(torch.cuda.current_stream(sym.device))
    return rho2, q


def sync_peaks(rho2, items, threshold2, hit, n_sym, n_word):
    """Launch 2 of the frame search (sy11_sync_peaks): over the item table of launch 1 (checked again, against ``n_sym`` symbols and ``n_word`` word
    symbols), ``hit[pos_off + p] = 1`` where ``rho2`` is at least ``threshold2`` (the SQUARED threshold, in (0, 1]), no earlier position within ``L - 1`` is at
    least as large and no later one within ``L - 1`` larger; else 0.  A refused call raises ``Sy11Error`` and writes nothing.  -> ``hit``."""
    what = "sync_peaks"
    _need_gpu(rho2, hit)
    if rho2.dtype != torch.float64 or rho2.dim() != 1 or rho2.shape[0] == 0 or rho2.shape[0] >= 2 ** 31 or not rho2.is_contiguous() or rho2.data_ptr() % 8:
        raise _lib.Sy11Error(f"{what}: `rho2` must be a non-empty 1-D contiguous float64 device tensor")
    _u8_vector(what, "hit", hit, rho2.device, rho2.shape[0])
    if isinstance(threshold2, bool) or not isinstance(threshold2, (int, float, np.integer, np.floating)) or not 0.0 < float(threshold2) <= 1.0:
        raise _lib.Sy11Error(f"{what}: the squared threshold {threshold2!r} is not in (0, 1]")
    n_sym, n_word = int(n_sym), int(n_word)
    if not (0 < n_sym < 2 ** 31 and 0 < n_word < 2 ** 31):
        raise _lib.Sy11Error(f"{what}: need symbols and word symbols, each below 2^31 (n_sym={n_sym} n_word={n_word})")
    it = _sync_items(what, items, n_sym, n_word, rho2.shape[0])
    t = torch.from_numpy(it.view(np.uint8)).to(rho2.device)
    call("sy11_sync_peaks", it.shape[0], C.c_void_p(it.ctypes.data), C.c_void_p(t.data_ptr()), n_word, n_sym, rho2.shape[0], _p(rho2), float(threshold2), _p(hit),
         _stream())
    t.record_stream(torch.cuda.current_stream(rho2.device))
    return hit


def sync_frames(sym, frames, words, rows, bits):
    """Launch 3 of the frame search (sy11_sync_frames): every frame of ``frames`` — ``sy11.data.frames.FRAME`` records (sym_off, n_sym, word_off, p, L,
    order, q, payload, row, reserved): the word ``words[word_off : word_off + L]`` at position ``p`` of the clip ``sym[sym_off : sym_off + n_sym]``, turned back
    by ``q`` steps of 2 pi / order — writes (errors, bit_errors, n_payload) to ``rows[row]`` (rows, 3) int32 and the packed payload bits, zero-padded, to
    ``bits[row]`` (rows, stride) uint8.  A refused call raises ``Sy11Error`` and writes nothing.  -> ``(rows, bits)``."""
    from .data.frames import FRAME, L_MAX, L_MIN, PAYLOAD_MAX
    what = "sync_frames"
    _need_gpu(sym, words, rows, bits)
    _packed_c64(what, "sym", sym)
    _u8_vector(what, "words", words, sym.device)
    if rows.dtype != torch.int32 or rows.dim() != 2 or rows.shape[1] != 3 or rows.shape[0] == 0 or rows.shape[0] >= 2 ** 31 or not rows.is_contiguous() \
            or rows.device != sym.device or rows.data_ptr() % 4:
        raise _lib.Sy11Error(f"{what}: `rows` must be a non-empty contiguous (rows, 3) int32 tensor on the symbols' device")
    if bits.dtype != torch.uint8 or bits.dim() != 2 or bits.shape[0] != rows.shape[0] or bits.shape[1] > PAYLOAD_MAX // 4 or not bits.is_contiguous() \
            or bits.device != sym.device:
        raise _lib.Sy11Error(f"{what}: `bits` must be a contiguous ({rows.shape[0]}, stride) uint8 tensor on the symbols' device, stride at most {PAYLOAD_MAX // 4}")
    fr = np.ascontiguousarray(frames)
    if fr.dtype != FRAME or fr.ndim != 1 or fr.shape[0] == 0 or fr.shape[0] >= 2 ** 31:
        raise _lib.Sy11Error(f"{what}: `frames` must be a non-empty 1-D array of sy11.data.frames.FRAME records")
    n_sym, n_word, n_rows, stride = sym.shape[0], words.shape[0], rows.shape[0], bits.shape[1]
    sym_off, ns, word_off, p = fr["sym_off"], fr["n_sym"], fr["word_off"], fr["p"]
    L, order, q, payload, row = (fr[k].astype(np.int64) for k in ("L", "order", "q", "payload", "row"))
    bad = (order != 2) & (order != 4)
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: frame {k}: order {int(order[k])} is not 2 or 4")
    bad = (q < 0) | (q >= order)
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: frame {k}: rotation {int(q[k])} is not below the order {int(order[k])}")
    bad = (sym_off < 0) | (ns < 1) | (ns > n_sym) | (sym_off > n_sym - ns)
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: frame {k}: the clip [{int(sym_off[k])}, {int(sym_off[k] + ns[k])}) leaves the {n_sym} packed symbols")
    bad = (L < L_MIN) | (L > L_MAX) | (L > ns)
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: frame {k}: a word of {int(L[k])} symbols is not {L_MIN} .. {L_MAX} of a clip of {int(ns[k])}")
    bad = (word_off < 0) | (word_off > n_word - L)
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: frame {k}: the word [{int(word_off[k])}, {int(word_off[k] + L[k])}) leaves the {n_word} packed word symbols")
    bad = (p < 0) | (p > ns - L)
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: frame {k}: the word at position {int(p[k])} ends after the clip's {int(ns[k])} symbols")
    bad = (payload < 0) | (payload >= PAYLOAD_MAX) | ((payload * (order // 2) + 7) // 8 > stride)
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: frame {k}: the bits of {int(payload[k])} payload symbols leave the {stride} bytes of a row")
    bad = (row < 0) | (row >= n_rows)
    if bad.any() or np.unique(row).shape[0] != row.shape[0]:
        k = _first(bad) if bad.any() else _first(np.bincount(row)[row] > 1)
        raise _lib.Sy11Error(f"{what}: frame {k} writes row {int(row[k])} of a table of {n_rows} rows (a row takes one frame)")
    t = torch.from_numpy(fr.view(np.uint8)).to(sym.device)
    call("sy11_sync_frames", fr.shape[0], C.c_void_p(fr.ctypes.data), C.c_void_p(t.data_ptr()), n_word, _p(words), n_sym,
         C.c_void_p(torch.view_as_real(sym).data_ptr()), n_rows, _p(rows), stride, _p(bits) if stride else None, _stream())
    t.record_stream(torch.cuda.current_stream(sym.device))
    return rows, bits


class EqRefused(_lib.Sy11Error, ValueError):
    """A refusal of ``eq_solve`` / ``eq_apply``, raised by the checks here or by the library's: a ``ValueError`` that is also the library's error."""


def _eq_call(name, *args):
    try:
        call(name, *args)
    except _lib.Sy11Error as e:
        raise EqRefused(str(e)) from None


def _eq_taps(what, taps):
    from .data.equalize import TAPS_MAX, TAPS_MIN
    if isinstance(taps, bool) or not isinstance(taps, (int, np.integer)) or not TAPS_MIN <= taps <= TAPS_MAX or taps % 2 == 0:
        raise EqRefused(f"{what}: {taps!r} taps are not an odd number in [{TAPS_MIN}, {TAPS_MAX}]")
    return int(taps)


def _eq_w(what, w, dev):
    from .data.equalize import TAPS_MAX
    if w.dtype != torch.complex128 or w.dim() != 2 or w.shape[1] != TAPS_MAX or w.shape[0] == 0 or w.shape[0] >= 2 ** 31 or not w.is_contiguous() or w.device != dev \
            or w.data_ptr() % 8:
        raise EqRefused(f"{what}: `w` must be a non-empty contiguous (rows, {TAPS_MAX}) complex128 tensor on the symbols' device")


def eq_solve(sym, frames, words, taps, reg, w, rows, decisions=None):
    """Launch 1 of the equaliser (sy11_eq_solve): every frame of ``frames`` — ``sy11.data.equalize.EQFRAME`` records (sym_off, n_sym, word_off, p, L, Lt, order, q,
    row, reserved, gain): the word ``words[word_off : word_off + L]`` at position ``p`` of the clip ``sym[sym_off : sym_off + n_sym]``, found at rotation ``q`` — writes the
    ``taps`` least-squares taps to ``w[row]`` (rows, 15) complex128, zero-padded, and (mse_before, mse_after, pivot_min, ok) to ``rows[row]`` (rows, 4) float64.  The
    training symbols from ``L`` to ``Lt`` take their targets from ``decisions`` (uint8, laid out as ``sym``: what ``eq_apply`` wrote).  A refused call raises a
    ``ValueError`` and writes nothing.  -> ``(w, rows)``."""
    from .data.equalize import EQFRAME, L_MAX, LT_MAX
    what = "eq_solve"
    _need_gpu(sym, words, w, rows)
    if sym.dtype != torch.complex64 or sym.dim() != 1 or not sym.is_contiguous() or sym.shape[0] == 0 or sym.shape[0] >= 2 ** 31 or sym.data_ptr() % 8:
        raise EqRefused(f"{what}: `sym` must be a non-empty 1-D contiguous 8-byte aligned complex64 device tensor below 2^31")
    dev = sym.device
    if words.dtype != torch.uint8 or words.dim() != 1 or words.shape[0] == 0 or words.shape[0] >= 2 ** 31 or not words.is_contiguous() or words.device != dev:
        raise EqRefused(f"{what}: `words` must be a non-empty 1-D contiguous uint8 tensor on the symbols' device")
    taps = _eq_taps(what, taps)
    if isinstance(reg, bool) or not isinstance(reg, (int, float, np.integer, np.floating)) or not 0.0 <= float(reg) <= 1.0:
        raise EqRefused(f"{what}: reg = {reg!r} is not in [0, 1]")
    _eq_w(what, w, dev)
    if rows.dtype != torch.float64 or rows.dim() != 2 or tuple(rows.shape) != (w.shape[0], 4) or not rows.is_contiguous() or rows.device != dev or rows.data_ptr() % 8:
        raise EqRefused(f"{what}: `rows` must be a contiguous ({w.shape[0]}, 4) float64 tensor on the symbols' device")
    if decisions is not None and (decisions.dtype != torch.uint8 or tuple(decisions.shape) != tuple(sym.shape) or not decisions.is_contiguous() or decisions.device != dev):
        raise EqRefused(f"{what}: `decisions` must be a contiguous ({sym.shape[0]},) uint8 tensor on the symbols' device")
    fr = np.ascontiguousarray(frames)
    if fr.dtype != EQFRAME or fr.ndim != 1 or fr.shape[0] == 0 or fr.shape[0] >= 2 ** 31:
        raise EqRefused(f"{what}: `frames` must be a non-empty 1-D array of sy11.data.equalize.EQFRAME records")
    n_sym, n_word, n_rows = sym.shape[0], words.shape[0], w.shape[0]
    sym_off, ns, word_off, p, gain = fr["sym_off"], fr["n_sym"], fr["word_off"], fr["p"], fr["gain"]
    L, Lt, order, q, row = (fr[k].astype(np.int64) for k in ("L", "Lt", "order", "q", "row"))
    bad = (order != 2) & (order != 4)
    if bad.any():
        k = _first(bad)
        raise EqRefused(f"{what}: frame {k}: order {int(order[k])} is not 2 or 4")
    bad = (q < 0) | (q >= order)
    if bad.any():
        k = _first(bad)
        raise EqRefused(f"{what}: frame {k}: rotation {int(q[k])} is not below the order {int(order[k])}")
    bad = (sym_off < 0) | (ns < 1) | (ns > n_sym) | (sym_off > n_sym - ns)
    if bad.any():
        k = _first(bad)
        raise EqRefused(f"{what}: frame {k}: the clip [{int(sym_off[k])}, {int(sym_off[k] + ns[k])}) leaves the {n_sym} packed symbols")
    bad = (L < 1) | (L > L_MAX) | (Lt < L) | (Lt > LT_MAX)
    if bad.any():
        k = _first(bad)
        raise EqRefused(f"{what}: frame {k}: a word of {int(L[k])} and {int(Lt[k])} training symbols are not 1 .. {L_MAX} and word .. {LT_MAX}")
    bad = (word_off < 0) | (word_off > n_word - L)
    if bad.any():
        k = _first(bad)
        raise EqRefused(f"{what}: frame {k}: the word [{int(word_off[k])}, {int(word_off[k] + L[k])}) leaves the {n_word} packed word symbols")
    bad = (p < 0) | (p > ns - Lt)
    if bad.any():
        k = _first(bad)
        raise EqRefused(f"{what}: frame {k}: {int(Lt[k])} training symbols at position {int(p[k])} end after the clip's {int(ns[k])} symbols")
    bad = (Lt != L) & (decisions is None)
    if bad.any():
        k = _first(bad)
        raise EqRefused(f"{what}: frame {k} trains on {int(Lt[k] - L[k])} symbols beyond its word, but the decisions are null")
    with np.errstate(invalid="ignore"):
        bad = ~(np.isfinite(gain) & (gain > 0))
    if bad.any():
        k = _first(bad)
        raise EqRefused(f"{what}: frame {k}: the gain {float(gain[k])} is not finite and positive")
    bad = (row < 0) | (row >= n_rows)
    if bad.any() or np.unique(row).shape[0] != row.shape[0]:
        k = _first(bad) if bad.any() else _first(np.bincount(row)[row] > 1)
        raise EqRefused(f"{what}: frame {k} writes row {int(row[k])} of a table of {n_rows} rows (a row takes one frame)")
    t = torch.from_numpy(fr.view(np.uint8)).to(dev)
    _eq_call("sy11_eq_solve", fr.shape[0], C.c_void_p(fr.ctypes.data), C.c_void_p(t.data_ptr()), taps, float(reg), n_word, _p(words), n_sym,
             C.c_void_p(torch.view_as_real(sym).data_ptr()), None if decisions is None else _p(decisions), n_rows, C.c_void_p(torch.view_as_real(w).data_ptr()), _p(rows),
             _stream())
    t.record_stream(torch.cuda.current_stream(dev))
    return w, rows


def eq_apply(sym, items, segments, taps, w, out, decisions):
    """Launch 2 of the equaliser (sy11_eq_apply): every item of ``items`` — ``sy11.data.equalize.EQITEM`` records (seg, tile): tile ``tile`` of the symbols ``[start, end)`` of
    the clip ``sym[sym_off : sym_off + n_sym]`` that ``segments[seg]`` (``EQSEGMENT`` records: sym_off, n_sym, start, end, frame, order) names — writes the symbols filtered by
    the ``taps`` taps ``w[frame]``, or copied bit for bit where ``frame`` is -1, to ``out`` (laid out as ``sym``) and their decisions to ``decisions`` (uint8).  A refused call
    raises a ``ValueError`` and writes nothing.  -> ``(out, decisions)``."""
    from .data.equalize import EQITEM, EQSEGMENT
    what = "eq_apply"
    _need_gpu(sym, w, out, decisions)
    if sym.dtype != torch.complex64 or sym.dim() != 1 or not sym.is_contiguous() or sym.shape[0] == 0 or sym.shape[0] >= 2 ** 31 or sym.data_ptr() % 8:
        raise EqRefused(f"{what}: `sym` must be a non-empty 1-D contiguous 8-byte aligned complex64 device tensor below 2^31")
    dev = sym.device
    if out.dtype != torch.complex64 or tuple(out.shape) != tuple(sym.shape) or not out.is_contiguous() or out.device != dev or out.data_ptr() % 8 or out.data_ptr() == sym.data_ptr():
        raise EqRefused(f"{what}: `out` must be a contiguous 8-byte aligned complex64 tensor of the symbols' length, on their device, and not the symbols themselves")
    if decisions.dtype != torch.uint8 or tuple(decisions.shape) != tuple(sym.shape) or not decisions.is_contiguous() or decisions.device != dev:
        raise EqRefused(f"{what}: `decisions` must be a contiguous ({sym.shape[0]},) uint8 tensor on the symbols' device")
    taps = _eq_taps(what, taps)
    _eq_w(what, w, dev)
    sg, it = np.ascontiguousarray(segments), np.ascontiguousarray(items)
    if sg.dtype != EQSEGMENT or sg.ndim != 1 or sg.shape[0] == 0 or sg.shape[0] >= 2 ** 31:
        raise EqRefused(f"{what}: `segments` must be a non-empty 1-D array of sy11.data.equalize.EQSEGMENT records")
    if it.dtype != EQITEM or it.ndim != 1 or it.shape[0] == 0 or it.shape[0] >= 2 ** 31:
        raise EqRefused(f"{what}: `items` must be a non-empty 1-D array of sy11.data.equalize.EQITEM records")
    T, n_sym, n_rows = _lib.load().sy11_eq_tile(), sym.shape[0], w.shape[0]
    sym_off, ns, start, end = sg["sym_off"], sg["n_sym"], sg["start"], sg["end"]
    frame, order = sg["frame"].astype(np.int64), sg["order"].astype(np.int64)
    bad = (order != 2) & (order != 4)
    if bad.any():
        k = _first(bad)
        raise EqRefused(f"{what}: segment {k}: order {int(order[k])} is not 2 or 4")
    bad = (sym_off < 0) | (ns < 1) | (ns > n_sym) | (sym_off > n_sym - ns)
    if bad.any():
        k = _first(bad)
        raise EqRefused(f"{what}: segment {k}: the clip [{int(sym_off[k])}, {int(sym_off[k] + ns[k])}) leaves the {n_sym} packed symbols")
    bad = (start < 0) | (start >= end) | (end > ns)
    if bad.any():
        k = _first(bad)
        raise EqRefused(f"{what}: segment {k}: symbols [{int(start[k])}, {int(end[k])}) are not inside the clip's {int(ns[k])}")
    bad = (frame < -1) | (frame >= n_rows)
    if bad.any():
        k = _first(bad)
        raise EqRefused(f"{what}: segment {k}: owner {int(frame[k])} is not -1 or a row of the {n_rows} of w")
    a = sym_off + start
    o = np.argsort(a, kind="stable")
    bad = (sym_off + end)[o][:-1] > a[o][1:]
    if bad.any():
        k = _first(bad)
        raise EqRefused(f"{what}: segment {int(o[k + 1])} writes symbol {int(a[o][k + 1])}, which segment {int(o[k])} of this call writes")
    seg, tile = it["seg"].astype(np.int64), it["tile"].astype(np.int64)
    bad = (seg < 0) | (seg >= sg.shape[0])
    if bad.any():
        k = _first(bad)
        raise EqRefused(f"{what}: item {k}: segment {int(seg[k])} is not one of the {sg.shape[0]}")
    bad = (tile < 0) | (tile * T >= (end - start)[seg])
    if bad.any():
        k = _first(bad)
        raise EqRefused(f"{what}: item {k}: tile {int(tile[k])} is not one of segment {int(seg[k])}'s {int((end - start)[seg[k]])} symbols")
    a = a[seg] + tile * T
    if np.unique(a).shape[0] != a.shape[0]:
        o = np.argsort(a, kind="stable")
        k = _first(a[o][1:] == a[o][:-1])
        raise EqRefused(f"{what}: item {int(o[k + 1])} writes symbol {int(a[o][k + 1])}, which item {int(o[k])} of this call writes")
    ts, ti = torch.from_numpy(sg.view(np.uint8)).to(dev), torch.from_numpy(it.view(np.uint8)).to(dev)
    _eq_call("sy11_eq_apply", it.shape[0], C.c_void_p(it.ctypes.data), C.c_void_p(ti.data_ptr()), sg.shape[0], C.c_void_p(sg.ctypes.data), C.c_void_p(ts.data_ptr()), taps,
             n_rows, C.c_void_p(torch.view_as_real(w).data_ptr()), n_sym, C.c_void_p(torch.view_as_real(sym).data_ptr()),
             C.c_void_p(torch.view_as_real(out).data_ptr()), _p(decisions), _stream())
    ts.record_stream(torch.cuda.current_stream(dev))
    ti.record_stream(torch.cuda.current_stream(dev))
    return out, decisions


def _fec_table(what, name, t, dtype, dev, n_rows=None, width=None, lo=1, hi=None, even=False):
    """A contiguous (rows, stride) device table of ``dtype``; ``width``: the exact stride, else ``lo <= stride <= hi``."""
    bad = t.dtype != dtype or t.dim() != 2 or t.shape[0] == 0 or t.shape[0] >= 2 ** 31 or not t.is_contiguous() or t.device != dev \
        or (n_rows is not None and t.shape[0] != n_rows)
    if not bad:
        s = t.shape[1]
        bad = s != width if width is not None else (s < lo or s > hi or (even and s % 2 == 1))
    if bad or t.data_ptr() % {torch.int32: 4, torch.int8: 2, torch.uint8: 1}[dtype]:
        raise _lib.Sy11Error(f"{what}: `{name}` must be a non-empty contiguous (rows, stride) {dtype} tensor on the other tensors' device" +
                             (f", stride {width}" if width is not None else f", {'an even ' if even else ''}stride in [{lo}, {hi}]") +
                             ("" if n_rows is None else f", of {n_rows} rows"))


def _fec_frames(what, frames, n_rows):
    """The checks the three launches of the frame decoder share (the library repeats them) -> the contiguous ``FECFRAME`` table."""
    from .data.decode import FECFRAME, K
    fr = np.ascontiguousarray(frames)
    if fr.dtype != FECFRAME or fr.ndim != 1 or fr.shape[0] == 0 or fr.shape[0] >= 2 ** 31:
        raise _lib.Sy11Error(f"{what}: `frames` must be a non-empty 1-D array of sy11.data.decode.FECFRAME records")
    T_MAX = _lib.load().sy11_fec_tmax()
    T, order, q, tail, row = (fr[k].astype(np.int64) for k in ("T", "order", "q", "tail", "row"))
    bad = (order != 2) & (order != 4)
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: frame {k}: order {int(order[k])} is not 2 or 4")
    bad = (q < 0) | (q >= order)
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: frame {k}: rotation {int(q[k])} is not below the order {int(order[k])}")
    bad = (tail != 0) & (tail != 1)
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: frame {k}: tail {int(tail[k])} is not 0 or 1")
    bad = (T < np.where(tail == 1, K, 1)) | (T > T_MAX)
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: frame {k}: {int(T[k])} trellis steps are not {K if tail[k] else 1} .. {T_MAX}")
    bad = (row < 0) | (row >= n_rows)
    if bad.any() or np.unique(row).shape[0] != row.shape[0]:
        k = _first(bad) if bad.any() else _first(np.bincount(row)[row] > 1)
        raise _lib.Sy11Error(f"{what}: frame {k} writes row {int(row[k])} of a table of {n_rows} rows (a row takes one frame)")
    return fr


def _fec_polys(what, polys):
    try:
        g = tuple(polys)
    except TypeError:
        g = ()
    if len(g) != 2 or not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) and 0 <= v < 128 and (v & 0x41) == 0x41 for v in g):
        raise _lib.Sy11Error(f"{what}: the generators {polys!r} are not two 7-bit integers with bits 6 and 0 set")
    return int(g[0]), int(g[1])


def _fec_fit(what, fr, stride_soft, stride_bits=None):
    bad = 2 * fr["T"].astype(np.int64) > stride_soft
    if stride_bits is not None:
        bad |= (fr["T"].astype(np.int64) + 7) // 8 > stride_bits
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: frame {k}: {int(fr['T'][k])} steps leave a row of {stride_soft} soft bytes" + ("" if stride_bits is None else f" or {stride_bits} bit bytes"))


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _crc_arg(what, crc, n_bits, whole_bytes, exc):
    """The ``crc`` of a check launch over ``n_bits`` information bits: None, or a dict width / poly / init / refin / refout / xorout of 8 .. 32 bits (``whole_bytes``, the
    byte-serial check: 8, 16, 24 or 32) -> the ``FecCrc``, checked as the library checks it (csrc/frame_check.h).  A refusal raises ``exc``."""
    if crc is None:
        return _lib.FecCrc()
    try:
        W, poly, init, xorout, refin, refout = (int(crc[k]) for k in ("width", "poly", "init", "xorout", "refin", "refout"))
    except (KeyError, TypeError, ValueError):
        raise exc(f"{what}: `crc` must be None or a dict of width, poly, init, refin, refout and xorout") from None
    if W not in ((8, 16, 24, 32) if whole_bytes else range(8, 33)) or n_bits <= W or not all(0 <= v < 2 ** W for v in (poly, init, xorout)) or refin not in (0, 1) \
            or refout not in (0, 1) or (refin and (n_bits - W) % 8):
        raise exc(f"{what}: the crc {crc!r} is not of {'8, 16, 24 or 32' if whole_bytes else '8 .. 32'} bits below the {n_bits} information bits, with fields of that width "
                  f"(and whole bytes with refin)")
    return _lib.FecCrc(W, poly, init, xorout, refin, refout)


def _frame_rows(what, frames, n_rows):
    """The rows the frames of a launch read, each inside the tables of ``n_rows`` rows and named once -> the contiguous int32 table."""
    fr = np.asarray(frames)
    if fr.ndim != 1 or fr.shape[0] == 0 or fr.shape[0] >= 2 ** 31 or not np.issubdtype(fr.dtype, np.integer):
        raise ValueError(f"{what}: `frames` must be a non-empty 1-D integer array of the rows the frames read")
    row = fr.astype(np.int64)
    bad = (row < 0) | (row >= n_rows)
    if bad.any() or np.unique(row).shape[0] != row.shape[0]:
        i = _first(bad) if bad.any() else _first(np.bincount(row)[row] > 1)
        raise ValueError(f"{what}: frame {i} reads row {int(row[i])} of a table of {n_rows} rows (a row takes one frame)")
    return np.ascontiguousarray(row.astype(np.int32))


def fec_soft(sym, frames, soft, period=2, pattern=3):
    """Launch 1 of the frame decoder (sy11_fec_soft): every frame of ``frames`` — ``sy11.data.decode.FECFRAME`` records (sym_off, T, order, q, tail, row, scale):
    the payload symbols from ``sym[sym_off]`` on, turned back by ``q`` steps of 2 pi / order — writes its ``2T`` depunctured soft bits
    ``clamp(rintf(x * scale), -127, 127)`` to ``soft[row]`` (rows, stride) int8, 0 where the puncture pattern (bit i of ``pattern`` = mother position i, applied with the
    even ``period`` <= 64; 1 = sent) removed the bit.  A refused call raises ``Sy11Error`` and writes nothing.  -> ``soft``."""
    what = "fec_soft"
    _need_gpu(sym, soft)
    _packed_c64(what, "sym", sym)
    T_MAX = _lib.load().sy11_fec_tmax()
    _fec_table(what, "soft", soft, torch.int8, sym.device, lo=2, hi=2 * T_MAX, even=True)
    fr = _fec_frames(what, frames, soft.shape[0])
    if isinstance(period, bool) or not isinstance(period, (int, np.integer)) or not 2 <= period <= 64 or period % 2 or isinstance(pattern, bool) \
            or not isinstance(pattern, (int, np.integer)) or not 0 < pattern < 2 ** int(period):
        raise _lib.Sy11Error(f"{what}: the pattern {pattern!r} of period {period!r} is not a non-zero word of an even 2 .. 64 positions")
    period, pattern = int(period), int(pattern)
    _fec_fit(what, fr, soft.shape[1])
    pat = np.array([(pattern >> i) & 1 for i in range(period)], dtype=np.int64)
    twoT = 2 * fr["T"].astype(np.int64)
    n_coded = twoT // period * int(pat.sum()) + np.concatenate(([0], np.cumsum(pat)))[twoT % period]
    w = fr["order"].astype(np.int64) // 2
    need = -(-n_coded // w)
    bad = (fr["sym_off"] < 0) | (fr["sym_off"] > sym.shape[0] - need)
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: frame {k}: the {int(need[k])} payload symbols at {int(fr['sym_off'][k])} leave the {sym.shape[0]} packed symbols")
    bad = ~(np.isfinite(fr["scale"]) & (fr["scale"] > 0))
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: frame {k}: the scale {float(fr['scale'][k])!r} is not finite and above 0")
    t = torch.from_numpy(fr.view(np.uint8)).to(sym.device)
    call("sy11_fec_soft", fr.shape[0], C.c_void_p(fr.ctypes.data), C.c_void_p(t.data_ptr()), period, pattern, sym.shape[0],
         C.c_void_p(torch.view_as_real(sym).data_ptr()), soft.shape[0], soft.shape[1], _p(soft), _stream())
    t.record_stream(torch.cuda.current_stream(sym.device))
    return soft


def fec_viterbi(soft, frames, polys, bits, out):
    """Launch 2 of the frame decoder (sy11_fec_viterbi): the Viterbi decoder of the rate 1/2, K = 7 code with the generators ``polys`` over the ``2T`` soft bits
    ``soft[row]`` of every frame of ``frames`` (int32 path metrics from state 0; traceback from state 0 with ``tail``, else from the best state, the lowest on
    a tie) — writes the ``T`` decided bits packed MSB first, zero-padded, to ``bits[row]`` (rows, stride) uint8 and (final metric, end state) to ``out[row]``
    (rows, 2) int32.  One wavefront per frame.  A refused call raises ``Sy11Error`` and writes nothing.  -> ``(bits, out)``."""
    what = "fec_viterbi"
    _need_gpu(soft, bits, out)
    T_MAX = _lib.load().sy11_fec_tmax()
    _fec_table(what, "soft", soft, torch.int8, soft.device, lo=2, hi=2 * T_MAX, even=True)
    _fec_table(what, "bits", bits, torch.uint8, soft.device, n_rows=soft.shape[0], lo=1, hi=T_MAX // 8)
    _fec_table(what, "out", out, torch.int32, soft.device, n_rows=soft.shape[0], width=2)
    g0, g1 = _fec_polys(what, polys)
    fr = _fec_frames(what, frames, soft.shape[0])
    _fec_fit(what, fr, soft.shape[1], bits.shape[1])
    t = torch.from_numpy(fr.view(np.uint8)).to(soft.device)
    call("sy11_fec_viterbi", fr.shape[0], C.c_void_p(fr.ctypes.data), C.c_void_p(t.data_ptr()), g0, g1, soft.shape[0], soft.shape[1], _p(soft), bits.shape[1], _p(bits),
         _p(out), _stream())
    t.record_stream(torch.cuda.current_stream(soft.device))
    return bits, out


def fec_check(soft, bits, frames, polys, n_info, data, rows, whiten=None, crc=None):
    """Launch 3 of the frame decoder (sy11_fec_check): for every frame of ``frames`` the decided bits ``bits[row]`` are encoded again and compared with the signs
    of ``soft[row]`` where it is not 0; the first ``n_info`` of them, XORed with ``whiten`` (a uint8 device vector of ``n_info`` 0/1, or None), are written packed MSB first,
    zero-padded, to ``data[row]`` (rows, stride) uint8, and (crc_calc, crc_recv, crc_ok, channel_errors, n_channel) to ``rows[row]`` (rows, 5) int32; ``crc``: None
    (crc_ok = -1) or a dict width / poly / init / refin / refout / xorout (``sy11.data.decode.CRCS``).  A refused call raises ``Sy11Error`` and writes nothing.
    -> ``(data, rows)``."""
    from .data.decode import K
    what = "fec_check"
    _need_gpu(soft, bits, data, rows)
    T_MAX = _lib.load().sy11_fec_tmax()
    dev, n = soft.device, soft.shape[0]
    _fec_table(what, "soft", soft, torch.int8, dev, lo=2, hi=2 * T_MAX)
    _fec_table(what, "bits", bits, torch.uint8, dev, n_rows=n, lo=1, hi=T_MAX // 8)
    _fec_table(what, "data", data, torch.uint8, dev, n_rows=n, lo=1, hi=T_MAX // 8)
    _fec_table(what, "rows", rows, torch.int32, dev, n_rows=n, width=5)
    g0, g1 = _fec_polys(what, polys)
    if not _is_int(n_info) or not 1 <= n_info <= T_MAX or (n_info + 7) // 8 > data.shape[1]:
        raise _lib.Sy11Error(f"{what}: {n_info!r} information bits are not 1 .. {T_MAX} or leave the {data.shape[1]} bytes of a data row")
    n_info = int(n_info)
    if whiten is not None:
        _u8_vector(what, "whiten", whiten, dev, n_info)
    spec = _crc_arg(what, crc, n_info, False, _lib.Sy11Error)
    fr = _fec_frames(what, frames, n)
    bad = fr["T"].astype(np.int64) != n_info + (K - 1) * fr["tail"].astype(np.int64)
    if bad.any():
        k = _first(bad)
        raise _lib.Sy11Error(f"{what}: frame {k}: {int(fr['T'][k])} steps are not the {n_info} information bits" + (" and a tail of 6" if fr["tail"][k] else ""))
    _fec_fit(what, fr, soft.shape[1], bits.shape[1])
    t = torch.from_numpy(fr.view(np.uint8)).to(dev)
    call("sy11_fec_check", fr.shape[0], C.c_void_p(fr.ctypes.data), C.c_void_p(t.data_ptr()), g0, g1, n_info, _p(whiten), C.byref(spec), n, soft.shape[1], _p(soft),
         bits.shape[1], _p(bits), data.shape[1], _p(data), _p(rows), _stream())
    t.record_stream(torch.cuda.current_stream(dev))
    return data, rows


def _dev_table(what, name, t, dtype, dev, n_rows=None, shape=None, least=1):
    """A contiguous device table of ``dtype``: 2-D (rows, stride >= least), or of the trailing ``shape``."""
    bad = not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or t.dim() < 2 or t.shape[0] == 0 or t.shape[0] >= 2 ** 31 or not t.is_contiguous() \
        or (dev is not None and t.device != dev) or (n_rows is not None and t.shape[0] != n_rows)
    if not bad:
        bad = tuple(t.shape[1:]) != tuple(shape) if shape is not None else (t.dim() != 2 or t.shape[1] < least or t.shape[1] >= 2 ** 31)
    if bad or t.data_ptr() % t.element_size():
        raise ValueError(f"{what}: `{name}` must be a non-empty contiguous {dtype} tensor on the device" +
                         (f" of shape (rows,) + {tuple(shape)}" if shape is not None else f", (rows, stride) with a stride of at least {least}") +
                         ("" if n_rows is None else f", of {n_rows} rows"))


def _rs_args(what, code, interleave, frames, n_rows):
    """The checks the two launches of the frame corrector share (the library repeats them) -> (the ``RsCode``, the int32 table of the frames' rows)."""
    from .data.correct import gf_tables
    if not isinstance(code, dict) or set(code) - {"name"} != {"n", "k", "poly", "fcr", "prim"} or not all(_is_int(code[key]) for key in ("n", "k", "poly", "fcr", "prim")):
        raise ValueError(f"{what}: `code` must be a dict of the integers n, k, poly, fcr and prim, got {code!r}")
    n, k, poly, fcr, prim = (int(code[key]) for key in ("n", "k", "poly", "fcr", "prim"))
    if not 1 <= k < n <= 255 or n - k > 64:
        raise ValueError(f"{what}: the code (n={n}, k={k}) is not 1 <= k < n <= 255 with n - k <= 64")
    if not 0 <= fcr <= 254:
        raise ValueError(f"{what}: fcr {fcr} is not in [0, 254]")
    if not 1 <= prim <= 254 or math.gcd(prim, 255) != 1:
        raise ValueError(f"{what}: prim {prim} is not in [1, 254] and coprime to 255")
    if not _is_int(interleave) or not 1 <= interleave <= 8:
        raise ValueError(f"{what}: interleave {interleave!r} is not in [1, 8]")
    gf_tables(poly, what)                                                       # 9 bits, primitive
    return _lib.RsCode(n, k, fcr, prim, int(interleave), poly), _frame_rows(what, frames, n_rows)


def rs_decode(data, frames, code, info, cw, interleave=1, offset=0):
    """Launch 1 of the frame corrector (sy11_rs_decode): for every frame of ``frames`` (the rows they read, a 1-D integer array) the ``interleave`` Reed-Solomon
    codewords of ``code`` (a dict n, k, poly, fcr, prim: ``sy11.data.correct.CODES``) that lie byte by byte from byte ``offset`` of ``data[row]`` (rows, stride)
    uint8 are corrected by up to ``(n - k) // 2`` byte errors each.  ``info[row]`` (rows, stride >= interleave k) uint8 takes the information bytes, codeword after
    codeword, and ``cw[row]`` (rows, interleave, 2) int32 the byte errors (-1: not correctable, the bytes pass through) and bit errors of each.  One wavefront
    per codeword.  A refused call raises ``ValueError`` and writes nothing.  -> ``(info, cw)``."""
    what = "rs_decode"
    _dev_table(what, "data", data, torch.uint8, None)
    dev, n_rows = data.device, data.shape[0]
    spec, row = _rs_args(what, code, interleave, frames, n_rows)
    _dev_table(what, "info", info, torch.uint8, dev, n_rows=n_rows, least=spec.interleave * spec.k)
    _dev_table(what, "cw", cw, torch.int32, dev, n_rows=n_rows, shape=(spec.interleave, 2))
    if not _is_int(offset) or offset < 0 or offset + spec.interleave * spec.n > data.shape[1]:
        raise ValueError(f"{what}: the {spec.interleave} x {spec.n} bytes at offset {offset!r} leave the {data.shape[1]} bytes of a data row")
    t = torch.from_numpy(row).to(dev)
    call("sy11_rs_decode", row.shape[0], C.c_void_p(row.ctypes.data), _p(t), C.byref(spec), int(offset), n_rows, data.shape[1], _p(data), info.shape[1], _p(info), _p(cw),
         _stream())
    t.record_stream(torch.cuda.current_stream(dev))
    return info, cw


def rs_check(info, cw, frames, code, rows, interleave=1, crc=None):
    """Launch 2 of the frame corrector (sy11_rs_check): for every frame of ``frames`` ``rows[row]`` (rows, 6) int32 takes n_failed (the codewords of ``cw[row]`` with -1),
    the sums of byte and bit errors over the others, and crc_calc, crc_recv, crc_ok over the ``interleave k`` bytes of ``info[row]``: ``crc`` None (crc_ok = -1) or a
    dict width / poly / init / refin / refout / xorout of whole bytes (``sy11.data.decode.CRCS``), the check field the last bytes, MSB first.  A refused call raises
    ``ValueError`` and writes nothing.  -> ``rows``."""
    what = "rs_check"
    _dev_table(what, "info", info, torch.uint8, None)
    dev, n_rows = info.device, info.shape[0]
    spec, row = _rs_args(what, code, interleave, frames, n_rows)
    n_bytes = spec.interleave * spec.k
    _dev_table(what, "info", info, torch.uint8, dev, least=n_bytes)
    _dev_table(what, "cw", cw, torch.int32, dev, n_rows=n_rows, shape=(spec.interleave, 2))
    _dev_table(what, "rows", rows, torch.int32, dev, n_rows=n_rows, shape=(6,))
    check = _crc_arg(what, crc, 8 * n_bytes, True, ValueError)
    t = torch.from_numpy(row).to(dev)
    call("sy11_rs_check", row.shape[0], C.c_void_p(row.ctypes.data), _p(t), C.byref(spec), C.byref(check), n_rows, info.shape[1], _p(info), _p(cw), _p(rows), _stream())
    t.record_stream(torch.cuda.current_stream(dev))
    return rows


def _ldpc_call(name, *args):
    """The library's refusal as a ``ValueError``, as this file's own."""
    try:
        call(name, *args)
    except _lib.Sy11Error as e:
        raise ValueError(str(e)) from None


def ldpc_decode(soft, frames, code, bits, out, post=None, iterations=20, scale=12):
    """Launch 2 of the LDPC frame decoder (sy11_ldpc_decode): the layered normalised min-sum decoder of ``code`` (a ``sy11.data.ldpc.LdpcCode`` or a dict Z, base) over
    the N int8 soft bits ``soft[row]`` (rows, stride) of every frame of ``frames`` (the rows they read, a 1-D integer array), at most ``iterations`` sweeps (1 .. 100) with
    the check messages scaled by ``scale`` sixteenths (1 .. 16); a frame stops at the first sweep whose decision satisfies every check.  ``bits[row]`` (rows, stride)
    uint8 takes the N decided bits packed MSB first, zero-padded to the stride, ``out[row]`` (rows, 2) int32 the iterations run and the checks left unsatisfied, and
    ``post[row]`` (rows, stride >= N) int16, if given, the final values Q.  One workgroup per frame, exact integer arithmetic.  A refused call raises ``ValueError`` and
    writes nothing.  -> ``(bits, out, post)``."""
    from .data.ldpc import _code_of
    what = "ldpc_decode"
    n_max = _lib.load().sy11_ldpc_nmax()
    cd = _code_of(what, code)
    _dev_table(what, "soft", soft, torch.int8, None, least=cd.N)
    dev, n_rows = soft.device, soft.shape[0]
    _dev_table(what, "bits", bits, torch.uint8, dev, n_rows=n_rows, least=(cd.N + 7) // 8)
    _dev_table(what, "out", out, torch.int32, dev, n_rows=n_rows, shape=(2,))
    if post is not None:
        _dev_table(what, "post", post, torch.int16, dev, n_rows=n_rows, least=cd.N)
    if soft.shape[1] > n_max or bits.shape[1] > n_max // 8 or (post is not None and post.shape[1] > n_max):
        raise ValueError(f"{what}: a row of `soft` / `post` holds at most {n_max} values and one of `bits` {n_max // 8} bytes")
    if not _is_int(iterations) or not 1 <= iterations <= 100:
        raise ValueError(f"{what}: iterations {iterations!r} is not an integer in [1, 100]")
    if not _is_int(scale) or not 1 <= scale <= 16:
        raise ValueError(f"{what}: scale {scale!r} is not an integer in [1, 16] (sixteenths)")
    row = _frame_rows(what, frames, n_rows)
    # one upload: the frames' rows, the layers' offsets, the entries
    layer, entry = np.ascontiguousarray(cd.layer, dtype=np.int32), np.ascontiguousarray(cd.entry)
    host = np.concatenate((row, layer, entry.view(np.int32)))
    t = torch.from_numpy(host).to(dev)
    o1, o2 = row.shape[0], row.shape[0] + layer.shape[0]
    spec = _lib.LdpcCode(cd.Z, cd.mb, cd.nb, entry.shape[0])
    _ldpc_call("sy11_ldpc_decode", row.shape[0], C.c_void_p(row.ctypes.data), C.c_void_p(t.data_ptr()), C.byref(spec), C.c_void_p(layer.ctypes.data),
               C.c_void_p(t.data_ptr() + 4 * o1), C.c_void_p(entry.ctypes.data), C.c_void_p(t.data_ptr() + 4 * o2), int(iterations), int(scale), n_rows, soft.shape[1], _p(soft),
               bits.shape[1], _p(bits), _p(out), 0 if post is None else post.shape[1], _p(post), _stream())
    t.record_stream(torch.cuda.current_stream(dev))
    return bits, out, post


def ldpc_check(soft, bits, frames, N, K, data, rows, whiten=None, crc=None):
    """Launch 3 of the LDPC frame decoder (sy11_ldpc_check): for every frame of ``frames`` the ``N`` decided bits ``bits[row]`` are compared with the signs of ``soft[row]`` where
    it is not 0; the first ``K`` of them, XORed with ``whiten`` (a uint8 device vector of ``K`` 0/1, or None), are written packed MSB first, zero-padded, to ``data[row]`` (rows,
    stride) uint8, and (crc_calc, crc_recv, crc_ok, channel_errors, n_channel) to ``rows[row]`` (rows, 5) int32; ``crc``: None (crc_ok = -1) or a dict width / poly / init /
    refin / refout / xorout (``sy11.data.decode.CRCS``), the check field the last bits of the K.  A refused call raises ``ValueError`` and writes nothing.
    -> ``(data, rows)``."""
    what = "ldpc_check"
    n_max = _lib.load().sy11_ldpc_nmax()
    if not _is_int(N) or not _is_int(K) or not 2 <= N <= n_max or N % 2 or not 1 <= K < N:
        raise ValueError(f"{what}: N = {N!r} is not an even integer in [2, {n_max}], or K = {K!r} not an integer in [1, N)")
    N, K = int(N), int(K)
    _dev_table(what, "soft", soft, torch.int8, None, least=N)
    dev, n_rows = soft.device, soft.shape[0]
    _dev_table(what, "bits", bits, torch.uint8, dev, n_rows=n_rows, least=(N + 7) // 8)
    _dev_table(what, "data", data, torch.uint8, dev, n_rows=n_rows, least=(K + 7) // 8)
    _dev_table(what, "rows", rows, torch.int32, dev, n_rows=n_rows, shape=(5,))
    if soft.shape[1] > n_max or bits.shape[1] > n_max // 8 or data.shape[1] > n_max // 8:
        raise ValueError(f"{what}: a row of `soft` holds at most {n_max} values and one of `bits` / `data` {n_max // 8} bytes")
    if whiten is not None:
        _u8_vector(what, "whiten", whiten, dev, K, ValueError)
    spec = _crc_arg(what, crc, K, False, ValueError)
    row = _frame_rows(what, frames, n_rows)
    t = torch.from_numpy(row).to(dev)
    _ldpc_call("sy11_ldpc_check", row.shape[0], C.c_void_p(row.ctypes.data), _p(t), N, K, _p(whiten), C.byref(spec), n_rows, soft.shape[1], _p(soft), bits.shape[1], _p(bits),
               data.shape[1], _p(data), _p(rows), _stream())
    t.record_stream(torch.cuda.current_stream(dev))
    return data, rows


SCAN_METRICS = {"iou": 0, "ios": 1}


def scan_merge(window, boxes, score, cls, start, n_frames, metric="ios", thres=0.5, agnostic=False):
    """Seam merge of a scan's per-window survivors: ``window`` (n,) int32 (non-decreasing), ``boxes`` (n, 4) f32 window-local xyxy,
    ``score`` (n,) f32, ``cls`` (n,) int32, ``start`` (W,) int64 first strip frame of every window (non-decreasing; host or device)
    -> bool keep mask (n,): greedy class-aware suppression in strip coordinates (include/sy11.h)."""
    _need_gpu(window, boxes, score, cls)
    if metric not in SCAN_METRICS:
        raise _lib.Sy11Error(f"scan_merge: metric must be one of {sorted(SCAN_METRICS)}, got {metric!r}")
    n = window.shape[0]
    dev = boxes.device
    start = torch.as_tensor(start, dtype=torch.int64)
    W = start.numel()
    if boxes.shape != (n, 4) or score.shape != (n,) or cls.shape != (n,) or W == 0:
        raise _lib.Sy11Error("scan_merge: expected window (n,), boxes (n, 4), score (n,), cls (n,) and a non-empty start")
    if W > 1 and bool((start[1:] < start[:-1]).any()):
        raise _lib.Sy11Error("scan_merge: `start` must be non-decreasing")
    keep = torch.zeros((n,), dtype=torch.uint8, device=dev)
    if n == 0:
        return keep.bool()
    window = window.to(torch.int32).contiguous()
    if bool((window[1:] < window[:-1]).any()) or int(window[0]) < 0 or int(window[-1]) >= W:
        raise _lib.Sy11Error("scan_merge: rows must be grouped by window, in ascending window order, with 0 <= window < len(start)")
    ws = torch.empty((_lib.load().sy11_scan_merge_workspace_bytes(n, W),), dtype=torch.uint8, device=dev)
    call("sy11_scan_merge", n, W, int(n_frames), _p(window), _p(boxes.float().contiguous()), _p(score.float().contiguous()),
         _p(cls.to(torch.int32).contiguous()), _p(start.to(dev).contiguous()), SCAN_METRICS[metric], float(thres), 1 if agnostic else 0,
         _p(ws), _p(keep), _stream())
    return keep.bool()


def scan_link(tf, cls, gap_t, gap_f=None, align=0.5, agnostic=False, return_passes=False):
    """Tracks of a scan's rows: ``tf`` (n, 4) float64 [t0_s, f_lo_hz, t1_s, f_hi_hz] and ``cls`` (n,) integer on the device -> (n,) int64
    labels in the caller's row order, label[i] = the smallest row index of the connected component of row i under the link relation
    of include/sy11.h (``gap_f`` None: the time branch alone).  One stable sort by t0, one call, one un-permute, all on the device.
    ``return_passes``: also the number of hook passes the call ran."""
    _need_gpu(tf, cls)
    n = tf.shape[0]
    if tf.dim() != 2 or tf.shape[1] != 4 or tf.dtype != torch.float64 or cls.shape != (n,) or cls.dtype.is_floating_point \
            or cls.dtype == torch.bool or cls.device != tf.device:
        raise _lib.Sy11Error("scan_link: expected tf (n, 4) float64 and cls (n,) of an integer type on tf's device")
    use_f = gap_f is not None
    gap_t, gap_f, align = float(gap_t), float(gap_f) if use_f else 0.0, float(align)
    if not (math.isfinite(gap_t) and gap_t >= 0 and math.isfinite(gap_f) and gap_f >= 0 and 0 < align <= 1):
        raise _lib.Sy11Error(f"scan_link: gap_t and gap_f must be finite and >= 0 and align in (0, 1], got {gap_t!r} / {gap_f!r} / {align!r}")
    if n >= 2 ** 31:
        raise _lib.Sy11Error(f"scan_link: {n} rows; one call takes fewer than 2^31")
    if n == 0:
        out = torch.zeros((0,), dtype=torch.int64, device=tf.device)
        return (out, 0) if return_passes else out
    if not bool(torch.isfinite(tf).all()):
        raise _lib.Sy11Error("scan_link: every value of tf must be finite")
    if bool(((tf[:, 2] < tf[:, 0]) | (tf[:, 3] < tf[:, 1])).any()):
        raise _lib.Sy11Error("scan_link: a rectangle is inverted (t1 < t0 or f_hi < f_lo)")
    _, order = torch.sort(tf[:, 0], stable=True)               # order[k] = the caller's row at sorted position k
    rect = tf[order].contiguous()
    label = torch.empty((n,), dtype=torch.int32, device=tf.device)
    ws = torch.empty((_lib.load().sy11_scan_link_workspace_bytes(n),), dtype=torch.uint8, device=tf.device)
    passes = C.c_int32(0)
    call("sy11_scan_link", n, _p(rect), _p(cls[order].to(torch.int32).contiguous()), gap_t, gap_f, int(use_f), align, int(bool(agnostic)),
         _p(ws), _p(label), C.byref(passes), _stream())
    root = label.to(torch.int64)                               # the component of sorted position k, named by a sorted position
    first = torch.full((n,), n, dtype=torch.int64, device=tf.device).scatter_reduce(0, root, order, "amin")   # its smallest caller row
    out = torch.empty((n,), dtype=torch.int64, device=tf.device)
    out[order] = first[root]
    return (out, int(passes.value)) if return_passes else out


# ------------------------------------------------------------------------------------------------ image side of preprocess
def _img_dt(t):
    return _lib.U8 if t.dtype == torch.uint8 else _DT[t.dtype]


def image_u8_to_float(x, dtype=torch.float32, out=None):
    """batch["img"].float() / 255 (models/yolo/detect/train.py:59) in one pass; `out` may be a graph's static input."""
    if x.dtype != torch.uint8 or not x.is_contiguous():
        raise _lib.Sy11Error("image_u8_to_float: x must be a contiguous uint8 tensor")
    y = out if out is not None else torch.empty(x.shape, dtype=dtype, device=x.device)
    if tuple(y.shape) != tuple(x.shape) or not y.is_contiguous() or y.device != x.device:
        raise _lib.Sy11Error("image_u8_to_float: `out` must be a contiguous tensor of x's shape on x's device")
    call("sy11_image_u8_to_float", _DT[y.dtype], x.numel(), _p(x), _p(y), _stream())
    return y


def image_resize_bilinear(x, size, dtype=None, out=None):
    """F.interpolate(x, size=size, mode="bilinear", align_corners=False) on (B, C, H, W); a uint8 x is divided by 255
    first (the multi_scale branch of preprocess_batch, models/yolo/detect/train.py:60-73)."""
    if x.dim() != 4 or not x.is_contiguous():
        raise _lib.Sy11Error("image_resize_bilinear: x must be a contiguous (B, C, H, W) tensor")
    B, Cc, IH, IW = x.shape
    OH, OW = int(size[0]), int(size[1])
    dtype = dtype or (torch.float32 if x.dtype == torch.uint8 else x.dtype)
    y = out if out is not None else torch.empty((B, Cc, OH, OW), dtype=dtype, device=x.device)
    if tuple(y.shape) != (B, Cc, OH, OW) or not y.is_contiguous() or y.device != x.device:
        raise _lib.Sy11Error("image_resize_bilinear: `out` must be a contiguous (B, C, OH, OW) tensor on x's device")
    call("sy11_image_resize_bilinear", _img_dt(x), _DT[y.dtype], B * Cc, IH, IW, OH, OW, _p(x), _p(y), _stream())
    return y


def image_letterbox(src, dst, new_hw, top, left, fill=114, reverse_c=False, chw=True):
    """src (h, w, 3) uint8 HWC on the device -> dst: a (3, H, W) / (H, W, 3) uint8 or float tensor (one batch slot).
    LetterBox.__call__ (data/augment.py:1544-1591) + the BGR->RGB / HWC->CHW / /255 of predictor.preprocess."""
    if src.dtype != torch.uint8 or src.dim() != 3 or src.shape[2] != 3 or not src.is_contiguous():
        raise _lib.Sy11Error("image_letterbox: src must be a contiguous (h, w, 3) uint8 tensor")
    if dst.dim() != 3 or not dst.is_contiguous() or dst.device != src.device or dst.shape[0 if chw else 2] != 3:
        raise _lib.Sy11Error("image_letterbox: dst must be a contiguous (3, H, W) [chw] or (H, W, 3) tensor on src's device")
    H, W = (dst.shape[1], dst.shape[2]) if chw else (dst.shape[0], dst.shape[1])
    call("sy11_image_letterbox", _img_dt(dst), src.shape[0], src.shape[1], H, W, int(new_hw[0]), int(new_hw[1]), int(top),
         int(left), int(fill), int(bool(reverse_c)), int(bool(chw)), _p(src), _p(dst), _stream())
    return dst


def _pack_tiles(who, tiles, device):
    """tiles -> (count, host array of device pointers, host array of 8 int32 per tile) as the image_*_warp entries take them."""
    n = len(tiles)
    srcs = (C.c_void_p * max(n, 1))()
    geom = (C.c_int32 * (8 * max(n, 1)))()
    for t, (src, x1, y1, x2, y2, padw, padh) in enumerate(tiles):
        if src.dtype != torch.uint8 or src.dim() != 3 or src.shape[2] != 3 or not src.is_contiguous() or src.device != device:
            raise _lib.Sy11Error(f"{who}: every tile must be a contiguous (h, w, 3) uint8 tensor on dst's device")
        srcs[t] = src.data_ptr()
        geom[8 * t:8 * t + 8] = [src.shape[0], src.shape[1], int(x1), int(y1), int(x2), int(y2), int(padw), int(padh)]
    return n, srcs, geom


def _pack_lut(who, hsv_lut):
    """-> (pointer or None, the array that keeps it alive)."""
    import numpy as np
    if hsv_lut is None:
        return None, None
    lut_np = np.ascontiguousarray(hsv_lut, dtype=np.uint8)
    if lut_np.size != 768:
        raise _lib.Sy11Error(f"{who}: hsv_lut must hold 3 x 256 bytes")
    return lut_np.ctypes.data_as(C.c_void_p), lut_np


def image_mosaic_warp(tiles, canvas_hw, dst, minv=None, hsv_lut=None, flip_ud=False, flip_lr=False, fill=114,
                      reverse_c=False, chw=True):
    """Render one augmented sample (sy11_image_mosaic_warp).  tiles = [(src (h, w, 3) uint8 device tensor, x1, y1, x2,
    y2, padw, padh)] (at most 4); minv = 6 floats of the inverted affine map or None; hsv_lut = (3, 256) uint8 numpy
    array or None; dst = (3, H, W) / (H, W, 3) uint8 or float device tensor."""
    if dst.dim() != 3 or not dst.is_contiguous() or dst.shape[0 if chw else 2] != 3:
        raise _lib.Sy11Error("image_mosaic_warp: dst must be a contiguous (3, H, W) [chw] or (H, W, 3) tensor")
    H, W = (dst.shape[1], dst.shape[2]) if chw else (dst.shape[0], dst.shape[1])
    n, srcs, geom = _pack_tiles("image_mosaic_warp", tiles, dst.device)
    m = (C.c_double * 6)(*[float(v) for v in minv]) if minv is not None else None
    lut, _keep = _pack_lut("image_mosaic_warp", hsv_lut)
    call("sy11_image_mosaic_warp", _img_dt(dst), n, srcs, geom, int(canvas_hw[0]), int(canvas_hw[1]), m, H, W, lut,
         int(bool(flip_ud)), int(bool(flip_lr)), int(fill), int(bool(reverse_c)), int(bool(chw)), _p(dst), _stream())
    return dst


def image_mixup_warp(tiles_a, canvas_hw_a, minv_a, tiles_b, canvas_hw_b, minv_b, r, dst, hsv_lut=None, flip_ud=False,
                     flip_lr=False, fill=114, reverse_c=False, chw=True):
    """Render one MixUp sample (sy11_image_mixup_warp): recipe a (the sample) and recipe b (the partner), each as in
    image_mosaic_warp, blended per pixel as (a * r + b * (1 - r)).astype(uint8) — 1 - r is formed here, in float64 —
    then hsv_lut / flips / layout as in image_mosaic_warp.  Both recipes must produce dst's H x W."""
    if dst.dim() != 3 or not dst.is_contiguous() or dst.shape[0 if chw else 2] != 3:
        raise _lib.Sy11Error("image_mixup_warp: dst must be a contiguous (3, H, W) [chw] or (H, W, 3) tensor")
    H, W = (dst.shape[1], dst.shape[2]) if chw else (dst.shape[0], dst.shape[1])
    na, srcs_a, geom_a = _pack_tiles("image_mixup_warp", tiles_a, dst.device)
    nb, srcs_b, geom_b = _pack_tiles("image_mixup_warp", tiles_b, dst.device)
    ma = (C.c_double * 6)(*[float(v) for v in minv_a]) if minv_a is not None else None
    mb = (C.c_double * 6)(*[float(v) for v in minv_b]) if minv_b is not None else None
    lut, _keep = _pack_lut("image_mixup_warp", hsv_lut)
    r = float(r)
    call("sy11_image_mixup_warp", _img_dt(dst), na, srcs_a, geom_a, int(canvas_hw_a[0]), int(canvas_hw_a[1]), ma,
         nb, srcs_b, geom_b, int(canvas_hw_b[0]), int(canvas_hw_b[1]), mb, r, 1.0 - r, H, W, lut,
         int(bool(flip_ud)), int(bool(flip_lr)), int(fill), int(bool(reverse_c)), int(bool(chw)), _p(dst), _stream())
    return dst


class DetLossWorkspace:
    """Device buffers of one fused-loss evaluation (kept for the backward launch)."""

    def __init__(self, maps, strides, nc, gt):
        self.maps = maps
        self.nl = len(maps)
        self.B = maps[0].shape[0]
        self.nc = nc
        self.G = gt.shape[1]
        self.gt = gt.contiguous().float()
        dev = maps[0].device
        self.A = sum(m.shape[1] * m.shape[2] for m in maps)
        self.ptrs = (C.c_void_p * self.nl)(*[m.data_ptr() for m in maps])
        self.hs = (C.c_int32 * self.nl)(*[m.shape[1] for m in maps])
        self.ws = (C.c_int32 * self.nl)(*[m.shape[2] for m in maps])
        self.st = (C.c_float * self.nl)(*[float(s) for s in strides])
        B, A, G = self.B, self.A, max(self.G, 1)
        self.pbox = torch.empty((B, A, 4), dtype=torch.float32, device=dev)
        self.align = torch.empty((B, G, A), dtype=torch.float32, device=dev)
        self.overlap = torch.empty((B, G, A), dtype=torch.float32, device=dev)
        self.topk = torch.empty((B, G, 10), dtype=torch.int32, device=dev)
        self.assign = torch.empty((B, A), dtype=torch.int32, device=dev)
        self.norm = torch.empty((B, A), dtype=torch.float32, device=dev)
        self.zero = torch.zeros(2 * B * G + 256, dtype=torch.float32, device=dev)      # pos maxima + sums, one memset
        self.pos = self.zero[: 2 * B * G]
        self.sums = self.zero[2 * B * G:].view(64, 4)


def det_loss_assign(maps, strides, nc, gt):
    """Stage 1 of the criterion (decode + task-aligned assignment + normalised alignment and its sum `tss`):
    maps: contiguous NHWC f32 (B,H,W,64+nc) list; gt (B,G,5).  -> workspace holding assign / norm / sums[:, 0]."""
    _need_gpu(*maps, gt)
    for m in maps:
        if m.dtype != torch.float32 or not m.is_contiguous() or m.shape[-1] != 64 + nc:
            raise _lib.Sy11Error("det_loss: maps must be contiguous NHWC f32 with 64+nc channels")
    w = DetLossWorkspace(maps, strides, nc, gt)
    cast = lambda a: C.cast(a, C.c_void_p)
    call("sy11_det_loss_assign", w.B, nc, w.nl, cast(w.ptrs), cast(w.hs), cast(w.ws), cast(w.st), w.G, _p(w.gt), _p(w.pbox),
         _p(w.align), _p(w.overlap), _p(w.topk), _p(w.assign), _p(w.pos), _p(w.norm), _p(w.sums), _stream())
    return w


def det_loss_terms(w: DetLossWorkspace):
    """Stage 2: box / cls / dfl partial sums into sums[:, 1:4] for the assignment (w.assign, w.norm) the workspace holds."""
    cast = lambda a: C.cast(a, C.c_void_p)
    call("sy11_det_loss_terms", w.B, w.nc, w.nl, cast(w.ptrs), cast(w.hs), cast(w.ws), cast(w.st), w.G, _p(w.gt), _p(w.assign),
         _p(w.norm), _p(w.sums), _stream())
    return w


def det_loss_forward(maps, strides, nc, gt):
    """maps: contiguous NHWC f32 (B,H,W,64+nc) list; gt (B,G,5).  -> workspace (sums (64,4) = [tss, box, cls, dfl] partials)."""
    return det_loss_terms(det_loss_assign(maps, strides, nc, gt))


def det_loss_finish(w: DetLossWorkspace, gains):
    """-> device tensor [loss, box, cls, dfl, 1 / max(tss, 1)] (loss.py:268-275), one launch."""
    out = torch.empty(5, dtype=torch.float32, device=w.sums.device)
    call("sy11_det_loss_finish", _p(w.sums), w.B, float(gains[0]), float(gains[1]), float(gains[2]), _p(out), _stream())
    return out


def det_loss_pack_targets(batch_idx, cls, bboxes, B, G, scale_wh):
    """v8DetectionLoss.preprocess: three (n, ...) f32 device columns -> (B, G, 5) [cls, xyxy pixels]; strided views are fine."""
    _need_gpu(batch_idx, cls, bboxes)
    n = batch_idx.shape[0]
    gt = torch.empty((B, G, 5), dtype=torch.float32, device=batch_idx.device)
    if n == 0 or G == 0:
        return gt.zero_() if G else gt
    for t in (batch_idx, cls, bboxes):
        if t.dtype != torch.float32:
            raise _lib.Sy11Error("det_loss_pack_targets: target columns must be f32")
    bi, cl = batch_idx.reshape(n, -1)[:, 0], cls.reshape(n, -1)[:, 0]
    if bboxes.dim() != 2 or bboxes.shape[1] != 4 or bboxes.stride(1) != 1:
        raise _lib.Sy11Error("det_loss_pack_targets: bboxes must be (n, 4) with unit inner stride")
    call("sy11_det_loss_pack_targets", n, B, G, _p(bi), max(bi.stride(0), 1), _p(cl), max(cl.stride(0), 1), _p(bboxes), max(bboxes.stride(0), 4),
         float(scale_wh[0]), float(scale_wh[1]), _p(gt), _stream())
    return gt


def det_loss_backward(w: DetLossWorkspace, upstream: torch.Tensor, gains, out=None, inv_tss=None):
    """d loss / d maps.  ``upstream``: device scalar (upstream gradient; already divided by max(tss, 1) unless ``inv_tss`` — the
    device scalar 1 / max(tss, 1) of det_loss_finish — is given).  ``out``: optional list of NHWC f32 buffers to write into (the
    captured backward graph's static output-gradient tensors) — used when every shape matches, else fresh tensors are returned."""
    if out is not None and len(out) == w.nl and all(o.shape == m.shape and o.dtype == m.dtype and o.is_contiguous() for o, m in zip(out, w.maps)):
        dmaps = list(out)
    else:
        dmaps = [torch.empty_like(m) for m in w.maps]
    dptrs = (C.c_void_p * w.nl)(*[d.data_ptr() for d in dmaps])
    cast = lambda a: C.cast(a, C.c_void_p)
    call("sy11_det_loss_bwd", w.B, w.nc, w.nl, cast(w.ptrs), cast(dptrs), cast(w.hs), cast(w.ws), cast(w.st), w.G, _p(w.gt),
         _p(w.assign), _p(w.norm), _p(upstream), _p(inv_tss), float(gains[0]), float(gains[1]), float(gains[2]), _stream())
    return dmaps


# ------------------------------------------------------------------------------------------------ Fusion('ESChannel')
def fusion_stats(x, mm, amax, sq_slice):
    """x: NHWC view (B,H,W,C); mm (B,H,W,2) f32; amax (B,H,W) int16/uint16; sq_slice: (B, C) view of the (B, n*C) buffer."""
    _need_gpu(x, mm, amax, sq_slice)
    B, H, W, Cn = x.shape
    call("sy11_fusion_stats", dt_code(x.dtype), B, H * W, Cn, _p(x), view_ld(x), _p(mm), _p(amax), _p(sq_slice), sq_slice.stride(0), _stream())


def sab_map_fwd(mm, w18, S):
    B, H, W, _ = mm.shape
    call("sy11_sab_map_fwd", B, H, W, _p(mm), _p(w18), _p(S), _stream())


def sab_map_bwd(dS, S, mm, w18, dmm, dw18):
    B, H, W, _ = mm.shape
    call("sy11_sab_map_bwd", B, H, W, _p(dS), _p(S), _p(mm), _p(w18), _p(dmm), _p(dw18), _stream())


def gct_gate_fwd(sq, alpha, gamma, beta, eps, G):
    B, Ct = sq.shape
    call("sy11_gct_gate_fwd", B, Ct, _p(sq), _p(alpha), _p(gamma), _p(beta), float(eps), _p(G), _stream())


def gct_gate_bwd(sq, alpha, gamma, beta, eps, dG, q, dalpha, dgamma, dbeta):
    B, Ct = sq.shape
    call("sy11_gct_gate_bwd", B, Ct, _p(sq), _p(alpha), _p(gamma), _p(beta), float(eps), _p(dG), _p(q), _p(dalpha), _p(dgamma),
         _p(dbeta), _stream())


def fusion_combine(xs, Ss, G, out):
    _need_gpu(*xs, out)
    B, H, W, Cn = xs[0].shape
    a = []
    for i in range(3):
        a += [_p(xs[i]), view_ld(xs[i]), _p(Ss[i])] if i < len(xs) else [None, 0, None]
    call("sy11_fusion_combine", dt_code(out.dtype), B, H * W, Cn, len(xs), *a, _p(G), _p(out), view_ld(out), _stream())
    return out


def fusion_bwd_reduce(dout, x, dG_slice, dS):
    B, H, W, Cn = x.shape
    call("sy11_fusion_bwd_reduce", dt_code(x.dtype), B, H * W, Cn, _p(dout), view_ld(dout), _p(x), view_ld(x), _p(dG_slice),
         dG_slice.stride(0), _p(dS), _stream())


def fusion_bwd_apply(dout, x, G_slice, q_slice, S, dmm, amax, dx, accumulate):
    B, H, W, Cn = x.shape
    call("sy11_fusion_bwd_apply", dt_code(x.dtype), B, H * W, Cn, _p(dout), view_ld(dout), _p(x), view_ld(x), _p(G_slice), _p(q_slice),
         G_slice.stride(0), _p(S), _p(dmm), _p(amax), _p(dx), view_ld(dx), int(accumulate), _stream())


# ------------------------------------------------------------------------------------------------ trainer step (flat buffers)
OPT_PARTS = 1024


def opt_workspace(device):
    return torch.zeros(_lib.load().sy11_opt_workspace_floats(OPT_PARTS), dtype=torch.float32, device=device)


def opt_step(param, grad, mom, sq, ema, buf, ema_buf, ws, group_end, lr, momentum, weight_decay, kind, ema_decay, max_norm=10.0,
             beta2=0.999, eps=1e-8, scale=None, growth_tracker=None, adam_step=None, growth=2.0, backoff=0.5, interval=2000,
             norm_out=None):
    """engine/trainer.py:585-593 in two launches (csrc/optim.hip): unscale + ||g||, then clip + SGD-nesterov / AdamW + EMA +
    zero_grad + GradScaler.update.  All tensors are flat f32 device buffers; ``scale`` / ``growth_tracker``: GradScaler's device
    scalars (None = no AMP); ``ema`` / ``ema_buf`` None = no EMA."""
    _need_gpu(param, grad, mom, sq, ema, buf, ema_buf, ws)
    n = param.numel()
    for t in (grad, mom, sq, ema):
        if t is not None and (t.numel() != n or t.dtype != torch.float32 or not t.is_contiguous()):
            raise _lib.Sy11Error("opt_step: grad / mom / sq / ema must be contiguous f32 buffers of the parameter buffer's length")
    d = OptDesc()
    d.n, d.n_buf = n, (buf.numel() if (buf is not None and ema_buf is not None) else 0)
    for k in range(3):
        d.group_end[k], d.lr[k], d.momentum[k], d.weight_decay[k] = int(group_end[k]), float(lr[k]), float(momentum[k]), float(weight_decay[k])
    d.kind, d.beta2, d.eps, d.max_norm, d.ema_decay = int(kind), float(beta2), float(eps), float(max_norm), float(ema_decay)
    d.amp = int(scale is not None)
    d.growth_factor, d.backoff_factor, d.growth_interval, d.nparts = float(growth), float(backoff), int(interval), OPT_PARTS
    call("sy11_opt_grad_norm", n, _p(grad), _p(scale), _p(adam_step), _p(ws), OPT_PARTS, _stream())
    call("sy11_opt_step", C.byref(d), _p(param), _p(grad), _p(mom), _p(sq), _p(ema), _p(buf) if d.n_buf else None,
         _p(ema_buf) if d.n_buf else None, _p(ws), _p(scale), _p(growth_tracker), _p(adam_step), _p(norm_out), _stream())
