"""Float64 references, case lists and a Python mirror of the depthwise dispatch for the convolution variants that the
dense 3x3 / 1x1 tests never reach: depthwise (csrc/direct.hip), grouped (1 < groups < C) and the dense tap table away
from "k in {1, 3}, pad k // 2, dilation 1" (csrc/igemm.hip, csrc/wgrad.hip).

Two operand families.

* exact: small integers (depthwise x, dy in [-3, 3], w in [-2, 2]; every MFMA path x, w, dy in {-1, 0, 1}).  They are
  exact in f16 / bf16 / f32, every product and every partial sum in any order is an exact f32 integer, so a device result
  must be BIT-EQUAL to the float64 reference.  `assert_exact_conditions` states what that rests on and is asserted on the
  reference before anything is compared.
* real: uniform [-1, 1] operands rounded through the dtype, compared element by element against
  ``u_out * |ref| + (K + 4) * 2^-23 * S`` with ``S`` the same operation on the absolute values (see `real_case`).

This module imports neither the package nor a device: tests/test_conv_ref_cpu.py runs all of it on the CPU.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

U23 = 2.0 ** -23
U_OUT = {torch.float32: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
# the project's bar for epilogues with a transcendental (tests/test_kernels_gpu.py `close`): relative to the output scale
TOL_SCALE = {torch.float32: 2e-5, torch.float16: 4e-3, torch.bfloat16: 3e-2}
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
SEED = 1


def pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def out_hw(H, W, k, s, p, d):
    kh, kw = pair(k)
    return (H + 2 * p - d * (kh - 1) - 1) // s + 1, (W + 2 * p - d * (kw - 1) - 1) // s + 1


# ------------------------------------------------------------------------------------------------------------ case lists
# depthwise 3x3 / stride 1 / pad 1 / dilation 1, (B, C, H, W); the branch named is the one f16 / bf16 reach
DW_SHAPES = [
    (2, 8, 7, 7),          # window, cpv = 1, run = W
    (3, 64, 9, 20),        # window, run 10
    (2, 256, 5, 16),       # window, run 8
    (1, 1024, 6, 13),      # window, ragged run 10 + 3 (f32: cpv = 256)
    (2, 24, 7, 5),         # generic vec, cpv = 3, rows_pb = 85, one idle thread
    (2, 40, 6, 11),        # generic vec
    (1, 2056, 3, 4),       # generic vec, two channel blocks
    (2, 5, 6, 6),          # scalar
    (1, 300, 4, 5),        # scalar, two channel blocks
    (1, 8, 1, 1), (2, 16, 1, 5), (2, 16, 5, 1),      # degenerate maps: every off-centre tap masked
]
DW_SHAPES_F32_ONLY = [(2, 4, 6, 6), (2, 12, 7, 5), (2, 6, 6, 6)]
DW_SHAPE_BIG = (4, 1024, 66, 80)   # f16 only: the wgrad window grid hits its 512-workgroup cap (270 336 runs)
DW_SLICE_SHAPE = (3, 64, 9, 20)    # run once inside wider buffers, aligned (window, ld > C) and misaligned (VEC = 1)
# other geometries, (k, s, p, d), all on DW_GEOM_SHAPE
DW_GEOM_SHAPE = (3, 64, 9, 11)
DW_GEOMS = [(3, 2, 1, 1), (3, 1, 0, 1), (3, 1, 2, 2), (3, 2, 2, 2), (3, 1, 1, 3), ((1, 3), 1, 1, 1), ((3, 1), 2, 1, 1),
            (2, 2, 0, 1), (1, 1, 0, 1), (3, 3, 1, 1)]
DW_ADVANCE_CASE = ((3, 8, 6, 6), (3, 2, 1, 1))     # rows_pb = 256 > one image's 9 outputs: the f16 3x3 wgrad pixel advance


def dw_cases(dtype):
    """Every exact depthwise case of a dtype as (B, C, H, W, k, s, p, d)."""
    shapes = list(DW_SHAPES)
    if dtype == torch.float32:
        shapes += DW_SHAPES_F32_ONLY
    if dtype == torch.float16:
        shapes.append(DW_SHAPE_BIG)
    cases = [sh + (3, 1, 1, 1) for sh in shapes]
    cases += [DW_GEOM_SHAPE + g for g in DW_GEOMS]
    cases.append(DW_ADVANCE_CASE[0] + DW_ADVANCE_CASE[1])
    return cases


def all_dw_cases():
    seen = []
    for dt in DTYPES:
        for c in dw_cases(dt):
            if c not in seen:
                seen.append(c)
    return seen


# grouped, (B, C, N, H, W, k, s, p, d, g)
GROUPED_CASES = [
    (2, 64, 128, 18, 18, 7, 2, 6, 2, 8),
    (2, 128, 64, 11, 9, 3, 2, 2, 2, 8),
    (2, 64, 96, 16, 16, 3, 1, 1, 1, 2),      # group sub-problems the halo kernel may take, on slices with x_ld = 64
    (2, 64, 64, 12, 70, 3, 1, 1, 1, 4),      # C/g = N/g = 16: the few-channel kernel on slices
    (2, 32, 32, 9, 7, 3, 1, 1, 1, 8),        # C/g = 4: f32 only (the 16-bit paths need C/g % 8 == 0)
]


def grouped_cases(dtype):
    epc = 4 if dtype == torch.float32 else 8
    return [c for c in GROUPED_CASES if (c[1] // c[-1]) % epc == 0 and (c[2] // c[-1]) % epc == 0]


# dense, away from the 3x3 / 1x1, pad k // 2, dilation 1 diagonal, (B, C, N, H, W, k, s, p, d)
DENSE_CASES = [
    (2, 32, 48, 11, 13, 5, 1, 2, 1),
    (1, 16, 40, 17, 15, 7, 2, 3, 1),
    (1, 32, 64, 13, 10, 3, 1, 3, 3),
    (2, 64, 32, 18, 18, 3, 1, 0, 1),
    (2, 32, 32, 9, 12, (1, 3), 1, 1, 1),
    (2, 32, 32, 9, 12, (3, 1), 2, 1, 1),
    (2, 32, 64, 14, 16, 3, 3, 1, 1),
    (2, 32, 64, 12, 14, 2, 2, 0, 1),
    (2, 64, 64, 15, 17, 3, 2, 2, 2),
]
# shaped like what the special kernels take (halo tiles: width % 16 == 0; patch filter gradient: width 80; few-channel kernel:
# C = N = 32), but dilated: igemm configurations 15..19 and wgrad configurations 12..15 must refuse and fall back
DILATED_SPECIAL_CASES = [
    (2, 64, 64, 16, 32, 3, 1, 2, 2),
    (1, 64, 64, 4, 80, 3, 1, 2, 2),
    (2, 32, 32, 12, 70, 3, 1, 2, 2),
]
FORCED_IGEMM_CFGS = [15, 16, 17, 18, 19]
FORCED_WGRAD_CFGS = [12, 13, 14, 15]

# the real-valued family: one shape per kernel family (the mirror below names it) — the precision of a kernel does not depend
# on which index branch fed it
REAL_DW_CASES = [
    (3, 64, 9, 20, 3, 1, 1, 1),          # window
    (2, 40, 6, 11, 3, 1, 1, 1),          # generic vec (f16: the 3x3 filter-gradient kernel)
    (2, 5, 6, 6, 3, 1, 1, 1),            # scalar
    (3, 64, 9, 11, 3, 2, 2, 2),          # generic vec, strided + dilated (holes in dx)
]
REAL_GROUPED_CASES = [(2, 64, 128, 18, 18, 7, 2, 6, 2, 8), (2, 64, 64, 12, 70, 3, 1, 1, 1, 4)]
REAL_DENSE_CASES = [(2, 32, 48, 11, 13, 5, 1, 2, 1), (2, 64, 64, 15, 17, 3, 2, 2, 2)]


# ------------------------------------------------------------------------------------------------------------ operands
def int_operands(B, C, N, H, W, k, s, p, d, g, seed=SEED, density=None):
    """Integer operands of the exact family as float64 NCHW / OIHW tensors: (x, w, dy).  `density` (None: every value of the range
    equally likely, as before) is the fraction of non-zeros of each operand, drawn after the values so that the default is unchanged:
    long sums (K or 9 N in the thousands) stay inside the exact range without losing the -1 / 0 / 1 alphabet."""
    kh, kw = pair(k)
    OH, OW = out_hw(H, W, k, s, p, d)
    depthwise = g == C and C == N
    ax, aw = (3, 2) if depthwise else (1, 1)
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(-ax, ax + 1, (B, C, H, W), generator=gen).double()
    w = torch.randint(-aw, aw + 1, (N, C // g, kh, kw), generator=gen).double()
    dy = torch.randint(-ax, ax + 1, (B, N, OH, OW), generator=gen).double()
    if density is not None:
        def sparse(t, a):
            sign = torch.randint(0, 2, t.shape, generator=gen).double() * 2 - 1
            mag = torch.randint(1, a + 1, t.shape, generator=gen).double()
            return sign * mag * (torch.rand(t.shape, generator=gen) < density)
        x, w, dy = sparse(x, ax), sparse(w, aw), sparse(dy, ax)
    return x, w, dy


def real_operands(B, C, N, H, W, k, s, p, d, g, dtype, seed=SEED):
    """Uniform [-1, 1] operands rounded through dtype, as float64: (x, w, dy, bias); bias stays f32."""
    kh, kw = pair(k)
    OH, OW = out_hw(H, W, k, s, p, d)
    gen = torch.Generator().manual_seed(seed)

    def u(*shape):
        return torch.rand(*shape, generator=gen) * 2 - 1
    x, w, dy, bias = u(B, C, H, W), u(N, C // g, kh, kw), u(B, N, OH, OW), u(N)
    return tuple(t.to(dtype).double() for t in (x, w, dy)) + (bias.double(),)


# ------------------------------------------------------------------------------------------------------------ references
def conv_ref(x, w, dy, s, p, d, g):
    """float64 F.conv2d, autograd for the two gradients: (y, dx, dw)."""
    assert x.dtype == torch.float64 and w.dtype == torch.float64 and dy.dtype == torch.float64
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv2d(xr, wr, None, s, p, d, g)
    dx, dw = torch.autograd.grad(y, (xr, wr), dy)
    return y.detach(), dx, dw


def conv_loops(x, w, dy, s, p, d, g):
    """The same three results by a plain loop nest over Python floats (what conv_ref is checked against on tiny cases)."""
    B, C, H, W = x.shape
    N, cg, kh, kw = w.shape
    ng = N // g
    OH, OW = (H + 2 * p - d * (kh - 1) - 1) // s + 1, (W + 2 * p - d * (kw - 1) - 1) // s + 1
    xl, wl, dyl = x.tolist(), w.tolist(), dy.tolist()
    y = [[[[0.0] * OW for _ in range(OH)] for _ in range(N)] for _ in range(B)]
    dx = [[[[0.0] * W for _ in range(H)] for _ in range(C)] for _ in range(B)]
    dw = [[[[0.0] * kw for _ in range(kh)] for _ in range(cg)] for _ in range(N)]
    for b in range(B):
        for n in range(N):
            c0 = (n // ng) * cg
            for oy in range(OH):
                for ox in range(OW):
                    acc = 0.0
                    for ci in range(cg):
                        for r in range(kh):
                            iy = oy * s - p + r * d
                            if iy < 0 or iy >= H:
                                continue
                            for q in range(kw):
                                ix = ox * s - p + q * d
                                if ix < 0 or ix >= W:
                                    continue
                                acc += xl[b][c0 + ci][iy][ix] * wl[n][ci][r][q]
                                dx[b][c0 + ci][iy][ix] += dyl[b][n][oy][ox] * wl[n][ci][r][q]
                                dw[n][ci][r][q] += dyl[b][n][oy][ox] * xl[b][c0 + ci][iy][ix]
                    y[b][n][oy][ox] = acc
    return (torch.tensor(y, dtype=torch.float64).reshape(B, N, OH, OW), torch.tensor(dx, dtype=torch.float64).reshape(B, C, H, W),
            torch.tensor(dw, dtype=torch.float64).reshape(N, cg, kh, kw))


def assert_exact_conditions(x, dy, y, dx, dw):
    """What bit-equality with the float64 reference rests on.  A failure here means a case list or an operand range was edited
    into territory where a 16-bit store or an f32 sum rounds: fix the case, never the comparison."""
    for t in (x, dy, y, dx, dw):
        assert torch.equal(t, t.round()), "operands and reference must be integers"
    assert y.abs().max().item() <= 256, f"|y| = {y.abs().max().item()} is past the bf16-exact integers"
    assert dx.abs().max().item() <= 256 and 2 * dx.abs().max().item() <= 256, f"2|dx| = {2 * dx.abs().max().item()} is past the bf16-exact integers"
    ssq = (y * y).sum((0, 2, 3)).max().item()
    assert ssq < 2 ** 24, f"per-channel sum of y^2 = {ssq} is not an exact f32 integer"
    assert 2 * dw.abs().max().item() < 2 ** 24, f"|2 dw| = {2 * dw.abs().max().item()} is not an exact f32 integer"
    # every PARTIAL sum of a filter gradient, in any order, after a second call: bounded by the number of terms times the largest
    M = dy.shape[0] * dy.shape[2] * dy.shape[3]
    assert 2 * M * x.abs().max().item() * dy.abs().max().item() < 2 ** 24, "a partial sum of dw could leave the exact f32 integers"


@functools.lru_cache(maxsize=3)
def exact_case(B, C, N, H, W, k, s, p, d, g, seed=SEED, density=None):
    """Operands and float64 results of an exact case, computed once and shared (callers must not write into them):
    dict with x, w, dy, y, dx, dw (NCHW / OIHW) after `assert_exact_conditions`."""
    x, w, dy = int_operands(B, C, N, H, W, k, s, p, d, g, seed, density)
    y, dx, dw = conv_ref(x, w, dy, s, p, d, g)
    assert_exact_conditions(x, dy, y, dx, dw)
    return {"x": x, "w": w, "dy": dy, "y": y, "dx": dx, "dw": dw}


def dgrad_has_holes(k, s, p, d):
    """True when some input parity class receives no tap (the dense / grouped input gradient then needs accumulate into zeros)."""
    return any(all((ph + p - r * d) % s for r in range(kk)) for kk in pair(k) for ph in range(s))


def real_case(B, C, N, H, W, k, s, p, d, g, dtype, seed=SEED):
    """Real-valued operands, float64 results and the elementwise bounds of the real family."""
    x, w, dy, bias = real_operands(B, C, N, H, W, k, s, p, d, g, dtype, seed)
    y, dx, dw = conv_ref(x, w, dy, s, p, d, g)
    S_y, S_dx, S_dw = conv_ref(x.abs(), w.abs(), dy.abs(), s, p, d, g)
    kh, kw = pair(k)
    cg, ng = C // g, N // g
    M = dy.shape[0] * dy.shape[2] * dy.shape[3]
    K = kh * kw * cg
    # taps that really contribute to an input pixel (stride / dilation / border leave some out), times the filters of its group
    taps = F.conv_transpose2d(torch.ones(1, 1, *dy.shape[2:], dtype=torch.float64), torch.ones(1, 1, kh, kw, dtype=torch.float64),
                              None, s, p, 0, 1, d)
    taps = F.pad(taps, (0, W - taps.shape[3], 0, H - taps.shape[2]))      # pixels past the last window: no tap
    u = U_OUT[dtype]
    return {
        "x": x, "w": w, "dy": dy, "bias": bias, "y": y, "dx": dx, "dw": dw, "K": K, "M": M,
        "bound_y": u * y.abs() + (K + 4) * U23 * S_y,
        "bound_y_bias": u * (y + bias.view(1, -1, 1, 1)).abs() + (K + 4) * U23 * (S_y + bias.abs().view(1, -1, 1, 1)),
        "bound_dx": u * dx.abs() + (taps * ng + 4) * U23 * S_dx,
        "bound_dw": (M + 4) * U23 * S_dw,
        "bound_sum": (K + M + 4) * U23 * S_y.sum((0, 2, 3)),
        "bound_sumsq": (2 * K + M + 8) * U23 * (S_y * S_y).sum((0, 2, 3)),
    }


def worst_ratio(got, ref, bound):
    """max over elements of |got - ref| / bound (0 / 0 counts as 0, x / 0 as inf)."""
    err = (got.double() - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return r.max().item()


# ------------------------------------------------------------------------------------------------------------ BatchNorm tail
def bn_tail_ref(s1, s2, count, gamma, beta, eps, momentum, rm0=None, rv0=None):
    """csrc/bn_tail.h in float64 from exact per-channel sums.  Returns {name: (value, allowed absolute error)}: mean must be
    float32(mu) exactly; rstd within one f32 ulp; scale / shift / running statistics (each at most three f32 operations) within
    four f32 ulps of the largest term of their expression."""
    s1, s2, gamma, beta = (np.asarray(t, dtype=np.float64) for t in (s1, s2, gamma, beta))
    eps, mom = float(np.float32(eps)), float(np.float32(momentum))
    mu = s1 / count
    var = np.maximum(s2 / count - mu * mu, 0.0)
    r = 1.0 / np.sqrt(var + eps)

    def ulps(n, *terms):
        big = np.max(np.abs(np.stack(terms)), axis=0).astype(np.float32)
        return n * np.spacing(big).astype(np.float64)
    scale = gamma * r
    out = {"mean": (mu.astype(np.float32).astype(np.float64), np.zeros_like(mu)), "rstd": (r, ulps(1, r)),
           "scale": (scale, ulps(4, scale)), "shift": (beta - mu * scale, ulps(4, beta, mu * scale))}
    if rm0 is not None:
        rm0, rv0 = np.asarray(rm0, dtype=np.float64), np.asarray(rv0, dtype=np.float64)
        unbiased = var * count / (count - 1) if count > 1 else var
        om = float(np.float32(1.0) - np.float32(momentum))
        out["running_mean"] = (om * rm0 + mom * mu, ulps(4, om * rm0, mom * mu))
        out["running_var"] = (om * rv0 + mom * unbiased, ulps(4, om * rv0, mom * unbiased))
    return out


# ------------------------------------------------------------------------------------------------------------ dispatch mirror
def dw_branches(dtype, C, H, W, k, s, p, d, ld=None, aligned=True):
    """Which depthwise kernel each of forward / dgrad / wgrad reaches: a Python copy of `dw_setup` and `dw3x3_ok` in
    csrc/direct.hip, with SY11_DW_WINDOW_WGRAD at its default.  It is a COPY: it can drift from the C++, and then only the labels
    (and the coverage assertion of the CPU test) go stale — the device comparisons never depend on it.

    Returns {"fwd", "dgrad", "wgrad"} -> one of "window0" / "window1" / "window2" / "vec" / "scalar" / "f16_3x3", plus "cpv",
    "rows_pb" and "channel_blocks"."""
    kh, kw = pair(k)
    OH, OW = out_hw(H, W, k, s, p, d)
    ve = 16 // torch.empty((), dtype=dtype).element_size()
    ld = C if ld is None else ld
    vec = C % ve == 0 and ld % ve == 0 and aligned
    cpv = C // (ve if vec else 1)
    window = (vec and (kh, kw, s, p, d) == (3, 3, 1, 1, 1) and (H, W) == (OH, OW) and C <= 1536 and 256 % (C // ve) == 0)
    plain = "vec" if vec else "scalar"
    wgrad = "window2" if window else ("f16_3x3" if vec and dtype == torch.float16 and (kh, kw) == (3, 3) else plain)
    return {"fwd": "window0" if window else plain, "dgrad": "window1" if window else plain, "wgrad": wgrad,
            "cpv": cpv, "rows_pb": 256 // min(cpv, 256), "channel_blocks": math.ceil(cpv / 256)}


def dw_label(dtype, case, **kw):
    B, C, H, W, k, s, p, d = case
    b = dw_branches(dtype, C, H, W, k, s, p, d, **kw)
    return f"{b['fwd']}/{b['dgrad']}/{b['wgrad']} cpv={b['cpv']} rows_pb={b['rows_pb']} blocks_y={b['channel_blocks']}"


def case_id(case):
    return "-".join("x".join(map(str, v)) if isinstance(v, tuple) else str(v) for v in case)
