"""GPU: the four BatchNorm kernels of csrc/elementwise.hip (sy11_bn_finalize, sy11_bn_act_fwd, sy11_bn_act_bwd_reduce,
sy11_bn_act_bwd_apply[_res]) one by one against the float64 reference of tests/_bn_ref.py, with the bar of tests/_kernel_ref.py
(8 * e_ref + u * scale, every element), in f32 / f16 / bf16, with and without SiLU and residual, on contiguous tensors and on
channel slices of wider buffers, and (reduce, apply) in the ordered and in the atomic reduction mode.

Every kernel is called on its own.  The per-channel vectors a kernel reads (mean, rstd, scale, shift, gamma, slot rows) are made
on the CPU, rounded to f32 and uploaded, and the reference starts from exactly those values: no kernel's error reaches another's bar.

Inputs (`_case`): y has a per-channel offset in [-2, 2] and spread in [0.2, 2], dz a per-channel offset in [-0.5, 0.5] plus noise, so
mean(g) and mean(g * xhat) are O(1) and the k1 / k2 terms of the backward apply are far above the bar.  gamma has a negative value and
an exact zero; channel 1 of y is constant (variance 0, xhat = 0); channel 2 has gamma = 25, which drives u = y * scale + shift
past +-30, where SiLU saturates both ways.

Shapes (`SHAPES`): chosen from row_geom / row_walk of elementwise.hip; `test_every_case_reaches_the_branch_it_is_named_for` holds a
pure-Python mirror of the two functions and fails when a retune moves a case off its branch.  f32 runs a reduced set: cases F and G
exist for the f16 / bf16 geometry (273 reduce workgroups, one row per workgroup and the forward's rebalanced grid) and run in the
16-bit types only; G additionally runs half of the SiLU x layout combinations (its float64 reference is 8.6 M elements per tensor).

Measured ratios (MI355X) are in DESIGN.md section 5, "Kernel-level parity, measured".  No quantity needed an allowance for the fast
intrinsics of SiLU (worst f32 forward: 0.12 of the bar).
"""
import contextlib
import functools
import math

import pytest
import torch

from tests import _bn_ref as R
from tests._kernel_ref import DEV, Bars, lib, nhwc_view, ops, outside_untouched, reduction_mode, rnd, rounded, sum_bound  # noqa: F401

gpu = pytest.mark.gpu
F32, F16, BF16, F64 = torch.float32, torch.float16, torch.bfloat16, torch.float64
EPS, MOM = 1e-3, 0.03
C_NEG, C_CONST, C_SAT, C_ZERO = 0, 1, 2, 3          # channels with gamma < 0, constant y, saturating SiLU, gamma == 0
CONST = 1.625                                        # exact in every storage dtype
SUM_SLOTS = (1, 3, 8, 13)
STAT_SLOTS = (1, 8, 13, 32)

#        C     B   H   W
SHAPES = {
    "A": (64, 1, 30, 32),       # M = 960.   f16/bf16: 8 reduce workgroups; with sum_slots = 8 the slot count equals the grid
    "B": (136, 3, 37, 41),      # M = 4551.  16-bit: 17 vectors per row, rows_pb = 15: the tree over a non-power-of-two, one idle thread
    "C": (24, 5, 61, 67),       # M = 20435. 16-bit: rows_pb = 85
    "D": (2056, 2, 9, 11),      # M = 198.   f16: two channel blocks, the second with one vector; f32: three channel blocks
    "E": (20, 2, 23, 19),       # M = 874.   16-bit: C % 8 != 0, the scalar path on many workgroups; f32: vector path, 5 vectors per row
    "F": (512, 1, 66, 66),      # M = 4356.  f16: 273 reduce workgroups (> 256): staged ordered fold / fold into slot rows; four-trip apply
    "G": (1032, 2, 64, 65),     # M = 8320.  f16: rows_pb = 1; the forward's 2080 blocks are rebalanced to 1040
    "H1": (8, 1, 1, 1),         # M = 1:     fewer rows than one workgroup walks; count = 1
    "H3": (8, 1, 1, 3),         # M = 3
}
SIXTEEN_BIT_ONLY = ("F", "G")
ROW_MAP0 = {("B", F16), ("B", F32), ("F", F16)}      # the strided (grid-sized stride) walk: cases B and F only


def _configs():
    out = []
    for dtype in (F32, F16, BF16):
        for cid in SHAPES:
            if dtype == F32 and cid in SIXTEEN_BIT_ONLY:
                continue
            for row_map in (1, 0):
                if row_map == 0 and (cid, dtype) not in ROW_MAP0:
                    continue
                for silu in (True, False):
                    for strided in (False, True):
                        if cid == "G" and silu != strided:
                            continue
                        out.append(pytest.param(cid, dtype, row_map, silu, strided,
                                                id=f"{cid}-{str(dtype)[6:]}-{'chunk' if row_map else 'grid'}-{'silu' if silu else 'linear'}-{'slice' if strided else 'contig'}"))
    return out


CONFIGS = _configs()
per_config = pytest.mark.parametrize("cid,dtype,row_map,silu,strided", CONFIGS)


# ------------------------------------------------------------------------------------------------ geometry mirror
def _cdiv(a, b):
    return -(-a // b)


def _esz(dtype):
    return torch.empty((), dtype=dtype).element_size()


def _row_geom(C, dtype):
    """row_geom + vec_ok of elementwise.hip for the views this module makes (nhwc_view: base and pixel stride are multiples of 16
    bytes exactly when C is): -> vector path?, channel vectors per row, rows per workgroup, channel blocks."""
    vec = 16 // _esz(dtype)
    vector = C % vec == 0
    cpv = C // (vec if vector else 1)
    cw = min(cpv, 256)
    return dict(vector=vector, cpv=cpv, rows_pb=256 // cw, cblocks=_cdiv(cpv, 256), idle=256 - (256 // cw) * cw)


def _row_walk(M, rows_pb, trips, max_blocks, row_map, U=4):
    """row_walk of elementwise.hip: -> grid, rows one thread adds up (`per_thread`), whether the 2048 < blocks < 6144 rule fired."""
    if row_map == 0:
        g = max(1, min(_cdiv(M, rows_pb * U), min(max_blocks, 2048)))
        return dict(grid=g, per_thread=U * _cdiv(M, g * rows_pb * U), rebalanced=False, blocks=g, trips=_cdiv(M, g * rows_pb * U))
    unit = rows_pb * U
    units = _cdiv(M, unit)
    t = max(trips, 1)
    blocks = _cdiv(units, t)
    rebalanced = False
    if blocks > max_blocks:
        t = _cdiv(units, max_blocks)
    elif 2048 < blocks < 6144:
        t, rebalanced = _cdiv(units, 2048), True
    return dict(grid=_cdiv(M, unit * t), per_thread=U * t, rebalanced=rebalanced, blocks=blocks, trips=t)


def _geometry(kernel, M, C, dtype, row_map=1):
    g = _row_geom(C, dtype)
    if kernel == "fwd":
        w = _row_walk(M, g["rows_pb"], 1, 1 << 20, row_map)
    elif kernel == "reduce":
        w = _row_walk(M, g["rows_pb"], 2 if _cdiv(M, g["rows_pb"] * 4) > 640 else 1, 4096, row_map)
    else:
        w = _row_walk(M, g["rows_pb"], 4 if (C >= 512 and M <= 65536) else 2, 1 << 20, row_map)
        w["four_trip"] = C >= 512 and M <= 65536
    return {**g, **w}


def _arrivals(grid, slots, mode):
    """Additions a workgroup's partial passes through on its way into the caller's slot rows (the pre-loaded value counts as the
    first operand).  atomic (or a single workgroup): slot s takes the workgroups s, s + slots, ...: ceil(grid / slots) adds.
    ordered: the `grid` partial rows are folded by fold_stage_kernel / fold_slots_kernel: a lane adds every fourth row of its group
    in sequence, 3 adds join the four lanes, 1 adds onto the output; 64 rows -> 1 per extra stage (16 + 3) while rows > 256, or, with
    more than 256 rows and several slot rows, one launch in which a lane takes every (4 * slots)-th row."""
    if mode == "atomic" or grid == 1:
        return _cdiv(grid, slots)
    if grid > 256 and slots > 1:
        return _cdiv(grid, 4 * slots) + 3 + 1
    k, rows = 0, grid
    while rows > 256:
        k, rows = k + 16 + 3, _cdiv(rows, 64)
    return k + _cdiv(rows, 4) + 3 + 1


def _reduce_depth(geo, slots, mode):
    """Longest chain of f32 additions a term of sum_g / sum_gx passes through: the rows one thread walks, the levels of the tree
    over the rows_pb row groups, the arrivals at the slot row."""
    return geo["per_thread"] + math.ceil(math.log2(geo["rows_pb"])) + _arrivals(geo["grid"], slots, mode)


def test_every_case_reaches_the_branch_it_is_named_for():
    """No GPU needed.  The mirror above, applied to SHAPES: a retune of row_geom / row_walk that empties a case fails here."""
    M = {k: v[1] * v[2] * v[3] for k, v in SHAPES.items()}
    Cn = {k: v[0] for k, v in SHAPES.items()}
    geo = lambda kernel, cid, dtype, row_map=1: _geometry(kernel, M[cid], Cn[cid], dtype, row_map)
    for dt in (F16, BF16):
        a = geo("reduce", "A", dt)
        assert a["vector"] and a["grid"] == 8 and 8 in SUM_SLOTS, a                 # sum_slots == grid in atomic mode
        b = geo("reduce", "B", dt)
        assert b["vector"] and b["rows_pb"] == 15 and b["idle"] == 1 and b["grid"] > 1, b
        assert geo("reduce", "C", dt)["rows_pb"] == 85 and geo("reduce", "C", dt)["grid"] > 1
        d = geo("apply", "D", dt)
        assert d["vector"] and d["cblocks"] == 2 and d["cpv"] - 256 == 1 and d["rows_pb"] == 1, d
        e = geo("reduce", "E", dt)
        assert not e["vector"] and e["grid"] > 8 and geo("fwd", "E", dt)["grid"] > 8 and geo("apply", "E", dt)["grid"] > 4, e
        f = geo("reduce", "F", dt)
        assert f["grid"] == 273 and f["grid"] > 256, f                               # staged fold (1 slot), fold into slot rows (> 1)
        assert _arrivals(273, 1, "ordered") == 19 + 2 + 4 and _arrivals(273, 8, "ordered") == 9 + 4
        assert geo("apply", "F", dt)["four_trip"] and geo("apply", "F", dt)["trips"] == 4
        g = geo("fwd", "G", dt)
        assert g["rows_pb"] == 1 and g["blocks"] == 2080 and g["rebalanced"] and g["grid"] == 1040, g
        assert not geo("fwd", "G", dt, 0)["rebalanced"]
        for h in ("H1", "H3"):
            hh = geo("reduce", h, dt)
            assert hh["grid"] == 1 and M[h] < hh["rows_pb"], hh
    assert geo("apply", "D", F32)["cblocks"] == 3
    e32 = geo("reduce", "E", F32)
    assert e32["vector"] and e32["cpv"] == 5 and e32["idle"] == 1, e32
    assert geo("reduce", "A", F32)["grid"] == 15
    for cid in ("B", "C", "F", "G"):                    # the shapes the sensitivity check counts: more than one workgroup everywhere
        for dt in (F16, BF16) + (() if cid in SIXTEEN_BIT_ONLY else (F32,)):
            assert all(geo(k, cid, dt)["grid"] > 1 for k in ("fwd", "reduce", "apply"))
    for cid, dt in ROW_MAP0:                            # the strided walk makes more than one trip somewhere only on large maps; here: one grid
        assert geo("reduce", cid, dt, 0)["grid"] > 1
    assert any(s % 8 for s in SUM_SLOTS) and any(s > 8 and s % 8 for s in SUM_SLOTS)      # the apply prologue's ragged eight-slot fold
    # the bias-gradient use: f32 dz, C = 2 (scalar path, 2 workgroups) and C = 80 (vector path, 17 workgroups)
    assert not _row_geom(2, F32)["vector"] and _geometry("reduce", 800, 2, F32)["grid"] == 2
    assert _row_geom(80, F32)["vector"] and _geometry("reduce", 800, 80, F32)["grid"] == 17


# ------------------------------------------------------------------------------------------------ inputs
class Case:
    pass


@functools.lru_cache(maxsize=3)
def _case(cid, dtype):
    """The one input builder (module docstring).  Everything is CPU f32 holding values of the storage dtype (y, dz, res, old) or f32
    per-channel vectors; mean / rstd / scale / shift are the float64 batch statistics of the ROUNDED y, rounded to f32."""
    Cn, B, H, W = SHAPES[cid]
    seed = 1000 + 37 * list(SHAPES).index(cid)
    c = Case()
    c.cid, c.C, c.shape, c.M = cid, Cn, (B, H, W, Cn), B * H * W
    off = rnd(Cn, seed=seed, scale=2.0)
    spread = 0.2 + 0.9 * (rnd(Cn, seed=seed + 1) + 1)
    spread[C_SAT] = 2.0
    y = off + spread * rnd(B, H, W, Cn, seed=seed + 2)
    y[..., C_CONST] = CONST
    c.y = rounded(y, dtype)
    c.dz = rounded(rnd(Cn, seed=seed + 3, scale=0.5) + rnd(B, H, W, Cn, seed=seed + 4), dtype)
    c.res = rounded(rnd(B, H, W, Cn, seed=seed + 5, scale=1.5), dtype)
    c.old = rounded(rnd(B, H, W, Cn, seed=seed + 6), dtype)
    c.gamma = 1 + rnd(Cn, seed=seed + 7, scale=0.5)
    c.gamma[C_NEG], c.gamma[C_ZERO], c.gamma[C_SAT] = -0.7, 0.0, 25.0
    c.beta = rnd(Cn, seed=seed + 8, scale=0.3)
    y2 = c.y.double().reshape(-1, Cn)
    c.sum64, c.sq64 = y2.sum(0), (y2 * y2).sum(0)
    c.mean, c.rstd, c.scale, c.shift, _, _ = R.finalize(c.M, c.sum64, c.sq64, c.gamma, c.beta, EPS, MOM, None, None, F32)
    assert c.mean[C_CONST].item() == CONST and abs(c.rstd[C_CONST].item() - R.f32_value(EPS) ** -0.5) < 1e-5
    u = c.y[..., C_SAT].double() * c.scale[C_SAT].double() + c.shift[C_SAT].double()
    c.saturates = bool(u.max() > 30 and u.min() < -30)
    assert c.saturates or c.M < 100, (cid, u.min().item(), u.max().item())
    c.dev = {k: getattr(c, k).to(DEV) for k in ("mean", "rstd", "scale", "shift", "gamma", "beta")}
    return c


@functools.lru_cache(maxsize=4)
def _sums(cid, dtype, silu):
    """sum_g / sum_gx of a case: float64, float32, and the largest per-channel sum of |terms| (for sum_bound)."""
    c = _case(cid, dtype)
    g, gx = R.bwd_terms(c.y, c.dz, c.mean, c.rstd, c.scale, c.shift, silu, F64)
    s64 = torch.stack((g.reshape(-1, c.C).sum(0), gx.reshape(-1, c.C).sum(0)))
    absmax = (g.abs().reshape(-1, c.C).sum(0).max().item(), gx.abs().reshape(-1, c.C).sum(0).max().item())
    s32 = torch.stack(R.bwd_sums(c.y, c.dz, c.mean, c.rstd, c.scale, c.shift, silu, F32))
    return s64, s32, absmax


def _split(total64, slots, seed):
    """[.., C] float64 totals -> [.., slots, C] f32 rows that add up to about the totals, every row O(total) and different."""
    w = 1 + rnd(slots, seed=seed, scale=0.6).double()
    w = w / w.sum()
    return (total64.unsqueeze(-2) * w[:, None]).float()


@contextlib.contextmanager
def _row_map(value):
    _lib = lib()
    prev = _lib.get_option("row_map")
    try:
        _lib.set_option("row_map", value)
        yield
    finally:
        _lib.set_option("row_map", prev)


def _out_view(shape, dtype, strided):
    return nhwc_view(torch.full(shape, -7.0), dtype, strided)


# ------------------------------------------------------------------------------------------------ sy11_bn_finalize
@gpu
@pytest.mark.parametrize("slots", STAT_SLOTS)
@pytest.mark.parametrize("cid", ["B", "D", "E", "F", "H1", "H3"])
def test_bn_finalize(cid, slots):
    """mean, rstd, scale, shift and the running statistics from `slots` rows of sums, with and without running statistics.
    B / F: the unbiased factor count / (count - 1) at a count where it moves running_var by 2e-4 of the variance (the bar is ~1e-6
    of it).  H1: count = 1 (factor 1, not 1 / 0).  Channel 1 is constant, and its sum-of-squares rows are shrunk by 2^-20, so
    E[x^2] - mean^2 is below zero before the clamp."""
    c = _case(cid, F32)
    seed = 7 * slots + c.C
    ssum, ssq = _split(c.sum64, slots, seed), _split(c.sq64, slots, seed + 1)
    ssq[:, C_CONST] *= 1 - 2.0 ** -20
    var_before_clamp = ssq[:, C_CONST].double().sum() / c.M - (ssum[:, C_CONST].double().sum() / c.M) ** 2
    assert var_before_clamp < 0, var_before_clamp
    rm, rv = rnd(c.C, seed=seed + 2, scale=0.1), 1 + rnd(c.C, seed=seed + 3, scale=0.2).abs()
    names = ("mean", "rstd", "scale", "shift", "running_mean", "running_var")
    b = Bars(f"bn_finalize[{cid} C{c.C} count {c.M} slots {slots}]")
    for running in (True, False):
        out = [torch.full((c.C,), float("nan"), device=DEV) for _ in range(4)]
        rmd, rvd = (rm.to(DEV, copy=True), rv.to(DEV, copy=True)) if running else (None, None)
        rows = (ssum.to(DEV), ssq.to(DEV)) if slots > 1 else (ssum[0].to(DEV), ssq[0].to(DEV))
        ops().bn_finalize(c.M, rows[0], rows[1], c.dev["gamma"], c.dev["beta"], EPS, MOM, rmd, rvd, *out)
        torch.cuda.synchronize()
        r64 = R.finalize(c.M, ssum, ssq, c.gamma, c.beta, EPS, MOM, rm if running else None, rv if running else None, F64)
        r32 = R.finalize(c.M, ssum, ssq, c.gamma, c.beta, EPS, MOM, rm if running else None, rv if running else None, F32)
        got = out + ([rmd, rvd] if running else [])
        for name, gv, a, a32 in zip(names, got, r64, r32):
            b.add(name + ("" if running else "(no running)"), gv, a, a32)
        assert abs(out[1][C_CONST].item() - R.f32_value(EPS) ** -0.5) <= 4e-6, "the negative variance was not clamped to 0"
    b.check()


# ------------------------------------------------------------------------------------------------ sy11_bn_act_fwd
@gpu
@per_config
def test_bn_act_fwd(cid, dtype, row_map, silu, strided):
    """z = act(y * scale + shift) (+ res), residual off and on."""
    c = _case(cid, dtype)
    geo = _geometry("fwd", c.M, c.C, dtype, row_map)
    b = Bars(f"bn_act_fwd[{cid} {str(dtype)[6:]} {'silu' if silu else 'linear'} {'slice' if strided else 'contig'} map{row_map} grid {geo['grid']}x{geo['cblocks']}]")
    yv, _ = nhwc_view(c.y, dtype, strided)
    rv, _ = nhwc_view(c.res, dtype, strided)
    with _row_map(row_map):
        for res in (None, c.res):
            zv, zbuf = _out_view(c.shape, dtype, strided)
            ops().bn_act_fwd(yv, c.dev["scale"], c.dev["shift"], zv, silu=silu, res=None if res is None else rv)
            torch.cuda.synchronize()
            assert outside_untouched(zbuf, c.C), "z written outside its channel slice"
            z = zv.float().cpu()
            assert bool(torch.isfinite(z[..., C_SAT]).all()), "the saturating channel is not finite"
            b.add("z" + ("" if res is None else "+res"), z, R.act_fwd(c.y, c.scale, c.shift, silu, res, F64),
                  R.act_fwd(c.y, c.scale, c.shift, silu, res, F32), out_dtype=dtype)
    b.check()


# ------------------------------------------------------------------------------------------------ sy11_bn_act_bwd_reduce
@gpu
@per_config
def test_bn_act_bwd_reduce(reduction_mode, cid, dtype, row_map, silu, strided):
    """sum_g[c] += sum g, sum_gx[c] += sum g * xhat into PRE-LOADED slot rows, 1 / 3 / 8 / 13 of them: whatever slot a workgroup's
    partial lands in, the rows must add up to what they held before plus the sums (include/sy11.h: `+=`), in both modes.

    sum_bound depth (`_reduce_depth`): a term is added to a thread's accumulator (4 rows per trip x the trips of the walk), climbs the
    tree over the rows_pb row groups (ceil(log2 rows_pb) levels), and arrives at a slot row (`_arrivals`)."""
    c = _case(cid, dtype)
    s64, s32, absmax = _sums(cid, dtype, silu)
    geo = _geometry("reduce", c.M, c.C, dtype, row_map)
    b = Bars(f"bn_bwd_reduce[{reduction_mode} {cid} {str(dtype)[6:]} {'silu' if silu else 'linear'} {'slice' if strided else 'contig'} map{row_map} grid {geo['grid']}x{geo['cblocks']}]")
    yv, _ = nhwc_view(c.y, dtype, strided)
    dzv, _ = nhwc_view(c.dz, dtype, strided)
    with _row_map(row_map):
        for slots in SUM_SLOTS:
            pre = 0.5 + rnd(2, slots, c.C, seed=slots + c.C).abs()                      # every slot row holds something non-zero
            rows = pre.to(DEV, copy=True)
            ops().bn_act_bwd_reduce(yv, dzv, c.dev["mean"], c.dev["rstd"], c.dev["scale"], c.dev["shift"], silu, rows[0], rows[1])
            torch.cuda.synchronize()
            after = rows.cpu().double().sum(1)
            k = _reduce_depth(geo, slots, reduction_mode)
            for i, name in enumerate(("sum_g", "sum_gx")):
                held = pre[i].double().sum(0)
                b.add(f"{name}(slots {slots}, depth {k})", after[i], held + s64[i], (pre[i].sum(0) + s32[i]),
                      extra=sum_bound(k, absmax[i] + held.max().item()))
    b.check()


@gpu
@pytest.mark.parametrize("Cn", [2, 80])
def test_bias_gradient_through_the_reduce_kernel(reduction_mode, Cn):
    """What Conv's bias gradient does (nn/modules/conv.py): bn_act_bwd_reduce(dz, dz, 0, 1, 1, 0, silu=False) with f32 dz and ONE
    slot, adding into a live gradient vector.  C = 2: scalar path on 2 workgroups; C = 80: vector path on 17."""
    B, H, W = 2, 20, 20
    dz = rnd(Cn, seed=5, scale=0.5) + rnd(B, H, W, Cn, seed=6 + Cn)
    pre = rnd(2, Cn, seed=7 + Cn) + 2
    held = pre.to(DEV, copy=True)
    zero, one = torch.zeros(Cn, device=DEV), torch.ones(Cn, device=DEV)
    dzv = dz.to(DEV)
    ops().bn_act_bwd_reduce(dzv, dzv, zero, one, one, zero, False, held[0], held[1])
    torch.cuda.synchronize()
    geo = _geometry("reduce", B * H * W, Cn, F32)
    k = _reduce_depth(geo, 1, reduction_mode)
    d2 = dz.reshape(-1, Cn)
    b = Bars(f"bias_grad[{reduction_mode} C{Cn} grid {geo['grid']}]")
    b.add("dbias", held[0], pre[0].double() + d2.double().sum(0), pre[0] + d2.sum(0),
          extra=sum_bound(k, d2.abs().sum(0).max().item() + pre[0].abs().max().item()))
    b.add("scratch", held[1], pre[1].double() + (d2.double() ** 2).sum(0), pre[1] + (d2 * d2).sum(0),
          extra=sum_bound(k, (d2.double() ** 2).sum(0).max().item() + pre[1].abs().max().item()))
    b.check()


# ------------------------------------------------------------------------------------------------ sy11_bn_act_bwd_apply[_res]
RES_MODES = (None, False, True)                     # no residual gradient / res_grad = dz / res_grad += dz


@gpu
@per_config
def test_bn_act_bwd_apply(reduction_mode, cid, dtype, row_map, silu, strided):
    """dy = gamma * rstd * (g - sum_g / M - xhat * sum_gx / M) from GIVEN slot rows (1 / 3 / 8 / 13: the prologue's eight-at-a-time fold
    with ragged tails), dgamma += sum_gx and dbeta += sum_g into pre-loaded vectors, and the residual gradient (absent, =, +=), which
    is exact: one f32 add, one rounding.  Tensors above 2 M elements pair each slot count with one residual mode instead of all three.

    dgamma / dbeta: a slot row's value passes through `slots` sequential adds of the prologue and one add onto the pre-loaded value."""
    c = _case(cid, dtype)
    s64, _, _ = _sums(cid, dtype, silu)
    geo = _geometry("apply", c.M, c.C, dtype, row_map)
    b = Bars(f"bn_bwd_apply[{reduction_mode} {cid} {str(dtype)[6:]} {'silu' if silu else 'linear'} {'slice' if strided else 'contig'} map{row_map} grid {geo['grid']}x{geo['cblocks']}]")
    yv, _ = nhwc_view(c.y, dtype, strided)
    dzv, _ = nhwc_view(c.dz, dtype, strided)
    small = c.M * c.C <= 2_000_000
    want_res = {False: c.dz.to(dtype), True: (c.old + c.dz).to(dtype)}                # f32 add of two storage values, rounded once
    with _row_map(row_map):
        for n, slots in enumerate(SUM_SLOTS):
            rows = _split(s64, slots, seed=11 * slots + c.C)                           # [2, slots, C]
            rows_dev = rows.to(DEV)
            args = (c.y, c.dz, c.mean, c.rstd, c.scale, c.shift, c.gamma, silu, rows[0], rows[1], c.M)
            dy64, dg64, db64 = R.bwd_apply(*args, F64)
            dy32, dg32, db32 = R.bwd_apply(*args, F32)
            pre = rnd(2, c.C, seed=slots + 3) + 1.5
            for res_acc in (RES_MODES if small else (RES_MODES[n % 3],)):
                tag = f"(slots {slots}, res {'off' if res_acc is None else '+=' if res_acc else '='})"
                dyv, dybuf = _out_view(c.shape, dtype, strided)
                acc = pre.to(DEV, copy=True)
                resv, resbuf = nhwc_view(c.old, dtype, strided) if res_acc is not None else (None, None)
                ops().bn_act_bwd_apply(yv, dzv, c.dev["mean"], c.dev["rstd"], c.dev["scale"], c.dev["shift"], c.dev["gamma"], silu,
                                       rows_dev[0] if slots > 1 else rows_dev[0, 0], rows_dev[1] if slots > 1 else rows_dev[1, 0],
                                       dyv, acc[0], acc[1], res_grad=resv, res_accumulate=bool(res_acc))
                torch.cuda.synchronize()
                assert outside_untouched(dybuf, c.C), "dy written outside its channel slice " + tag
                dy = dyv.float().cpu()
                assert bool(torch.isfinite(dy[..., C_SAT]).all()), "the saturating channel's dy is not finite " + tag
                assert float(dy[..., C_ZERO].abs().max()) == 0.0, "gamma == 0 must give dy == 0 " + tag
                b.add("dy" + tag, dy, dy64, dy32, out_dtype=dtype)
                for i, (name, a64, a32) in enumerate((("dgamma", dg64, dg32), ("dbeta", db64, db32))):
                    terms = rows[1 - i].abs().sum(0) + pre[i].abs()
                    b.add(name + tag, acc[i], pre[i].double() + a64, pre[i] + a32, extra=sum_bound(slots + 1, terms.max().item()))
                if res_acc is not None:
                    assert outside_untouched(resbuf, c.C), "res_grad written outside its channel slice " + tag
                    assert torch.equal(resv.cpu(), want_res[res_acc]), "res_grad is not dz / old + dz rounded once " + tag
    b.check()
