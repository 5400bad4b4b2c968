"""Case table, integer alphabets, float64 references and a Python mirror of the dispatch of the first layer (csrc/direct.hip:
stem_fwd_kernel, stem_fwd_mma, stem_fwd_tile, stem_wgrad_kernel, stem_wgrad_mma, stem_wgrad_tile behind sy11_stem_conv_fwd[_bn]
and sy11_stem_conv_wgrad).

`stem_branches` restates `stem_fwd_tail`, `sy11_stem_conv_wgrad` and `stem_tiling` with the environment at its defaults
(SY11_STEM_TILE 1, 1024 forward and 512 filter-gradient workgroups).  It is a COPY, and it is checked on the device: after every
call tests/test_stem_kernels_gpu.py compares "stem_fwd_last" / "stem_wgrad_last" with it, so drift in either direction fails.

Two operand families, as in tests/_conv_ref.py.

* exact: integers.  "dense" alphabet x in [-2, 2], w in [-3, 3], dy in [-2, 2]: |y| <= 27 * 6 = 162 <= 256 is exact in bf16.  "sparse"
  alphabet (the two rows past the persistent caps, 136 500 and 546 000 pixels): x and dy in {-1, 0, 1} with a quarter non-zero, w in
  {-1, 0, 1}.  `assert_stem_exact_conditions` states what bit-equality in ANY summation order rests on and runs on every row.
* real: `R.real_case` unchanged (uniform [-1, 1] rounded through the dtype, elementwise order-independent bounds).

This module imports neither the package nor a device: tests/test_stem_ref_cpu.py runs all of it on the CPU.
"""
from __future__ import annotations

import functools

import torch
import torch.nn.functional as F

from tests import _conv_ref as R

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
GATHER, MMA, TILE_VEC, TILE_SCALAR = 1, 2, 3, 4          # csrc/tune.h SY11_STEM_*
FWD_WG_CAP, WGRAD_WG_CAP = 1024, 512                     # persistent workgroups (SY11_STEM_FWD_WG / SY11_STEM_WGRAD_WG defaults)
STILE_H, STILE_W = 4, 64

FIELDS = ("name", "dtype", "N", "B", "H", "W", "s", "p", "y_ld", "dy_ld", "bias", "silu", "slots", "mode")


def out_hw(H, W, s, p):
    return (H + 2 * p - 3) // s + 1, (W + 2 * p - 3) // s + 1


# ------------------------------------------------------------------------------------------------------------ dispatch mirror
def stem_tiling(B, H, W, s, p):
    """`stem_tiling` of direct.hip: the launch constants of the LDS-tiled kernels, or None where they refuse the shape."""
    if s < 1 or s > 2 or p < 0 or p > 3 or W < 4:
        return None
    OH, OW = out_hw(H, W, s, p)
    tiles_x, tiles_y = (OW + STILE_W - 1) // STILE_W, (OH + STILE_H - 1) // STILE_H
    tiles = B * tiles_y * tiles_x
    if tiles * tiles_x >= 2 ** 31 or tiles * tiles_y >= 2 ** 31:
        return None
    RH = (STILE_H - 1) * s + 3
    shift = (-p) & 3
    NV = (shift + (STILE_W - 1) * s + 3 + 3) >> 2
    if 3 * RH * NV > 256 * 4:
        return None
    return {"tiles_x": tiles_x, "tiles_y": tiles_y, "tiles": tiles, "RH": RH, "shift": shift, "NV": NV}


def stem_branches(dtype, N, B, H, W, s, p, y_ld=None, dy_ld=None, y_aligned=True, dy_aligned=True, x_aligned=True):
    """Which kernel sy11_stem_conv_fwd and sy11_stem_conv_wgrad launch: {"fwd": code, "wgrad": code}, codes as in csrc/tune.h."""
    y_ld = N if y_ld is None else y_ld
    dy_ld = N if dy_ld is None else dy_ld
    OH, OW = out_hw(H, W, s, p)
    sixteen = dtype != F32 and N in (32, 64)
    image_ok = B * 3 * H * W < 2 ** 31
    walk_ok = (OW + 64) * OW < 2 ** 20 and (OH + 64) * OH < 2 ** 20          # multiply-shift pixel walk of the gather MFMA kernels
    tiling = stem_tiling(B, H, W, s, p)
    tile_code = TILE_VEC if (W % 4 == 0 and x_aligned) else TILE_SCALAR
    mma = sixteen and y_ld == N and y_aligned and image_ok and walk_ok
    if mma and tiling:
        fwd = tile_code
    elif mma and p <= 1:               # the padding guard: stem_fwd_mma holds for padding 0 and 1 only
        fwd = MMA
    else:
        fwd = GATHER
    if sixteen and dy_ld % 8 == 0 and dy_aligned and image_ok:
        assert walk_ok, "sy11_stem_conv_wgrad refuses maps past 960 pixels per side on this path"
        wgrad = tile_code if tiling else MMA
    else:
        wgrad = GATHER
    return {"fwd": fwd, "wgrad": wgrad}


def stem_grids(dtype, N, B, H, W, s, p, **kw):
    """Workgroups and work items of the two launches: {"fwd": (workgroups, items), "wgrad": (workgroups, items)}; items are tiles
    for the tiled kernels (a workgroup loops when there are more items than workgroups), 256-pixel blocks / pixel chunks otherwise."""
    br = stem_branches(dtype, N, B, H, W, s, p, **kw)
    OH, OW = out_hw(H, W, s, p)
    M = B * OH * OW
    t = stem_tiling(B, H, W, s, p)
    out = {}
    if br["fwd"] >= TILE_VEC:
        out["fwd"] = (min(t["tiles"], FWD_WG_CAP), t["tiles"])
    else:
        out["fwd"] = ((M + 255) // 256,) * 2
    if br["wgrad"] >= TILE_VEC:
        out["wgrad"] = (min((t["tiles"] + 7) // 8, WGRAD_WG_CAP), t["tiles"])
    elif br["wgrad"] == MMA:
        nb = min((M + 2047) // 2048, 512)
        ppb = ((M + nb - 1) // nb + 127) // 128 * 128
        out["wgrad"] = ((M + ppb - 1) // ppb, (M + 127) // 128)
    else:
        nblk = min((M + 1023) // 1024, 2048)
        ppb = ((M + nblk - 1) // nblk + 63) // 64 * 64
        out["wgrad"] = ((M + ppb - 1) // ppb, (M + 63) // 64)
    return out


def n_class(N):
    """The NMAX template of the gather kernels that N falls into."""
    return 16 if N <= 16 else 32 if N <= 32 else 64


# ------------------------------------------------------------------------------------------------------------ case table
def _row(name, dtype, N, B, OH, OW, s, p, eh=0, ew=0, y_ld=None, dy_ld=None, bias=True, silu=False, slots=8, mode="exact"):
    """A table row from the OUTPUT map wanted: H, W are the smallest inputs that give (OH, OW), plus eh / ew (< s) spare lines."""
    assert 0 <= eh < s and 0 <= ew < s
    H, W = (OH - 1) * s + 3 - 2 * p + eh, (OW - 1) * s + 3 - 2 * p + ew
    assert H >= 1 and W >= 1 and out_hw(H, W, s, p) == (OH, OW), name
    return (name, dtype, N, B, H, W, s, p, N if y_ld is None else y_ld, N if dy_ld is None else dy_ld, bias, silu, slots, mode)


# Rows (name, dtype, N, B, H, W, s, p, y_ld, dy_ld, bias, silu, slots, mode).  A leading dimension above N puts the operand at channel
# offset (ld - N) / 2 of a wider buffer whose other channels hold a sentinel: N + 16 is a 16-byte-aligned slice, N + 4 a misaligned
# one with ld % 8 != 0.  mode: "exact" (dense alphabet), "exact-sparse", "exact-xoff" (the image starts one float into its
# buffer: contiguous, not 16-byte aligned), "real".  An exact row runs y with (N,) statistics, y with (slots, N) statistics, y + bias
# when `bias`, and dw after one and two calls, in both reduction modes.
EXACT_ROWS = [
    # LDS-tiled kernels: stride {1, 2} x padding {0, 1, 2, 3} (column shifts 0, 3, 2, 1), each with 16-byte image loads (W % 4 == 0)
    # and with element-wise fill; OW in {1, 63, 64, 65, 130}, OH in {1, 3, 4, 5, 9}
    _row("tile-s1p0-vec", F16, 32, 2, 9, 130, 1, 0),
    _row("tile-s1p0-fill", BF16, 64, 3, 3, 63, 1, 0),
    _row("tile-s1p1-vec", BF16, 32, 3, 1, 64, 1, 1),
    _row("tile-s1p1-fill", F16, 64, 1, 5, 65, 1, 1),
    _row("tile-s1p2-vec", F16, 64, 2, 4, 130, 1, 2),
    _row("tile-s1p2-fill", BF16, 32, 2, 5, 63, 1, 2),
    _row("tile-s1p3-vec", BF16, 64, 1, 9, 64, 1, 3),
    _row("tile-s1p3-fill", F16, 32, 3, 5, 130, 1, 3),
    _row("tile-s2p0-vec-iw4", F16, 32, 3, 1, 1, 2, 0, ew=1),                  # IW = 4: the smallest map the tiling takes
    _row("tile-s2p0-vec", BF16, 64, 2, 4, 63, 2, 0, ew=1),
    _row("tile-s2p0-fill", BF16, 32, 1, 5, 65, 2, 0, eh=1),
    _row("tile-s2p1-vec", F16, 64, 2, 9, 64, 2, 1, ew=1),
    _row("tile-s2p1-fill", BF16, 64, 3, 3, 65, 2, 1),
    _row("tile-s2p2-vec", BF16, 32, 2, 5, 63, 2, 2, ew=1),
    _row("tile-s2p2-fill", F16, 32, 1, 4, 130, 2, 2, eh=1),
    _row("tile-s2p3-vec", F16, 64, 1, 3, 130, 2, 3, ew=1),
    _row("tile-s2p3-fill", BF16, 64, 2, 9, 64, 2, 3),
    _row("tile-s1p1-xoff", F16, 32, 2, 4, 64, 1, 1, mode="exact-xoff"),          # W % 4 == 0 but a misaligned image: fill
    # slices on a tiled shape: y in a slice leaves the MFMA kernels; dy in an aligned slice stays, in a misaligned one leaves
    _row("tile-s2p1-yslice-dyslice8", F16, 32, 2, 5, 65, 2, 1, ew=1, y_ld=48, dy_ld=48),
    _row("tile-s2p1-dyslice4", BF16, 64, 2, 5, 65, 2, 1, ew=1, dy_ld=68),
    # gather MFMA kernels: stride 3 with padding 0 / 1, IW = 3; M = 84, 4, 714, 450, 30
    _row("mma-s3p0", F16, 32, 2, 6, 7, 3, 0, eh=2, ew=1),
    _row("mma-s3p0-tiny", BF16, 64, 1, 2, 2, 3, 0),
    _row("mma-s3p1", BF16, 32, 3, 14, 17, 3, 1, ew=2),
    _row("mma-iw3", F16, 64, 3, 50, 3, 1, 1),
    _row("mma-iw3-tiny", BF16, 32, 2, 5, 3, 1, 1),
    _row("mma-s3p1-yslice-dyslice8", BF16, 64, 2, 6, 7, 3, 1, y_ld=80, dy_ld=80),
    _row("mma-s3p0-dyslice4", F16, 32, 2, 6, 7, 3, 0, dy_ld=36),
    # the padding guard: forward on the gather kernel, filter gradient on the gather MFMA kernel
    _row("guard-s3p2", F16, 32, 2, 7, 8, 3, 2, eh=1),
    _row("guard-s1p4", BF16, 64, 2, 12, 15, 1, 4),
    _row("guard-s3p3", BF16, 32, 1, 5, 9, 3, 3, ew=2),
    # gather kernels: every N template at its width and strictly inside it; M = 1150 (five forward blocks, two ragged wgrad blocks)
    _row("gather-f32-n5", F32, 5, 2, 25, 23, 1, 1),
    _row("gather-f32-n16", F32, 16, 2, 25, 23, 2, 1, eh=1),
    _row("gather-f32-n24", F32, 24, 2, 25, 23, 1, 0),
    _row("gather-f32-n32", F32, 32, 2, 25, 23, 3, 2),
    _row("gather-f32-n48", F32, 48, 2, 25, 23, 2, 3, ew=1),
    _row("gather-f32-n64", F32, 64, 2, 25, 23, 1, 2),
    _row("gather-f16-n5", F16, 5, 2, 25, 23, 2, 1),
    _row("gather-f16-n24", F16, 24, 2, 25, 23, 1, 1),
    _row("gather-f16-n48", F16, 48, 2, 25, 23, 3, 0),
    _row("gather-bf16-n5", BF16, 5, 2, 25, 23, 1, 0),
    _row("gather-bf16-n24", BF16, 24, 2, 25, 23, 2, 2, eh=1),
    _row("gather-bf16-n48", BF16, 48, 2, 25, 23, 1, 1),
    _row("gather-f32-n32-slices", F32, 32, 2, 9, 11, 2, 1, y_ld=48, dy_ld=36),
    _row("gather-f16-n16-slices", F16, 16, 2, 9, 11, 2, 1, y_ld=20, dy_ld=32),
    # past the persistent caps (sparse alphabet): 1050 forward tiles for 1024 workgroups; 4200 tiles = 525 x 8 for 512 wgrad workgroups
    _row("cap-fwd", F16, 32, 3, 700, 65, 1, 1, mode="exact-sparse"),
    _row("cap-wgrad", BF16, 32, 12, 700, 65, 1, 1, mode="exact-sparse"),
]
CAP_ROWS = ("cap-fwd", "cap-wgrad")

# one shape per kernel and dtype: y, statistics, y + bias, SiLU with and without bias, dw
REAL_ROWS = [
    _row("real-tile-vec", F16, 32, 2, 9, 64, 2, 1, ew=1, silu=True, slots=1, mode="real"),
    _row("real-tile-vec", BF16, 64, 2, 9, 64, 2, 1, ew=1, silu=True, slots=1, mode="real"),
    _row("real-tile-fill", F16, 64, 2, 5, 71, 1, 2, silu=True, slots=1, mode="real"),
    _row("real-tile-fill", BF16, 32, 2, 5, 71, 1, 2, silu=True, slots=1, mode="real"),
    _row("real-mma", F16, 64, 2, 14, 17, 3, 1, silu=True, slots=1, mode="real"),
    _row("real-mma", BF16, 32, 2, 14, 17, 3, 1, silu=True, slots=1, mode="real"),
    _row("real-gather", F16, 24, 2, 14, 17, 2, 1, silu=True, slots=1, mode="real"),
    _row("real-gather", BF16, 48, 2, 14, 17, 2, 1, silu=True, slots=1, mode="real"),
    _row("real-gather", F32, 48, 2, 14, 17, 2, 1, silu=True, slots=1, mode="real"),
]

# stem_conv_fwd_bn: one exact row per forward kernel (the gather kernel has no fused tail: the library runs the finalize kernel)
BN_ROWS = ("gather-f16-n24", "mma-s3p1", "tile-s2p1-vec", "tile-s1p2-fill")


def row_dict(row):
    return dict(zip(FIELDS, row))


def row_id(row):
    return f"{row[0]}-{str(row[1])[6:]}"


def find_row(name):
    (row,) = [r for r in EXACT_ROWS if r[0] == name]
    return row


def slice_offset(ld, N):
    return (ld - N) // 2


def row_branches(row):
    """`stem_branches` of a row, with the alignment that the row's slice offsets and image offset give."""
    d = row_dict(row)
    esz = torch.empty((), dtype=d["dtype"]).element_size()
    return stem_branches(d["dtype"], d["N"], d["B"], d["H"], d["W"], d["s"], d["p"], d["y_ld"], d["dy_ld"],
                         y_aligned=(slice_offset(d["y_ld"], d["N"]) * esz) % 16 == 0,
                         dy_aligned=(slice_offset(d["dy_ld"], d["N"]) * esz) % 16 == 0, x_aligned=d["mode"] != "exact-xoff")


def promised():
    """Every (op, code, dtype, N template) that the rows of this table reach: what the GPU file must observe, no more and no less."""
    out = set()
    for row in EXACT_ROWS + REAL_ROWS:
        br = row_branches(row)
        out.add(("fwd", br["fwd"], row[1], n_class(row[2])))
        out.add(("wgrad", br["wgrad"], row[1], n_class(row[2])))
    return out


# ------------------------------------------------------------------------------------------------------------ operands, references
def stem_int_operands(N, B, H, W, s, p, sparse, seed=R.SEED):
    """(x, w, dy) of the exact family as float64 NCHW / OIHW tensors."""
    OH, OW = out_hw(H, W, s, p)
    gen = torch.Generator().manual_seed(seed)
    if not sparse:
        x = torch.randint(-2, 3, (B, 3, H, W), generator=gen).double()
        w = torch.randint(-3, 4, (N, 3, 3, 3), generator=gen).double()
        dy = torch.randint(-2, 3, (B, N, OH, OW), generator=gen).double()
        return x, w, dy

    def quarter(*shape):
        sign = torch.randint(0, 2, shape, generator=gen, dtype=torch.int8) * 2 - 1
        return (sign * (torch.rand(shape, generator=gen) < 0.25)).double()
    return quarter(B, 3, H, W), torch.randint(-1, 2, (N, 3, 3, 3), generator=gen).double(), quarter(B, N, OH, OW)


def assert_stem_exact_conditions(x, w, dy, y, dw, bias=None):
    """What bit-equality of y, the statistics and dw (after two accumulating calls) with float64 rests on, for ANY summation order.
    A failure means a row or an alphabet was edited into territory where a 16-bit store or an f32 sum rounds: fix the row, never
    the comparison."""
    for t in (x, w, dy, y, dw):
        assert torch.equal(t, t.round()), "operands and reference must be integers"
    assert max(x.abs().max().item(), w.abs().max().item(), dy.abs().max().item()) <= 256, "an operand is past the bf16-exact integers"
    ymax = y.abs().max().item() + (0 if bias is None else bias.abs().max().item())
    assert ymax <= 256, f"|y| (+ |bias|) = {ymax} is past the bf16-exact integers"
    s_abs, s_sq = y.abs().sum((0, 2, 3)).max().item(), (y * y).sum((0, 2, 3)).max().item()
    assert s_abs < 2 ** 24, f"per-channel sum |y| = {s_abs}: a partial sum could leave the exact f32 integers"
    assert s_sq < 2 ** 24, f"per-channel sum y^2 = {s_sq} is not an exact f32 integer"
    # sum_m |dy[m][n] * patch[m][k]| <= max|x| * sum_m |dy[m][n]|, and twice that after the second call
    s_dw = 2 * x.abs().max().item() * dy.abs().sum((0, 2, 3)).max().item()
    assert s_dw < 2 ** 24, f"2 sum |dy * patch| <= {s_dw}: a partial sum of dw could leave the exact f32 integers"


def int_bias(N):
    gen = torch.Generator().manual_seed(9)
    return torch.randint(-3, 4, (N,), generator=gen).double()


@functools.lru_cache(maxsize=2)
def _exact(N, B, H, W, s, p, sparse):
    x, w, dy = stem_int_operands(N, B, H, W, s, p, sparse)
    y, _, dw = R.conv_ref(x, w, dy, s, p, 1, 1)
    bias = int_bias(N)
    assert_stem_exact_conditions(x, w, dy, y, dw, bias)
    return {"x": x, "w": w, "dy": dy, "y": y, "dw": dw, "bias": bias}


def exact(row):
    """Operands and float64 results of an exact row, computed once and shared (callers must not write into them)."""
    d = row_dict(row)
    assert d["mode"].startswith("exact")
    return _exact(d["N"], d["B"], d["H"], d["W"], d["s"], d["p"], d["mode"] == "exact-sparse")


def real(row):
    d = row_dict(row)
    assert d["mode"] == "real"
    return R.real_case(d["B"], 3, d["N"], d["H"], d["W"], 3, d["s"], d["p"], 1, 1, d["dtype"])


def silu_refs(rr, s, p, bias):
    """float64 silu(conv + bias) and the same formula in f32 on the CPU from the same (already rounded) operands."""
    b64 = rr["bias"] if bias else torch.zeros_like(rr["bias"])
    r64 = F.silu(rr["y"] + b64.view(1, -1, 1, 1))
    r32 = F.silu(F.conv2d(rr["x"].float(), rr["w"].float(), b64.float(), s, p))
    return r64, r32
