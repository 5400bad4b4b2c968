"""The dense convolution kernels on the diagonal (3x3 / 1x1, pad k // 2, dilation 1): the case table of tests/test_igemm_kernels_gpu.py
and a Python restatement of the dispatch of csrc/igemm.hip (`cfg_legal`, `select_and_launch`, `sy11_conv2d_dgrad`) and csrc/wgrad.hip
(`sy11_conv2d_wgrad`) with the legality rules of conv3x3.hip, conv3x3s.hip, igemm8.hip and igemm8p.hip.

The restatement is a COPY, like `dw_branches` in tests/_conv_ref.py — but this one is checked on the device: after every call the
GPU tests read "igemm_last_cfg" / "wgrad_last_cfg" and compare with `expected_*`, so drift in either direction fails a test.
tests/test_igemm_ref_cpu.py holds the table to the rule: every configuration appears, in every dtype and epilogue it takes, on a
shape where the rule says it really runs.

A SHAPE is (B, C, N, H, W, k, s).  A ROW is (op, cfg, dtype, epi, shape name): op "fwd" / "dgrad" / "wgrad", epi the epilogue code of
`epi_code` in igemm.hip (1 statistics, 2 bias, 4 SiLU, 8 accumulate, 16 f32 output).  This module imports neither the package nor a device.
"""
from __future__ import annotations

import torch

from tests import _conv_ref as R

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
HALO_DGRAD_S2 = 100            # SY11_CFG_HALO_DGRAD_S2 (csrc/tune.h)
IGEMM_NCFG, WGRAD_NCFG = 26, 20
DEFAULT_OPTS = {"igemm_cfg": -1, "wgrad_cfg": -1, "igemm_deep": 0, "dgrad_s2_halo": 1}


def cdiv(a, b):
    return (a + b - 1) // b


def esize(dt):
    return 4 if dt == F32 else 2


# ------------------------------------------------------------------------------------------------------------ argument structs
def fwd_args(shape, dt, epi, x_ld=None, y_ld=None):
    """IgemmArgs as conv2d_fwd_impl fills them (igemm.hip), for pad k // 2, dilation 1; pointers are 16-byte aligned."""
    B, C, N, H, W, k, s = shape
    p = k // 2
    OH, OW = R.out_hw(H, W, k, s, p, 1)
    osz = 4 if epi & 16 else esize(dt)
    y_ld = N if y_ld is None else y_ld
    taps = [(r - p, q - p, r * k + q) for r in range(k) for q in range(k)]
    return dict(T=k * k, C=C, K=k * k * C, wK=k * k * C, M=B * OH * OW, N=N, x_ld=C if x_ld is None else x_ld, y_ld=y_ld, IH=H, IW=W,
                OH=OH, OW=OW, sy=s, sx=s, dense_out=True, epi=epi, taps=taps, vec_out=(y_ld * osz) % 16 == 0 and (N * osz) % 16 == 0)


def dgrad_launches(shape, dt, accumulate, dy_ld=None, dx_ld=None):
    """The per-parity IgemmArgs of sy11_conv2d_dgrad, in launch order (classes without a tap are left out)."""
    B, C, N, H, W, k, s = shape
    p = k // 2
    OH, OW = R.out_hw(H, W, k, s, p, 1)
    dx_ld = C if dx_ld is None else dx_ld
    out = []
    for ph in range(s):
        for pw in range(s):
            if ph >= H or pw >= W:
                continue
            taps = [((ph + p - r) // s, (pw + p - q) // s, r * k + q) for r in range(k) if (ph + p - r) % s == 0
                    for q in range(k) if (pw + p - q) % s == 0]
            if not taps:
                continue
            oh, ow = (H - ph + s - 1) // s, (W - pw + s - 1) // s
            out.append(dict(T=len(taps), C=N, K=len(taps) * N, wK=k * k * N, M=B * oh * ow, N=C, x_ld=N if dy_ld is None else dy_ld,
                            y_ld=dx_ld, IH=OH, IW=OW, OH=oh, OW=ow, sy=1, sx=1, dense_out=s == 1, epi=8 if accumulate else 0, taps=taps,
                            vec_out=(dx_ld * esize(dt)) % 16 == 0 and (C * esize(dt)) % 16 == 0))
    return out


# ------------------------------------------------------------------------------------------------------------ legality (copies)
def halo_tile(OW, OH, big):
    """conv3x3.hip halo_tile -> (th, tw) or None."""
    if OW % 16 == 0:
        th = 16 if (big and OH % 16 == 0) else 8
        return (th, 16) if (not big or th == 16) else None
    if OW == 20:
        return (12 if big else 6, 20)
    if OW == 40:
        return (6 if big else 3, 40)
    return None


def all_nine_taps(a):
    seen = set()
    for dy, dx, _ in a["taps"]:
        if not (-1 <= dy <= 1 and -1 <= dx <= 1):
            return False
        seen.add((dy, dx))
    return len(a["taps"]) == 9 and len(seen) == 9


def halo_bn(a, cfg):
    wide = 128 if a["N"] > 64 else (64 if a["N"] > 32 else 32)
    bn = wide if cfg in (15, 17) else (wide // 2 if wide > 32 else 0)
    return 0 if bn == 0 else (1000 + bn if cfg >= 17 else bn)


def halo3x3_legal(a, bn_code):
    big, bn = bn_code >= 1000, bn_code % 1000
    if big and (a["sy"] != 1 or bn < 64):
        return False
    if a["T"] != 9 or a["K"] != 9 * a["C"] or a["C"] % 32 or a["N"] % 8 or not a["dense_out"] or not a["vec_out"]:
        return False
    if (a["sy"], a["sx"]) not in ((1, 1), (2, 2)):
        return False
    if a["epi"] not in ((0, 1, 8, 6) if a["sy"] == 1 else (0, 1, 6)):
        return False
    if not all_nine_taps(a) or halo_tile(a["OW"], a["OH"], big) is None or bn not in (128, 64, 32):
        return False
    return not (bn > 32 and bn >= 2 * a["N"])


def smallc3x3_legal(a):
    if a["T"] != 9 or a["K"] != 9 * a["C"] or a["sy"] != 1 or a["sx"] != 1 or not a["dense_out"] or not a["vec_out"]:
        return False
    if a["C"] not in (16, 32) or a["N"] > 32 or a["N"] % 8 or a["x_ld"] % 8 or a["y_ld"] % 8 or a["wK"] % 8 or a["epi"] & 16:
        return False
    return all_nine_taps(a) and a["IH"] == a["OH"] and a["IW"] == a["OW"]


def igemm8_legal(a, bn, kb):
    if (bn == 64 and kb == 64) or (bn == 256 and kb != 64) or a["epi"] not in (0, 1, 8, 6):
        return False
    if not a["vec_out"] or a["M"] < 256 or a["K"] < 128 or a["C"] % 8:
        return False
    return a["N"] > 128 if bn == 256 else (a["N"] > 64 if bn == 128 else 32 < a["N"] <= 64)


def igemm8p_legal(a):
    return a["epi"] in (0, 1, 8, 6) and a["vec_out"] and a["M"] >= 256 and a["K"] >= 128 and a["N"] > 64 and a["C"] % 8 == 0


def cfg_legal(a, dt, cfg):
    """igemm.hip cfg_legal<T> (no BN tail ticket, debug 0)."""
    if cfg < 0 or cfg >= IGEMM_NCFG:
        return False
    epi = a["epi"]
    if 15 <= cfg <= 18:
        bn = halo_bn(a, cfg)
        return dt == F16 and bn > 0 and halo3x3_legal(a, bn)
    if cfg == 19:
        return dt != F32 and smallc3x3_legal(a)
    if cfg == 25:
        return dt == F16 and igemm8p_legal(a)
    if 20 <= cfg <= 24:
        return dt == F16 and igemm8_legal(a, 256 if cfg == 24 else (64 if cfg & 1 else 128), 128 if cfg < 22 else 64)
    if cfg in (7, 8):
        bn = 128 if cfg == 7 else 64
        if dt == F32 or a["T"] != 1 or a["taps"][0][:2] != (0, 0) or a["sy"] != 1 or a["sx"] != 1 or not a["dense_out"] or not a["vec_out"]:
            return False
        if epi not in (0, 1, 8, 6) or a["K"] % 32 or a["K"] != a["C"] or a["wK"] != a["K"] or a["N"] % 8:
            return False
        if a["N"] <= (64 if cfg == 7 else 32):
            return False
        return (a["K"] // 32) * 64 * (bn + 256) + 128 * bn * 2 <= 150 * 1024
    if cfg >= 9:
        if dt != F16 or epi not in (0, 1, 8, 6):
            return False
        return a["K"] >= (384 if cfg >= 12 else 128)
    if cfg >= 4:
        return a["K"] >= 256
    if cfg != 3:
        return True
    return dt == F16 and epi in (0, 1, 8, 6) and a["N"] > 64 and a["M"] >= 256


def heuristic_igemm(a, dt):
    bn = 128 if a["N"] > 64 else (64 if a["N"] > 32 else 32)
    while bn > 32 and cdiv(a["M"], 128) * cdiv(a["N"], bn) < 512:
        bn >>= 1
    cfg = {128: 0, 64: 1, 32: 2}[bn]
    if a["sy"] == 1 and a["T"] == 9 and cfg_legal(a, dt, 15):
        th, tw = (6, 20) if a["OW"] == 20 else ((3, 40) if a["OW"] == 40 else (8, 16))
        wgs = (a["M"] // (a["OH"] * a["OW"])) * cdiv(a["OH"], th) * cdiv(a["OW"], tw) * cdiv(a["N"], halo_bn(a, 15) % 1000)
        cfg = 16 if (wgs < 400 and cfg_legal(a, dt, 16)) else 15
    if cfg_legal(a, dt, 19):
        cfg = 19
    return cfg


def pick_key(a, dt):
    """The problem hash of select_and_launch's pick table (tune.h `hash` over the key ints) — what sy11_tune_import takes."""
    key = [esize(dt), a["M"], a["N"], a["K"], a["C"], a["T"], a["sy"], a["sx"], a["IW"], a["OW"], a["x_ld"], a["y_ld"], int(a["dense_out"]),
           4 if a["epi"] & 16 else 0]
    h = 1469598103934665603
    for v in key:
        h = ((h ^ (v & 0xffffffff)) * 1099511628211) & 0xffffffffffffffff
    return h


def select_igemm(a, dt, opts):
    """select_and_launch<T> with "tune" 0 and a pick table that is empty, or holds `opts["pick"]` for this problem."""
    forced, deep = opts.get("igemm_cfg", -1), opts.get("igemm_deep", 0)
    if forced >= 0 and cfg_legal(a, dt, forced):
        return forced
    cfg = heuristic_igemm(a, dt)
    if opts.get("pick") is not None and cfg_legal(a, dt, opts["pick"]):
        cfg = opts["pick"]
    if deep > 0:
        nwg = cdiv(a["M"], 128) * cdiv(a["N"], 64 if cfg % 4 == 1 else (32 if cfg % 4 == 2 else 128))
        if deep >= 2 or nwg <= 1024:
            up = cfg + 9 if cfg <= 2 else (cfg + 8 if 4 <= cfg <= 6 else -1)
            if up >= 0 and cfg_legal(a, dt, up):
                cfg = up
    return cfg


def halo_dgrad_s2_legal(shape, dy_ld=None, dx_ld=None):
    B, C, N, H, W, k, s = shape
    OH, OW = R.out_hw(H, W, k, s, k // 2, 1)
    if N % 32 or C % 8 or halo_tile(OW, OH, False) is None:
        return False
    if ((C if dx_ld is None else dx_ld) * 2) % 16 or ((N if dy_ld is None else dy_ld) * 2) % 16:
        return False
    return H in (2 * OH, 2 * OH - 1) and W in (2 * OW, 2 * OW - 1)


def wgrad3x3p_ws(shape):
    """wgrad.hip wgrad3x3p_ws for pad k // 2, dilation 1 (the taps are then in row-major order)."""
    B, C, N, H, W, k, s = shape
    if k != 3 or s != 1 or C % 8 or N % 8:
        return 0
    ws = 80 if W % 80 == 0 else (40 if W == 40 else (20 if W == 20 else 0))
    return ws if ws and H % (80 // ws) == 0 else 0


def wgrad3x3p_sp(shape, ws):
    return 160 if ws >= 40 and shape[3] % (160 // ws) == 0 else 80


# ------------------------------------------------------------------------------------------------------------ expected configuration
def expected_fwd(shape, dt, epi, opts=DEFAULT_OPTS, x_ld=None, y_ld=None):
    return select_igemm(fwd_args(shape, dt, epi, x_ld, y_ld), dt, opts)


def expected_dgrad(shape, dt, accumulate, opts=DEFAULT_OPTS, dy_ld=None, dx_ld=None):
    """What "igemm_last_cfg" holds after sy11_conv2d_dgrad: the LAST parity launch, or HALO_DGRAD_S2."""
    B, C, N, H, W, k, s = shape
    if dt == F16 and (k, s) == (3, 2) and opts.get("igemm_cfg", -1) < 0 and opts.get("dgrad_s2_halo", 1) != 0 \
            and halo_dgrad_s2_legal(shape, dy_ld, dx_ld):
        return HALO_DGRAD_S2
    return select_igemm(dgrad_launches(shape, dt, accumulate, dy_ld, dx_ld)[-1], dt, opts)


def expected_wgrad(shape, dt, opts=DEFAULT_OPTS):
    B, C, N, H, W, k, s = shape
    OH, OW = R.out_hw(H, W, k, s, k // 2, 1)
    M, K = B * OH * OW, k * k * C
    cfg = (4 if (N > 64 and K > 64 and M > 30000) else 0) + 2
    if dt != F32 and M >= 200000 and wgrad3x3p_ws(shape):
        cfg = 14
    forced = opts.get("wgrad_cfg", -1)
    ncfg = 8 if dt == F32 else WGRAD_NCFG

    def patch_ok(c):
        return c < 12 or (wgrad3x3p_ws(shape) != 0 if c < 16 else (N > 64 and K > 128))
    return forced if (0 <= forced < ncfg and patch_ok(forced)) else cfg


def expected_cfg(row, forced, options=None):
    """The configuration the library must report after running `row` with `forced` in igemm_cfg / wgrad_cfg: forced when legal, the
    heuristic otherwise, igemm_deep applied to the heuristic pick.  `options`: other option values, and x_ld / y_ld / dy_ld / dx_ld."""
    op, _, dt, epi, name = row
    o = dict(DEFAULT_OPTS, **(options or {}))
    lds = {k: o.pop(k) for k in ("x_ld", "y_ld", "dy_ld", "dx_ld") if k in o}
    shape = SHAPES[name]["shape"]
    if op == "wgrad":
        return expected_wgrad(shape, dt, dict(o, wgrad_cfg=forced))
    o["igemm_cfg"] = forced
    if op == "fwd":
        return expected_fwd(shape, dt, epi, o, lds.get("x_ld"), lds.get("y_ld"))
    return expected_dgrad(shape, dt, bool(epi & 8), o, lds.get("dy_ld"), lds.get("dx_ld"))


# ------------------------------------------------------------------------------------------------------------ the table
# which dtypes a configuration is compiled for, and the forward epilogues launch_cfg specialises for it (bf16 always runs the
# runtime-flag build, EPI = -1).  3 = statistics + bias: no specialisation, reaches the -1 build in f16 and f32 too.
ALL, HALF, F16_ONLY = (F32, F16, BF16), (F16, BF16), (F16,)
FWD_EPIS_FULL, FWD_EPIS_TRAIN = (1, 0, 2, 18, 6, 3), (1, 0, 6)
DGRAD_EPIS = (0, 8)


def igemm_dtypes(cfg):
    if cfg in (0, 1, 2, 4, 5, 6):
        return ALL
    return HALF if cfg in (7, 8, 19) else F16_ONLY


def fwd_epis(cfg):
    if cfg in (0, 1, 2, 4, 5, 6):
        return FWD_EPIS_FULL
    return (1, 0, 2, 6, 3) if cfg == 19 else FWD_EPIS_TRAIN


def wgrad_dtypes(cfg):
    return ALL if cfg < 8 else HALF


# configuration 23 (64 channels x 64-byte stages) is in the table of igemm.hip but sy11_igemm8_legal refuses it for every problem
# ("not instantiated"): it can never run, and the table below says so instead of pretending.
NEVER_LEGAL_IGEMM = (23,)

# name -> shape (B, C, N, H, W, k, s), density of non-zero operands, and per op the configurations forced on it.  `-1` in a list
# is the heuristic.  Every shape is the smallest that reaches the edge named.
SHAPES = {
    # M = 286 = 2 x 128 + 30 = 256 + 30 (ragged 128- and 256-row tiles), N = 160 = 128 + 32 (ragged 128 / 64 / 256 tiles), K = 360:
    # no multiple of a 64- or 128-byte stage, C = 40 smaller than one stage (several taps per stage), igemm_korder degrades to 0
    "c40": dict(shape=(2, 40, 160, 13, 11, 3, 1), density=0.5, fwd=[-1, 0, 1, 2, 3, 4, 5, 6, 9, 10, 11, 20, 22, 24, 25],
                dgrad=[-1, 0, 1, 2, 4, 5, 6, 9, 10, 11], wgrad=[-1]),
    # C = 192 = whole 64- and 128-byte stages (the two K orders differ), K = 1728 (27 128-byte stages: every ring wraps), M = 288;
    # C > 128 and N = 128 > 64 make 3, 20, 22, 24, 25 legal in the input gradient too (there N and C swap roles)
    "c192": dict(shape=(2, 192, 128, 12, 12, 3, 1), density=0.5, fwd=[-1, 0, 1, 2, 3, 4, 5, 6, 9, 10, 11, 12, 13, 14, 20, 22, 25],
                 dgrad=[-1, 0, 2, 3, 4, 9, 12, 13, 14, 20, 22, 24, 25], wgrad=[-1]),
    # 1x1, K = 384: exactly at the boundary of 12..14 (and, in the input gradient, K = 72 < 128: nothing deep is legal)
    "k384": dict(shape=(1, 384, 72, 16, 17, 1, 1), density=0.5, fwd=[-1, 4, 12, 13, 14], dgrad=[-1, 0, 1], wgrad=[-1]),
    # 1x1 persistent: K = 128 is the largest the 128-channel form holds in LDS, and the K boundary of 9..11 and 20..25; M = 300
    "p1x1": dict(shape=(1, 128, 96, 15, 20, 1, 1), density=0.5, fwd=[-1, 7, 8, 9, 10, 11, 20, 22, 25], dgrad=[-1, 7, 8], wgrad=[-1]),
    # halo 8 x 16 tiles with a partial last tile row (20 = 2 x 8 + 4); N = 48 (32 < N <= 64) and, in the input gradient, C = 64:
    # the only homes of configuration 21
    "h8x16": dict(shape=(1, 64, 48, 20, 16, 3, 1), density=0.5, fwd=[-1, 15, 16, 21], dgrad=[-1, 21], wgrad=[-1]),
    # halo 6 x 20 (9 = 6 + 3) with the 128- and 64-channel tiles, ragged in both (N = 160 forward, 96 in the input gradient)
    "h6x20": dict(shape=(1, 96, 160, 9, 20, 3, 1), density=0.5, fwd=[15, 16], dgrad=[-1, 15, 16], wgrad=[-1]),
    # halo 3 x 40 (4 = 3 + 1), N = 64: 64- and 32-channel tiles; the input gradient has 32 channels: the 32-channel tile
    "h3x40": dict(shape=(1, 32, 64, 4, 40, 3, 1), density=0.5, fwd=[15, 16], dgrad=[15], wgrad=[-1]),
    # the 256-pixel halo tiles: 16 x 16, 12 x 20 (14 = 12 + 2), 6 x 40 (8 = 6 + 2), 128- and 64-channel tiles
    "H16x16": dict(shape=(1, 64, 96, 16, 32, 3, 1), density=0.5, fwd=[17, 18], dgrad=[17], wgrad=[-1]),
    "H12x20": dict(shape=(1, 96, 96, 14, 20, 3, 1), density=0.5, fwd=[17, 18], dgrad=[17, 18], wgrad=[]),
    "H6x40": dict(shape=(1, 32, 72, 8, 40, 3, 1), density=0.5, fwd=[17, 18], dgrad=[-1], wgrad=[]),
    # stride 2 from odd input sizes -> 16 x 20 (the patch runs past the right / bottom border); the input gradient is the
    # fused-parity kernel (64-channel tile: C = 64 > 32), and the same problem as four parity launches with dgrad_s2_halo = 0
    "s2odd": dict(shape=(1, 64, 64, 31, 39, 3, 2), density=0.5, fwd=[-1, 0, 15, 16], dgrad=[-1, 0, 2], wgrad=[-1]),
    # stride 2 from even sizes -> 9 x 16 (partial tile row), C = 32: the fused-parity kernel's 32-channel tile
    "s2even": dict(shape=(2, 32, 64, 18, 32, 3, 2), density=0.5, fwd=[15, 16], dgrad=[-1], wgrad=[-1]),
    # few-channel kernel: 4 x 64 tiles ragged both ways (6 = 4 + 2, 70 = 64 + 6), C = 16; 8 x 32 tiles (96 % 64 != 0), C = 32, N = 24
    "fc16": dict(shape=(2, 16, 32, 6, 70, 3, 1), density=0.5, fwd=[-1, 19, 2], dgrad=[-1, 19], wgrad=[-1]),
    "fc32": dict(shape=(1, 32, 24, 9, 96, 3, 1), density=0.5, fwd=[19], dgrad=[-1], wgrad=[]),
    # vec_out false: output rows that are no multiple of 16 bytes (N = 20 in 16 bits, N = 18 in f32) take the scalar epilogue; forward
    # only (the gradients' entry points want 16-byte channel counts)
    "n20": dict(shape=(1, 40, 20, 5, 7, 3, 1), density=0.5, fwd=[-1, 0, 1, 2], dgrad=[], wgrad=[], dtypes=(F16, BF16)),
    "n18": dict(shape=(1, 40, 18, 5, 7, 3, 1), density=0.5, fwd=[-1, 0, 1, 2], dgrad=[], wgrad=[], dtypes=(F32,)),
    # filter gradient: M = 1056 > 1024 (three pixel splits: the partial-dW fold in ordered mode), K = 360 and N = 72 ragged for
    # the 64-, 128- and 128 x 256 tiles
    "w1056": dict(shape=(2, 40, 72, 24, 22, 3, 1), density=0.5, fwd=[], dgrad=[], wgrad=list(range(12)) + [16, 17, 18, 19]),
    # the wide tile with whole and partial tiles both ways at stride 2: N = 136, K = 360
    "wide_s2": dict(shape=(1, 40, 136, 23, 31, 3, 2), density=0.5, fwd=[], dgrad=[], wgrad=[5, 16, 19]),
}
# every instantiation of the patch filter-gradient kernel: (ws, sp) x (CB, NB), partial 32- / 64-blocks (C = 24 / 72, N = 16 / 72)
PATCH_TILINGS = {(80, 160): (2, 80), (80, 80): (3, 80), (40, 160): (4, 40), (40, 80): (2, 40), (20, 80): (4, 20)}
for _i, ((_ws, _sp), (_h, _w)) in enumerate(PATCH_TILINGS.items()):
    for _j, (_c, _n) in enumerate(((24, 16), (24, 72), (72, 16), (72, 72))):
        SHAPES[f"patch{_ws}_{_sp}_c{_c}n{_n}"] = dict(shape=(1, _c, _n, _h, _w, 3, 1), density=0.5, fwd=[], dgrad=[],
                                                      wgrad=[12 + (_i + _j) % 4])


def rows():
    """Every row of the table: (op, cfg forced (-1 = heuristic), dtype, epi, shape name)."""
    out = []
    for name, e in SHAPES.items():
        only = e.get("dtypes", ALL)
        for cfg in e["fwd"]:
            for dt in [d for d in (ALL if cfg < 0 else igemm_dtypes(cfg)) if d in only]:
                out += [("fwd", cfg, dt, epi, name) for epi in (FWD_EPIS_FULL if cfg < 0 else fwd_epis(cfg))
                        if not (e["shape"][6] == 2 and 15 <= cfg <= 18 and epi == 8)]
        for cfg in e["dgrad"]:
            for dt in [d for d in (ALL if cfg < 0 else igemm_dtypes(cfg)) if d in only]:
                out += [("dgrad", cfg, dt, epi, name) for epi in DGRAD_EPIS]
        for cfg in e["wgrad"]:
            for dt in [d for d in (ALL if cfg < 0 else wgrad_dtypes(cfg)) if d in only]:
                out.append(("wgrad", cfg, dt, 0, name))
    return out


def rows_of(name, dt):
    return [r for r in rows() if r[4] == name and r[2] == dt]


def shape_dtype_pairs():
    """(shape name, dtype) pairs that have rows, in table order: the GPU test's parametrisation (one float64 reference per shape)."""
    seen = []
    for (_, _, dt, _, name) in rows():
        if (name, dt) not in seen:
            seen.append((name, dt))
    return sorted(seen, key=lambda nd: list(SHAPES).index(nd[0]))


def case10(name):
    B, C, N, H, W, k, s = SHAPES[name]["shape"]
    return (B, C, N, H, W, k, s, k // 2, 1, 1)


def exact(name):
    return R.exact_case(*case10(name), density=SHAPES[name]["density"])


# forced-but-illegal: (op, forced cfg, dtype, epi, shape) — one per legality clause; the library must run the heuristic pick instead
FALLBACK_SHAPES = {
    "c120": (1, 120, 72, 16, 17, 1, 1),        # K = 120 < 128: 9..11, 20..25
    "c248": (1, 248, 72, 16, 17, 1, 1),        # K = 248 < 256: 4..6
    "c376": (1, 376, 72, 16, 17, 1, 1),        # K = 376 < 384: 12..14
    "n64": (1, 128, 64, 15, 20, 1, 1),         # N = 64: configuration 7 (and 3, 20) want more than 64 channels
    "m255": (1, 128, 96, 15, 17, 1, 1),        # M = 255: 3, 20..25
    "w18": (1, 32, 48, 20, 18, 3, 1),          # width 18: no halo tile
    "c48": (2, 48, 32, 6, 70, 3, 1),           # C = 48: not a few-channel shape
}
SHAPES.update({n: dict(shape=s, density=0.5, fwd=[], dgrad=[], wgrad=[]) for n, s in FALLBACK_SHAPES.items()})
FALLBACK_ROWS = [
    ("fwd", 9, F16, 1, "c120"), ("fwd", 20, F16, 1, "c120"), ("fwd", 25, F16, 0, "c120"),
    ("fwd", 4, F16, 1, "c248"), ("fwd", 5, F32, 1, "c248"),
    ("fwd", 12, F16, 1, "c376"),
    ("fwd", 3, BF16, 1, "c192"), ("fwd", 9, BF16, 1, "c192"), ("fwd", 20, BF16, 1, "c192"), ("fwd", 15, BF16, 1, "h8x16"),
    ("fwd", 19, F32, 1, "fc16"), ("fwd", 7, F32, 1, "p1x1"),
    ("fwd", 9, F16, 2, "c192"), ("fwd", 3, F16, 2, "c192"), ("fwd", 20, F16, 18, "c192"), ("fwd", 7, F16, 2, "p1x1"), ("fwd", 15, F16, 2, "h8x16"),
    ("fwd", 7, F16, 1, "n64"), ("fwd", 3, F16, 1, "n64"), ("fwd", 20, F16, 1, "n64"), ("fwd", 24, F16, 1, "c192"), ("fwd", 21, F16, 1, "c192"),
    ("fwd", 20, F16, 1, "m255"), ("fwd", 3, F16, 1, "m255"), ("fwd", 25, F16, 1, "m255"),
    ("fwd", 15, F16, 1, "w18"), ("fwd", 17, F16, 1, "h8x16"), ("fwd", 18, F16, 1, "h3x40"), ("fwd", 7, F16, 1, "c192"),
    ("fwd", 19, F16, 1, "c48"), ("fwd", 23, F16, 1, "c192"), ("fwd", 26, F16, 1, "c192"),
    ("dgrad", 15, F16, 0, "s2even"), ("dgrad", 7, F16, 0, "c192"),
    ("wgrad", 16, F16, 0, "n64"), ("wgrad", 12, F16, 0, "c192"), ("wgrad", 8, F32, 0, "c192"), ("wgrad", 20, F16, 0, "c192"),
]

# the real-valued family: one shape per distinct KERNEL, (label, op, cfg, shape name, dtypes).  A "fwd" entry runs forward, input
# gradient and (at the heuristic) filter gradient of its shape; a "wgrad" entry the filter gradient alone.
REAL_KERNELS = [
    ("igemm 64-byte stages x2", "fwd", 0, "c40", ALL), ("igemm 128-byte stages x2", "fwd", 4, "c40", ALL),
    ("igemm 64-byte stages x4", "fwd", 9, "c40", F16_ONLY), ("igemm 128-byte stages x3", "fwd", 12, "k384", F16_ONLY),
    ("igemm 256x128", "fwd", 3, "c40", F16_ONLY), ("1x1 persistent", "fwd", 7, "p1x1", HALF),
    ("halo 128-pixel", "fwd", 15, "h8x16", F16_ONLY), ("halo 256-pixel", "fwd", 17, "H16x16", F16_ONLY),
    ("few-channel", "fwd", 19, "fc16", HALF),
    ("igemm8 kb128", "fwd", 20, "c40", F16_ONLY), ("igemm8 kb64", "fwd", 22, "c40", F16_ONLY), ("igemm8 bn256", "fwd", 24, "c40", F16_ONLY),
    ("igemm8p", "fwd", 25, "c40", F16_ONLY), ("halo_dgrad_s2", "dgrad", -1, "s2odd", F16_ONLY),
    ("wgrad_kernel<float>", "wgrad", 2, "w1056", (F32,)), ("wgrad16 plain", "wgrad", 2, "w1056", HALF),
    ("wgrad16 pixel-split", "wgrad", 10, "w1056", HALF), ("wgrad patch", "wgrad", 14, "patch40_160_c72n72", HALF),
    ("wgrad wide tile", "wgrad", 18, "w1056", HALF),
]


def real(name, dt):
    return R.real_case(*case10(name), dtype=dt)


# ------------------------------------------------------------------------------------------------------------ sensitivity
def _blocks_all_hit(t, bp, bc, reach):
    """t: [B, ch, H, W] -> True when every (bp consecutive pixels in B, H, W order) x (bc channels) block holds a non-zero.
    `reach` [B, 1, H, W]: the pixels the tap can reach at all (a ragged last block that lies inside a border row is out of the
    reach of the taps that point across that border: no operand could change it)."""
    B, ch, H, W = t.shape
    m = (t != 0).permute(0, 2, 3, 1).reshape(-1, ch)
    ok = (reach != 0).expand(B, 1, H, W).permute(0, 2, 3, 1).reshape(-1)
    for p0 in range(0, m.shape[0], bp):
        if not ok[p0:p0 + bp].any():
            continue
        for c0 in range(0, ch, bc):
            if not m[p0:p0 + bp, c0:c0 + bc].any():
                return False
    return True


def tap_filter(w, r, q, lo=None, hi=None, out_slab=False):
    """w with everything but tap (r, q) — and, when given, but input channels (or, out_slab, filters) lo..hi of it — zeroed."""
    m = torch.zeros_like(w)
    if lo is None:
        m[:, :, r, q] = w[:, :, r, q]
    elif out_slab:
        m[lo:hi, :, r, q] = w[lo:hi, :, r, q]
    else:
        m[:, lo:hi, r, q] = w[:, lo:hi, r, q]
    return m


def sensitivity_failures(name):
    """Sparse operands must not blind the exact comparison: returns the list of (what, tap, slab) whose removal leaves some
    (128-pixel x 32-channel) block of y or of a parity class of dx — or, for dw, some 64 x 64 block — unchanged."""
    B, C, N, H, W, k, s, p, d, g = case10(name)
    r_ = exact(name)
    x, w, dy = r_["x"], r_["w"], r_["dy"]
    import torch.nn.functional as F
    bad = []
    one_x, one_dy, one_w = torch.ones_like(x[:, :1]), torch.ones_like(dy[:, :1]), torch.ones(1, 1, k, k, dtype=torch.float64)
    opad = (H - ((dy.shape[2] - 1) * s - 2 * p + k), W - ((dy.shape[3] - 1) * s - 2 * p + k))
    for r in range(k):
        for q in range(k):
            reach_y = F.conv2d(one_x, tap_filter(one_w, r, q), None, s, p)
            reach_dx = F.conv_transpose2d(one_dy, tap_filter(one_w, r, q), None, s, p, opad)[:, :, (r - p) % s::s, (q - p) % s::s]
            whole_y = torch.zeros_like(r_["y"])
            for c0 in range(0, C, 32):
                part = F.conv2d(x, tap_filter(w, r, q, c0, c0 + 32), None, s, p)
                whole_y += part
                if not _blocks_all_hit(part, 128, 32, reach_y):
                    bad.append(("y", (r, q), c0))
            if not _blocks_all_hit(whole_y, 128, 32, reach_y):
                bad.append(("y", (r, q), None))
            whole_dx = torch.zeros_like(r_["dx"])
            for n0 in range(0, N, 32):
                part = F.conv_transpose2d(dy, tap_filter(w, r, q, n0, n0 + 32, out_slab=True), None, s, p, opad)
                whole_dx += part
                cls = part[:, :, (r - p) % s::s, (q - p) % s::s]          # the parity class this tap reaches
                if not _blocks_all_hit(cls, 128, 32, reach_dx):
                    bad.append(("dx", (r, q), n0))
            if not _blocks_all_hit(whole_dx[:, :, (r - p) % s::s, (q - p) % s::s], 128, 32, reach_dx):
                bad.append(("dx", (r, q), None))
    OH, OW = dy.shape[2:]
    for b in range(B):
        for p0 in range(0, OH * OW, 64):
            m = torch.zeros(OH * OW, dtype=torch.bool)
            m[p0:p0 + 64] = True
            part = torch.nn.grad.conv2d_weight(x[b:b + 1], w.shape, dy[b:b + 1] * m.view(1, 1, OH, OW), s, p)
            flat = (part != 0).permute(0, 2, 3, 1).reshape(N, -1)          # [N][tap][c]: the K order of dW
            # taps these pixels can reach at all (a stage inside the first row never meets the taps that point above it)
            reach = torch.nn.grad.conv2d_weight(one_x[:1], one_w.shape, one_dy[:1] * m.view(1, 1, OH, OW), s, p).reshape(-1) != 0
            cols = reach.repeat_interleave(C)
            if not all(flat[n0:n0 + 64, k0:k0 + 64].any() for n0 in range(0, N, 64) for k0 in range(0, flat.shape[1], 64)
                       if cols[k0:k0 + 64].any()):
                bad.append(("dw", b, p0))
    return bad


# ------------------------------------------------------------------------------------------------------------ deliberate mistakes
def mistakes(r, case, ops=("fwd", "dgrad", "wgrad")):
    """Six wrong kernels, applied to the float64 results `r` of `case` (B, C, N, H, W, k, s, p, d, g): name -> (key, wrong tensor),
    key one of y / sum / y_wide / dx / dw.  A mistake that the geometry cannot make (no border at 1x1, no parity at stride 1) is left
    out, and so is one in a result that none of `ops` computes.  `y_wide` is y with one more channel (the neighbour of the slice): the sentinel
    there must survive."""
    import torch.nn.functional as F
    B, C, N, H, W, k, s, p, d, g = case
    x, w, dy, y = r["x"], r["w"], r["dy"], r["y"]
    OH, OW = y.shape[2:]
    out = {}
    if k == 3 and s == 1 and "fwd" in ops:
        # the right neighbour of the last column is the first pixel of the next row: a border mask one column too wide
        t = y.clone()
        t[0, :, 0, OW - 1] += w[:, :, 1, 2] @ x[0, :, 1, 0]
        out["one border tap of one corner pixel"] = ("y", t)
    if "fwd" in ops:
        n0 = (N - 1) // 32 * 32
        c0 = max(C - 32, 0)
        t = y.clone()
        t[:, n0:] -= F.conv2d(x, tap_filter(w, k - 1, k - 1, c0, C), None, s, p)[:, n0:]
        out["the last K stage of the last channel tile"] = ("y", t)
        out["the last row of a ragged pixel tile left out of the statistics"] = ("sum", y.sum((0, 2, 3)) - y[B - 1, :, OH - 1, OW - 1])
        out["a channel tile written one channel too wide"] = ("y_wide", torch.cat([y, y[:, :1] * 0 + 1], 1))
    if s == 2 and "dgrad" in ops:
        t = r["dx"].clone()
        t[:, :, 1::2, 1::2] = 0
        out["one parity class of a stride-2 dx"] = ("dx", t)
    if "wgrad" not in ops:
        return out
    M = OH * OW
    m = torch.zeros(M, dtype=torch.bool)
    m[M - max(64, M // 3):] = True
    part = torch.nn.grad.conv2d_weight(x[B - 1:], w.shape, dy[B - 1:] * m.view(1, 1, OH, OW), s, p)
    out["one pixel split missing from dW"] = ("dw", r["dw"] - part)
    return out


def mistake_reference(r, key, sentinel=77.0):
    y = r["y"]
    return {"y": y, "sum": y.sum((0, 2, 3)), "y_wide": torch.cat([y, y[:, :1] * 0 + sentinel], 1), "dx": r["dx"], "dw": r["dw"]}[key]


def mistake_bound(rr, key):
    """The real family's bound for `key` (the neighbour of a slice may not change at all: bound 0)."""
    if key == "y_wide":
        return torch.cat([rr["bound_y"], rr["bound_y"][:, :1] * 0], 1)
    return {"y": rr["bound_y"], "sum": rr["bound_sum"], "dx": rr["bound_dx"], "dw": rr["bound_dw"]}[key]


# ------------------------------------------------------------------------------------------------------------ f32 emulation
def mfma_ordered_sums(rr, case, chunk=16):
    """y and dw of a real case as a kernel computes them at best: float32 products, float32 accumulation in chunks of one MFMA's
    K depth (16), K in tap-major order for y and pixels in order for dw."""
    import torch.nn.functional as F
    B, C, N, H, W, k, s, p, d, g = case
    x, w, dy = rr["x"].float(), rr["w"].float(), rr["dy"].float()
    cols = F.unfold(x, k, 1, p, s)                                       # [B][C * k * k][L], rows ordered (c, r, q)
    A = cols.view(B, C, k * k, -1).permute(0, 3, 2, 1).reshape(-1, k * k * C)          # [M][tap][c]
    Wm = w.permute(2, 3, 1, 0).reshape(k * k * C, N)
    acc = torch.zeros(A.shape[0], N)
    for k0 in range(0, A.shape[1], chunk):
        acc = acc + A[:, k0:k0 + chunk] @ Wm[k0:k0 + chunk]
    OH, OW = rr["y"].shape[2:]
    y = acc.view(B, OH, OW, N).permute(0, 3, 1, 2)
    D = dy.permute(0, 2, 3, 1).reshape(-1, N)
    dw = torch.zeros(N, A.shape[1])
    for m0 in range(0, A.shape[0], chunk):
        dw = dw + D[m0:m0 + chunk].t() @ A[m0:m0 + chunk]
    return y, dw.view(N, k, k, C).permute(0, 3, 1, 2)


def row_id(row):
    op, cfg, dt, epi, name = row
    return f"{op}-cfg{cfg}-{str(dt)[6:]}-epi{epi}-{name}"
