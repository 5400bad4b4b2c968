"""CPU restatement of the NHWC data-movement kernels of csrc/elementwise.hip (copy2d, upsample2x forward / backward, the three
forward and two backward forms of the 5x5 stride-1 max-pool, cast): the host dispatch (`vec_width`, `pool_branch`, `row_geom`,
`row_walk`, `row_grid`), float64 / kernel-ordered f32 references, the sortable-integer key of the 16-bit pools, input builders, and
the case table shared by tests/test_pool_ref_cpu.py and tests/test_elementwise_kernels_gpu.py.  Not a test module.

The GPU file compares the library's "ew_vec_last" / "pool_fwd_last" / "pool_bwd_last" records with this mirror after every call, so
drift of either side fails; the CPU file proves that the table reaches every record value and every row-walk situation.

Pool rules (the comment above maxpool5_fwd_kernel):
  f32 ("equal"): ATen's loop.  Start at the first legal window position with -inf; a later position is taken when its value is
    greater or is a NaN, so +0 / -0 tie (the first stays), a NaN of either sign propagates and the LAST NaN names the position.
  16-bit ("plus_first"): the first maximum in IEEE totalOrder of the bit patterns: -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN,
    among +NaNs the larger payload is larger.  So +0 outranks -0 wherever it stands, a NaN with a clear sign bit propagates, and
    one with the sign bit set never wins against anything else.
"""
import zlib

import numpy as np
import torch

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DTYPES = (F16, BF16, F32)
SIXTEEN = (F16, BF16)
NAME = {F16: "f16", BF16: "bf16", F32: "f32"}
ESZ = {F16: 2, BF16: 2, F32: 4}
POOL_SCALAR, POOL_VEC, POOL_WALK = 1, 2, 3        # csrc/tune.h
ZERO_RULE = {F16: "plus_first", BF16: "plus_first", F32: "equal"}


def cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------------------ host dispatch
def vec_width(dtype, C, lds, ptrs):
    """`vec_ok`: 16 bytes of channels per thread when C, every pixel stride and every byte address allow it, else one element."""
    vec = 16 // ESZ[dtype]
    if C % vec or any(l % vec for l in lds) or any(p % 16 for p in ptrs):
        return 1
    return vec


def pool_branch(dtype, C, lds, ptrs, sep):
    """Which kernel sy11_maxpool5_fwd / sy11_maxpool5_bwd launch ("maxpool_sep" = `sep`)."""
    v = vec_width(dtype, C, lds, ptrs) > 1
    if sep and v and ESZ[dtype] == 2:
        return POOL_WALK
    return POOL_VEC if v else POOL_SCALAR


def row_geom(C, vec):
    cpv = C // vec
    cw = min(cpv, 256)
    return {"cpv": cpv, "rows_pb": 256 // cw, "cblocks": cdiv(cpv, 256)}


def row_walk(M, rows_pb, U, trips, max_blocks, row_map):
    """`row_walk`: grid and strides of a row-walking kernel; row = block * bs + trip * ts + u * us + rsub, below the block's end."""
    if row_map == 0:
        g = cdiv(M, rows_pb * U)
        cap = min(max_blocks, 2048)
        capped = g > cap
        g = max(1, min(g, cap))
        return {"grid": g, "bs": rows_pb, "us": g * rows_pb, "ts": g * rows_pb * U, "chunk": 0, "t": None, "capped": capped}
    unit = rows_pb * U
    units = cdiv(M, unit)
    t = max(trips, 1)
    blocks = cdiv(units, t)
    if blocks > max_blocks:
        t = cdiv(units, max_blocks)
    elif 2048 < blocks < 6144:
        t = cdiv(units, 2048)
    chunk = unit * t
    return {"grid": cdiv(M, chunk), "bs": chunk, "ts": unit, "us": rows_pb, "chunk": chunk, "t": t, "units": units, "unit": unit,
            "over_max": blocks > max_blocks}


def walk_rows(w, M, rows_pb, U):
    """Every (row) a grid of `w` stores, as a sorted list: what copy2d_kernel's loop visits with its `< mend` predicate."""
    out = []
    for b in range(w["grid"]):
        mend = M if w["chunk"] == 0 else min((b + 1) * w["chunk"], M)
        for rsub in range(rows_pb):
            m = b * w["bs"] + rsub
            while m < mend:
                out.extend(m + u * w["us"] for u in range(U) if m + u * w["us"] < mend)
                m += w["ts"]
    return sorted(out)


def row_grid(M, rows_pb):
    """Grid of the upsample and 25-way pool kernels: 4 rows per thread, at most 2048 blocks, then a grid-stride loop."""
    g = cdiv(M, rows_pb * 4)
    return max(1, min(g, 2048)), g > 2048


def copy_walk(dtype, C, M, vec, row_map):
    g = row_geom(C, vec)
    return row_walk(M, g["rows_pb"], 4, 1, 1 << 20, row_map)


def walk_situation(w, M):
    """Names of the row_walk situations a chunked walk is in."""
    s = set()
    if w["chunk"] == 0:
        if w["capped"]:
            s.add("cap2048")
        return s
    if w["units"] == 1 and M < w["unit"]:
        s.add("partial")
    if M == w["unit"]:
        s.add("exact")
    if M == w["unit"] + 1:
        s.add("unit+1")
    if w["t"] == 2:
        s.add("t2")
    if w["over_max"]:
        s.add("over_max")
    return s


# ------------------------------------------------------------------------------------------------ layouts and the case table
def layout(dtype, C, kind):
    """(pixel stride, channel offset) of a view inside its sentinel buffer."""
    vec = 16 // ESZ[dtype]
    if kind == "dense":
        return C, 0
    if kind == "slice":                 # 16-byte aligned, ld > C
        return C + 2 * vec, vec
    if kind == "off1":                  # one element in: misaligned address
        return C + 2 * vec, 1
    if kind == "oddld":                 # aligned address, pixel stride no multiple of the vector
        ld = C + 2 * vec + 1
        return (ld if ld % vec else ld + 1), 0
    if kind == "ld257":
        return 257, 0
    raise ValueError(kind)


MAPS = [(1, 1, 1), (2, 2, 9), (2, 7, 3), (1, 11, 4), (1, 4, 6), (1, 5, 5), (1, 6, 5), (2, 5, 23)]
PAIRS = [("dense", "dense"), ("slice", "slice"), ("slice", "dense"), ("dense", "slice"), ("off1", "dense"), ("dense", "off1"),
         ("oddld", "dense"), ("dense", "oddld")]
CAP_ROW = (F16, 1, 91, 91, 256, "ld257", "ld257")


def _rows():
    rows = []
    for dt in DTYPES:
        for C in (8, 40, 64, 3, 12):                       # every layout of each argument, at every channel count
            rows += [(dt, 2, 7, 3, C, a, b) for a, b in PAIRS]
        for B, H, W in MAPS:                               # every map, vector and scalar, dense and sliced
            for C in (8, 3):
                rows += [(dt, B, H, W, C, a, b) for a, b in PAIRS[:2]]
        rows += [(dt, 3, 20, 20, 64, a, b) for a, b in PAIRS[:2]]
        rows += [(dt, 1, 3, 3, 301, a, b) for a, b in PAIRS[:2]]                       # scalar, cblocks = 2
        wide = 1028 if dt == F32 else 2056                                              # vector, cblocks = 2
        rows += [(dt, 1, 2, 2, wide, a, b) for a, b in PAIRS[:2]] + [(dt, 1, 3, 3, wide, "dense", "dense")]
        rows += [(dt, 1, 4, 6, 40, "off1", "dense"), (dt, 1, 5, 5, 40, "off1", "dense")]   # scalar C = 40: one unit of 24 rows, and 25
    rows.append(CAP_ROW)
    seen, out = set(), []
    for r in rows:
        if r not in seen:
            seen.add(r)
            out.append(r)
    return out


ROWS = _rows()
# SPPF: three chained pools inside one B x H x W x 4C buffer, slice i -> slice i + 1, ld = 4C on both sides
SPPF_ROWS = [(dt, B, H, W, C) for dt in DTYPES for (B, H, W, C) in ((2, 5, 23, 8), (1, 6, 5, 3), (3, 20, 20, 64), (1, 6, 5, 40))]


def row_id(row):
    dt, B, H, W, C = row[:5]
    return f"{NAME[dt]}-{B}x{H}x{W}x{C}" + ("-" + "-".join(row[5:]) if len(row) > 5 else "")


def row_seed(row, salt=0):
    return zlib.crc32(f"{row_id(row)}/{salt}".encode()) & 0x7fffffff


def row_args(row):
    """(lds, byte offsets) of the two tensor arguments of a table row, relative to 16-byte aligned buffers."""
    dt, _, _, _, C, a, b = row
    (lda, offa), (ldb, offb) = layout(dt, C, a), layout(dt, C, b)
    return (lda, ldb), (offa * ESZ[dt], offb * ESZ[dt])


def row_vec(row):
    lds, ptrs = row_args(row)
    return vec_width(row[0], row[4], lds, ptrs)


def row_forms(row):
    """[(maxpool_sep, record code)] to run for a pool row: both switch values where they select different kernels."""
    lds, ptrs = row_args(row)
    on, off = pool_branch(row[0], row[4], lds, ptrs, 1), pool_branch(row[0], row[4], lds, ptrs, 0)
    return [(1, on)] + ([(0, off)] if off != on else [])


def sppf_forms(row):
    dt, _, _, _, C = row
    per_stage = [{pool_branch(dt, C, (4 * C, 4 * C), (i * C * ESZ[dt], (i + 1) * C * ESZ[dt]), s) for i in range(3)} for s in (1, 0)]
    assert all(len(p) == 1 for p in per_stage), "the three stages of one SPPF row run the same kernel"
    on, off = min(per_stage[0]), min(per_stage[1])
    return [(1, on)] + ([(0, off)] if off != on else [])


def promised():
    """Every (record, code, dtype) the GPU session must observe."""
    out = set()
    for r in ROWS:
        out.add(("ew_vec_last", row_vec(r), r[0]))
        for _, code in row_forms(r):
            out.add(("pool_fwd_last", code, r[0]))
            out.add(("pool_bwd_last", code, r[0]))
    for r in SPPF_ROWS:
        for _, code in sppf_forms(r):
            out.add(("pool_fwd_last", code, r[0]))
    return out


# ------------------------------------------------------------------------------------------------ sortable-integer key (16-bit pools)
def widen_bits(bits16, dtype):
    """The f32 bit patterns (int64 array) of 16-bit patterns `bits16` (any integer array, values 0..65535)."""
    b = np.asarray(bits16).astype(np.uint16)
    if dtype == BF16:
        return (b.astype(np.int64) << 16)
    return b.view(np.float16).astype(np.float32).view(np.uint32).astype(np.int64)


def _as_i32(u):
    """int64 array holding unsigned 32-bit patterns -> the same bits read as signed 32-bit, still in int64."""
    return np.where(u >= 1 << 31, u - (1 << 32), u)


def key_of(bits32):
    """`bits ^ ((bits >> 31) & 0x7fffffe0)` on f32 bit patterns (int64 array of unsigned patterns) -> signed keys in int64."""
    s = _as_i32(np.asarray(bits32, dtype=np.int64))
    return s ^ ((s >> 31) & 0x7fffffe0)


def value_of(key):
    """Inverse of key_of on a key with anything in its low five bits -> unsigned f32 bit pattern (int64)."""
    o = np.asarray(key, dtype=np.int64) & ~31
    v = o ^ ((o >> 31) & 0x7fffffe0)
    return v & 0xffffffff


def total_order(bits16):
    """IEEE totalOrder rank of 16-bit patterns as a signed integer (independent of key_of): -0 -> -1, +0 -> 0."""
    b = np.asarray(bits16).astype(np.int64) & 0xffff
    return np.where(b < 0x8000, b, 0x7fff - b)


def is_nan_bits(bits16, dtype):
    b = np.asarray(bits16).astype(np.int64) & 0x7fff
    return b > (0x7c00 if dtype == F16 else 0x7f80)


# ------------------------------------------------------------------------------------------------ pool references
def _bits16(x):
    return x.contiguous().view(torch.int16).to(torch.int64) & 0xffff


def _shifted(t, wy, wx, fill):
    """t[b, h + wy - 2, w + wx - 2, c] with `fill` outside the map, and the (H, W, 1) legality mask."""
    B, H, W, C = t.shape
    hh = torch.arange(H) + wy - 2
    ww = torch.arange(W) + wx - 2
    legal = ((hh >= 0) & (hh < H)).view(H, 1, 1) & ((ww >= 0) & (ww < W)).view(1, W, 1)
    g = t[:, hh.clamp(0, H - 1)][:, :, ww.clamp(0, W - 1)]
    return torch.where(legal, g, torch.full_like(g, fill)), legal


def pool_fwd_ref(x, zero_rule):
    """x: (B, H, W, C) in the kernel's dtype.  Returns (values in x's dtype with x's bits, window positions 0..24 as uint8) of the
    first maximum in row-major window order over the positions inside the map, under the rule of the module docstring."""
    B, H, W, C = x.shape
    if zero_rule == "plus_first":
        assert x.dtype in SIXTEEN
        bits = _bits16(x)
        rank = torch.where(bits < 0x8000, bits, 0x7fff - bits)
        best = torch.full(x.shape, -(1 << 40), dtype=torch.int64)
        pos = torch.full(x.shape, 255, dtype=torch.int64)
        for p in range(25):
            v, legal = _shifted(rank, p // 5, p % 5, 0)
            take = legal & (v > best)
            best, pos = torch.where(take, v, best), torch.where(take, torch.full_like(pos, p), pos)
    else:
        assert zero_rule == "equal"
        xd = x.double()
        best = torch.full(x.shape, float("-inf"), dtype=torch.float64)
        h0 = (2 - torch.arange(H)).clamp(min=0).view(1, H, 1, 1)
        w0 = (2 - torch.arange(W)).clamp(min=0).view(1, 1, W, 1)
        pos = (h0 * 5 + w0).expand(x.shape).clone()
        for p in range(25):
            v, legal = _shifted(xd, p // 5, p % 5, 0.0)
            take = legal & ((v > best) | torch.isnan(v))
            best, pos = torch.where(take, v, best), torch.where(take, torch.full_like(pos, p), pos)
    assert int(pos.max()) < 25
    return take_positions(x, pos), pos.to(torch.uint8)


def take_positions(x, pos):
    """x[b, h + pos // 5 - 2, w + pos % 5 - 2, c]: the stored bits of the pixel each window position names."""
    B, H, W, C = x.shape
    pos = pos.long()
    hh = torch.arange(H).view(1, H, 1, 1) + pos // 5 - 2
    ww = torch.arange(W).view(1, 1, W, 1) + pos % 5 - 2
    assert bool(((hh >= 0) & (hh < H) & (ww >= 0) & (ww < W)).all()), "a window position outside the map"
    flat = (hh * W + ww).reshape(B, H * W, C)
    raw = x.contiguous().view(torch.int16 if x.element_size() == 2 else torch.int32).reshape(B, H * W, C)
    return torch.gather(raw, 1, flat).reshape(B, H, W, C).view(x.dtype)


def aten_index(pos):
    """Window positions (B, H, W, C) -> ATen's flat h * W + w indices."""
    B, H, W, C = pos.shape
    pos = pos.long()
    return (torch.arange(H).view(1, H, 1, 1) + pos // 5 - 2) * W + torch.arange(W).view(1, 1, W, 1) + pos % 5 - 2


def pool_bwd_ref(dy, idx, old=None):
    """float64 scatter: dy[q] goes to the pixel that idx[q] names; + old."""
    B, H, W, C = dy.shape
    tgt = aten_index(idx)
    pos = idx.long()
    th, tw = torch.arange(H).view(1, H, 1, 1) + pos // 5 - 2, torch.arange(W).view(1, 1, W, 1) + pos % 5 - 2
    assert bool(((th >= 0) & (th < H) & (tw >= 0) & (tw < W)).all()), "idx names a pixel outside the map"
    dx = torch.zeros(B, H * W, C, dtype=torch.float64) if old is None else old.double().reshape(B, H * W, C).clone()
    dx.scatter_add_(1, tgt.reshape(B, H * W, C), dy.double().reshape(B, H * W, C))
    return dx.reshape(B, H, W, C)


def pool_bwd_ref32(dy, idx, old=None):
    """The same sum in f32 in the kernels' order: `old` first, then the 25 windows containing the pixel, window rows top to bottom,
    columns left to right; a window adds only where it selected this pixel."""
    B, H, W, C = dy.shape
    g32 = torch.nn.functional.pad(dy.float(), (0, 0, 2, 2, 2, 2))
    ip = torch.nn.functional.pad(idx.to(torch.int16), (0, 0, 2, 2, 2, 2), value=255)
    acc = torch.zeros(B, H, W, C, dtype=torch.float32) if old is None else old.float().clone()
    for oy in range(-2, 3):
        for ox in range(-2, 3):
            pos = (2 - oy) * 5 + (2 - ox)
            sel = ip[:, 2 + oy:2 + oy + H, 2 + ox:2 + ox + W] == pos
            acc = torch.where(sel, acc + g32[:, 2 + oy:2 + oy + H, 2 + ox:2 + ox + W], acc)
    return acc


def random_legal_positions(B, H, W, C, seed):
    """Uniform over the window positions whose source pixel lies inside the map, per element."""
    g = torch.Generator().manual_seed(seed)
    h, w = torch.arange(H).view(1, H, 1, 1), torch.arange(W).view(1, 1, W, 1)
    y0, x0 = (2 - h).clamp(min=0), (2 - w).clamp(min=0)                      # the legal window rows / columns are contiguous runs
    ny, nx = (H + 1 - h).clamp(max=4) - y0 + 1, (W + 1 - w).clamp(max=4) - x0 + 1
    k = (torch.rand(B, H, W, C, generator=g, dtype=torch.float64) * (ny * nx)).long().clamp(max=24)
    k = torch.minimum(k, (ny * nx - 1).expand_as(k))
    return ((y0 + k // nx) * 5 + x0 + k % nx).to(torch.uint8)


# ------------------------------------------------------------------------------------------------ upsample references
def upsample_fwd_ref(x):
    return x.repeat_interleave(2, 1).repeat_interleave(2, 2)


def upsample_bwd_ref(dy, old=None):
    """(float64, f32 in the kernel's order ((a + b) + c) + d, then + old) of the 2x2 sums."""
    q = [dy[:, i::2, j::2] for i in (0, 1) for j in (0, 1)]
    r64 = q[0].double() + q[1].double() + q[2].double() + q[3].double()
    r32 = ((q[0].float() + q[1].float()) + q[2].float()) + q[3].float()
    if old is not None:
        r64, r32 = r64 + old.double(), r32 + old.float()
    return r64, r32


# ------------------------------------------------------------------------------------------------ inputs
def from_bits(bits, dtype):
    """int array of bit patterns -> tensor of `dtype` with exactly those bits."""
    if dtype == F32:
        return torch.from_numpy(np.asarray(bits).astype(np.uint32).view(np.int32).copy()).view(F32)
    return torch.from_numpy(np.asarray(bits).astype(np.uint16).view(np.int16).copy()).view(dtype)


def ints(shape, lo, hi, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).to(dtype)


def reals(shape, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * scale).float().to(dtype)


def plateau_input(B, H, W, C, dtype, seed):
    """Ties everywhere, on a half-integer grid.  Channel c % 5: 0 values in [-2, 0] with zeros of both signs (the maximum of most
    windows is a zero), 1 all negative (a zero pad would win), 2 all -inf, 3 +inf plateaus among finite values, 4 values in [-2, 2]
    with zeros of both signs."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-4, 5, (B, H, W, C), generator=g).double() / 2
    c = torch.arange(C) % 5
    x = torch.where((c == 0).view(1, 1, 1, C), -x.abs(), x)
    neg = torch.rand(B, H, W, C, generator=g) < 0.5
    x = torch.where(x == 0, torch.where(neg, torch.full_like(x, -0.0), torch.zeros_like(x)), x)
    x = torch.where((c == 1).view(1, 1, 1, C), -x.abs() - 0.5, x)
    x = torch.where((c == 2).view(1, 1, 1, C), torch.full_like(x, float("-inf")), x)
    inf = torch.rand(B, H, W, C, generator=g) < 0.15
    x = torch.where((c == 3).view(1, 1, 1, C) & inf, torch.full_like(x, float("inf")), x)
    return x.to(dtype)


def nan_patterns(dtype):
    """Quiet NaNs of both signs with three payloads each, as bit patterns of `dtype`."""
    base, step = {F16: (0x7e00, 0x0040), BF16: (0x7fc0, 0x0008), F32: (0x7fc00000, 0x00040000)}[dtype]
    sign = 0x8000 if dtype != F32 else 0x80000000
    pos = [base, base + step, base + 3 * step]
    return pos, [p | sign for p in pos]


def nan_input(B, H, W, C, dtype, seed):
    """Finite plateaus with about one pixel in twelve a NaN: channel c % 3 == 0 NaNs with a clear sign bit only, 1 with the sign
    bit set only, 2 both.  On any map of 5 x 5 or more every NaN stands at each of the 25 positions of some window."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randint(-4, 5, (B, H, W, C), generator=g).double() / 2).to(dtype)
    raw = x.view(torch.int16 if dtype != F32 else torch.int32).clone()
    pos, neg = nan_patterns(dtype)
    hit = torch.rand(B, H, W, C, generator=g) < 1.0 / 12
    which = torch.randint(0, 3, (B, H, W, C), generator=g)
    minus = torch.rand(B, H, W, C, generator=g) < 0.5
    c = (torch.arange(C) % 3).view(1, 1, 1, C)
    minus = torch.where(c == 0, torch.zeros_like(minus), torch.where(c == 1, torch.ones_like(minus), minus))
    pt = from_bits(pos, dtype).view(raw.dtype)[which]
    nt = from_bits(neg, dtype).view(raw.dtype)[which]
    raw = torch.where(hit, torch.where(minus, nt, pt), raw)
    return raw.view(dtype)


def all_patterns_input(dtype, seed=5):
    """1 x 64 x 128 x 8: every non-NaN 16-bit pattern once, in a seeded permutation, the leftover filled with repeats."""
    bits = np.arange(65536)
    bits = bits[~is_nan_bits(bits, dtype)]
    rng = np.random.RandomState(seed)
    bits = rng.permutation(bits)
    bits = np.concatenate([bits, bits[:65536 - bits.size]])
    return from_bits(bits, dtype).view(1, 64, 128, 8)


def peak_input(B, H, W, C, dtype):
    """A constant map with one higher pixel per image and channel: every window that contains it selects it (25 terms on a map of
    5 x 5 or more), every other window its first legal position."""
    x = torch.zeros(B, H, W, C, dtype=dtype)
    x[:, H // 2, W // 2] = 1.0
    return x


# ------------------------------------------------------------------------------------------------ cast inputs
def cast_pool(src, dst, seed=11):
    """The inputs of one (src, dst) dtype pair as a 1-D tensor of `src`, in a seeded order.
    From 16 bit: every pattern.  f32 -> 16 bit: every pattern of the destination widened; every midpoint between adjacent
    destination values (subnormals, the step across each power of two, and the midpoint between the largest finite value and
    2^(emax + 1), the overflow threshold) with its two f32 neighbours, both signs; f32 subnormals; +-0, +-inf and NaNs ride along
    with the patterns.  f32 -> f32: the f16 pool."""
    rng = np.random.RandomState(seed)
    if src != F32:
        return from_bits(rng.permutation(65536), src)
    ref = dst if dst != F32 else F16
    pats = from_bits(np.arange(65536), ref).float()
    fin = from_bits(np.arange(0x7c00 if ref == F16 else 0x7f80), ref).double()             # +0 ... largest finite, ascending
    top = 2.0 ** (16 if ref == F16 else 128)
    grid = torch.cat([fin, torch.tensor([top], dtype=torch.float64)])
    mid64 = (grid[:-1] + grid[1:]) / 2
    mid = mid64.float()
    assert torch.equal(mid.double(), mid64), "a midpoint that f32 cannot hold"
    up, down = torch.nextafter(mid, torch.full_like(mid, float("inf"))), torch.nextafter(mid, torch.full_like(mid, float("-inf")))
    tiny = from_bits([1, 2, 0x007fffff, 0x00800000, 0x80000001, 0x807fffff], F32)
    allv = torch.cat([pats, mid, up, down, -mid, -up, -down, tiny])
    return allv[torch.from_numpy(rng.permutation(allv.numel()))]


def cast_input(src, dst, n):
    pool = cast_pool(src, dst)
    reps = cdiv(n, pool.numel())
    return pool.repeat(reps)[:n].clone()
