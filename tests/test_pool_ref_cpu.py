"""CPU: the references and the case table of tests/_pool_ref.py.  The sortable-integer key of the 16-bit pools over every bit
pattern; the pool / upsample references against ATen and autograd; the table reaches every record value that
tests/test_elementwise_kernels_gpu.py must observe and every row_walk situation that test sizes can reach."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _pool_ref as P

ALL = np.arange(65536)


# ------------------------------------------------------------------------------------------------ the key
@pytest.mark.parametrize("dtype", P.SIXTEEN, ids=["f16", "bf16"])
def test_key_transform_over_every_bit_pattern(dtype):
    wide = P.widen_bits(ALL, dtype)
    key = P.key_of(wide)
    nan = P.is_nan_bits(ALL, dtype)
    assert not (wide & 0x1fff).any(), "a widened 16-bit value has 13 zero low bits"
    assert not (key & 31).any(), "the low five bits of every key are free"
    assert key.min() >= -(1 << 31) and (key + 25).max() < (1 << 31), "key + 25 stays a 32-bit integer"
    for low in range(26):
        assert np.array_equal(P.value_of(key + low), wide), f"value_of(key_of(b) + {low}) != b"
    # strictly monotonic on the non-NaN values in float order with -0 < +0, by more than the 25 of the position bits
    vals = P.from_bits(ALL[~nan], dtype).double().numpy()
    neg_zero = ALL[~nan] == 0x8000
    order = np.lexsort((~neg_zero, vals))                    # by value, -0 before +0
    k = key[~nan][order]
    assert (np.diff(k) >= 32).all()
    assert vals[order][0] == -np.inf and vals[order][-1] == np.inf
    inf_key = key[0x7c00 if dtype == P.F16 else 0x7f80]
    assert inf_key == k[-1] and inf_key + 25 < (1 << 31)
    assert key[0x8000] + 25 < key[0x0000], "-0 at the earliest position still loses against +0 at the last"
    # the key order is IEEE totalOrder of the 16-bit patterns, NaNs included: the rule the reference uses
    assert np.array_equal(np.argsort(key, kind="stable"), np.argsort(P.total_order(ALL), kind="stable"))
    sign = ALL >= 0x8000
    assert (key[nan & ~sign] > inf_key + 25).all(), "a NaN with a clear sign bit outranks +inf at any position"
    assert (key[nan & sign] + 25 < key[0xfc00 if dtype == P.F16 else 0xff80]).all(), "a NaN with the sign bit set is below -inf"
    assert (key[nan & sign] > -(1 << 31)).all(), "... but above the empty key, so a window of nothing else returns it"


# ------------------------------------------------------------------------------------------------ pool references
def _aten(x_nhwc):
    y, i = F.max_pool2d(x_nhwc.permute(0, 3, 1, 2).contiguous(), 5, 1, 2, return_indices=True)
    return y.permute(0, 2, 3, 1), i.permute(0, 2, 3, 1)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


@pytest.mark.parametrize("shape", [(1, 1, 1, 4), (2, 2, 9, 8), (2, 7, 3, 8), (1, 6, 5, 12), (2, 5, 23, 8), (1, 11, 4, 5)], ids=str)
def test_equal_rule_is_aten_bit_for_bit(shape):
    for x in (P.plateau_input(*shape, P.F32, 3), P.nan_input(*shape, P.F32, 4)):
        y, pos = P.pool_fwd_ref(x, "equal")
        ya, ia = _aten(x)
        assert torch.equal(P.aten_index(pos), ia)
        nan = torch.isnan(ya)
        assert torch.equal(torch.isnan(y), nan) and torch.equal(_bits(y)[~nan], _bits(ya)[~nan])
        assert torch.equal(_bits(y), _bits(ya)), "NaN payload and sign come from the pixel the index names"
    # NaNs of both signs propagate, and the last one in the window names the position
    x = torch.zeros(1, 5, 5, 1)
    pos_nan, neg_nan = (P.from_bits(b, P.F32) for b in P.nan_patterns(P.F32))
    x[0, 0, 0, 0], x[0, 2, 2, 0], x[0, 4, 4, 0] = pos_nan[0], neg_nan[1], pos_nan[2]
    y, pos = P.pool_fwd_ref(x, "equal")
    assert bool(torch.isnan(y).all()) and int(pos[0, 2, 2, 0]) == 24 and int(pos[0, 0, 0, 0]) == 24 and int(pos[0, 0, 4, 0]) == 20
    assert int(_bits(y)[0, 2, 2, 0]) == int(_bits(pos_nan[2:3])[0])


@pytest.mark.parametrize("dtype", P.SIXTEEN, ids=["f16", "bf16"])
def test_plus_first_rule(dtype):
    """Away from zeros of mixed sign and NaNs it is ATen's rule; at them it is what the kernel comment states."""
    x = P.plateau_input(2, 7, 9, 8, dtype, 6)
    y, pos = P.pool_fwd_ref(x, "plus_first")
    ya, ia = _aten(x.float())
    assert torch.equal(y.float(), ya)                                        # == : a zero of either sign is a zero
    assert torch.equal(P.aten_index(pos)[ya != 0], ia[ya != 0])
    ye, pe = P.pool_fwd_ref(x.float(), "equal")
    assert not torch.equal(pos, pe), "the plateau data must contain a window where +0 and -0 decide the position"
    x = torch.full((1, 5, 5, 1), -0.0, dtype=dtype)
    x[0, 4, 4, 0] = 0.0
    y, pos = P.pool_fwd_ref(x, "plus_first")
    assert int(pos[0, 2, 2, 0]) == 24 and int(_bits(y)[0, 2, 2, 0]) == 0 and int(pos[0, 0, 0, 0]) == 12 and int(_bits(y)[0, 0, 0, 0]) != 0
    # NaNs: clear sign bit propagates, larger payload first, then earlier position; sign bit set loses against everything
    pb, nb = P.nan_patterns(dtype)
    pn, nn = P.from_bits(pb, dtype), P.from_bits(nb, dtype)
    x = torch.full((1, 5, 5, 1), float("inf"), dtype=dtype)
    x[0, 0, 0, 0], x[0, 2, 2, 0], x[0, 4, 4, 0] = pn[0], pn[2], pn[2]
    y, pos = P.pool_fwd_ref(x, "plus_first")
    assert int(pos[0, 2, 2, 0]) == 12 and int(_bits(y)[0, 2, 2, 0]) & 0xffff == pb[2] and int(pos[0, 0, 0, 0]) == 24
    x = torch.full((1, 5, 5, 1), float("-inf"), dtype=dtype)
    x[0, 0, 0, 0], x[0, 2, 2, 0], x[0, 4, 4, 0] = nn[0], nn[2], nn[1]
    y, pos = P.pool_fwd_ref(x, "plus_first")
    assert not bool(torch.isnan(y).any()) and int(pos[0, 2, 2, 0]) == 1 and int(pos[0, 0, 0, 0]) == 13
    x = P.from_bits([nb[1]] * 25, dtype).view(1, 5, 5, 1).clone()
    x[0, 4, 4, 0] = nn[0]                                                    # smaller payload = larger in totalOrder
    y, pos = P.pool_fwd_ref(x, "plus_first")
    assert bool(torch.isnan(y).all()) and int(pos[0, 2, 2, 0]) == 24 and int(pos[0, 0, 0, 0]) == 12
    # the reference's maximum is the maximum of the kernel's keys
    x = P.nan_input(2, 6, 7, 6, dtype, 9)
    y, pos = P.pool_fwd_ref(x, "plus_first")
    key = torch.from_numpy(P.key_of(P.widen_bits(P._bits16(x).numpy(), dtype))).view(x.shape)
    best = torch.full(x.shape, -(1 << 31), dtype=torch.int64)
    for p in range(25):
        v, legal = P._shifted(key, p // 5, p % 5, 0)
        best = torch.maximum(best, torch.where(legal, v + 25 - p, best))
    assert torch.equal(25 - (best & 31), pos.long())
    assert np.array_equal(P.value_of(best.numpy()), P.widen_bits(P._bits16(y).numpy(), dtype).reshape(x.shape))


def test_all_patterns_input_and_builders():
    for dtype in P.SIXTEEN:
        x = P.all_patterns_input(dtype)
        bits = P._bits16(x).flatten().numpy()
        assert x.shape == (1, 64, 128, 8) and not bool(torch.isnan(x).any())
        assert set(bits.tolist()) == set(ALL[~P.is_nan_bits(ALL, dtype)].tolist())
    for dtype in P.DTYPES:
        x = P.plateau_input(2, 7, 9, 8, dtype, 1)
        raw = _bits(x)
        assert bool(((x == 0) & (raw != 0)).any()) and bool(((x == 0) & (raw == 0)).any()), "zeros of both signs"
        assert bool((x[..., 1] < 0).all()) and bool((x[..., 2] == float("-inf")).all()) and bool((x[..., 3] == float("inf")).any())
        n = P.nan_input(2, 6, 7, 6, dtype, 2)
        neg = _bits(n) < 0
        assert bool((torch.isnan(n) & neg).any()) and bool((torch.isnan(n) & ~neg).any())
        assert not bool((torch.isnan(n[..., 0]) & neg[..., 0]).any()) and bool((neg[..., 1] | ~torch.isnan(n[..., 1])).all())
    pos = P.random_legal_positions(2, 5, 23, 4, 3)
    P.take_positions(torch.zeros(2, 5, 23, 4), pos)                          # asserts legality
    assert set(pos[:, 2, 2:21].flatten().tolist()) == set(range(25)) and set(pos[:, 0, 0].flatten().tolist()) <= {12, 13, 14, 17, 18, 19, 22, 23, 24}
    x = P.peak_input(2, 5, 23, 4, P.F16)
    _, pk = P.pool_fwd_ref(x, "plus_first")
    count = torch.zeros(2, 5 * 23, 4).scatter_add_(1, P.aten_index(pk).reshape(2, -1, 4), torch.ones(2, 5 * 23, 4))
    assert int(count.max()) == 25, "the peak collects a term from each of the 25 windows around it"


@pytest.mark.parametrize("shape", [(2, 2, 9, 4), (2, 7, 3, 5), (1, 6, 5, 8), (2, 5, 23, 3)], ids=str)
def test_pool_bwd_ref_is_autograd(shape):
    x = P.reals(shape, P.F32, 1).double().requires_grad_(True)
    dy = P.reals(shape, P.F32, 2)
    _, pos = P.pool_fwd_ref(x.detach().float(), "equal")
    ya, _ = _aten(x)
    ya.backward(dy.double())
    old = P.reals(shape, P.F32, 3)
    assert torch.equal(P.pool_bwd_ref(dy, pos), x.grad)
    r64, r32 = P.pool_bwd_ref(dy, pos, old), P.pool_bwd_ref32(dy, pos, old)
    assert (r64 - (x.grad + old.double())).abs().max() < 1e-15 and r32.dtype == torch.float32
    assert (r32.double() - r64).abs().max() < 26 * 2.0 ** -24 * 26
    # integers: the scatter and the ordered gather are the same numbers, for any legal positions
    pos = P.random_legal_positions(*shape, 4)
    di, oi = P.ints(shape, -4, 4, P.BF16, 5), P.ints(shape, -4, 4, P.BF16, 6)
    r64 = P.pool_bwd_ref(di, pos, oi)
    assert torch.equal(P.pool_bwd_ref32(di, pos, oi).double(), r64) and r64.abs().max() <= 104
    assert torch.equal(r64.to(P.BF16).double(), r64), "|sum| <= 104 is exact in bf16"
    with pytest.raises(AssertionError):
        P.pool_bwd_ref(di, torch.zeros(shape, dtype=torch.uint8), oi)        # position 0 of pixel (0, 0) lies outside


def test_upsample_refs_are_interpolate_and_its_autograd():
    x = P.reals((2, 3, 5, 6), P.F32, 1).double().requires_grad_(True)
    up = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2.0, mode="nearest").permute(0, 2, 3, 1)
    assert torch.equal(P.upsample_fwd_ref(x.detach()), up)
    dy = P.reals((2, 6, 10, 6), P.F32, 2)
    up.backward(dy.double())
    r64, r32 = P.upsample_bwd_ref(dy)
    assert (r64 - x.grad).abs().max() < 1e-15 and (r32.double() - r64).abs().max() < 4 * 2.0 ** -24 * 4
    di, oi = P.ints((2, 6, 10, 6), -16, 16, P.BF16, 3), P.ints((2, 3, 5, 6), -16, 16, P.BF16, 4)
    r64, r32 = P.upsample_bwd_ref(di, oi)
    assert torch.equal(r32.double(), r64) and r64.abs().max() <= 80 and torch.equal(r64.to(P.BF16).double(), r64)


# ------------------------------------------------------------------------------------------------ dispatch mirror and the table
def test_mirror_on_the_shapes_the_model_uses():
    # SPPF of yolo11n at 640: 20 x 20 x 128 slices of a 512-channel buffer, f16
    assert P.pool_branch(P.F16, 128, (512, 512), (0, 256), 1) == P.POOL_WALK
    assert P.pool_branch(P.F16, 128, (512, 512), (0, 256), 0) == P.POOL_VEC
    assert P.pool_branch(P.F32, 128, (512, 512), (0, 512), 1) == P.POOL_VEC
    assert P.pool_branch(P.F16, 128, (512, 512), (0, 2), 1) == P.POOL_SCALAR
    assert P.vec_width(P.F16, 12, (12, 12), (0, 0)) == 1 and P.vec_width(P.F32, 12, (12, 12), (0, 0)) == 4
    assert P.vec_width(P.BF16, 64, (64, 72), (0, 16)) == 8 and P.vec_width(P.BF16, 64, (64, 73), (0, 0)) == 1
    assert P.row_geom(40, 8) == {"cpv": 5, "rows_pb": 51, "cblocks": 1} and 256 % 5
    assert P.row_geom(301, 1) == {"cpv": 301, "rows_pb": 1, "cblocks": 2}
    assert P.row_geom(2056, 8)["cblocks"] == 2 and P.row_geom(1028, 4)["cblocks"] == 2
    for kind in ("dense", "slice", "off1", "oddld"):
        for dt in P.DTYPES:
            for C in (8, 40, 64, 3, 12, 301):
                ld, off = P.layout(dt, C, kind)
                vec = 16 // P.ESZ[dt]
                assert ld >= off + C
                assert (P.vec_width(dt, C, (ld,), (off * P.ESZ[dt],)) > 1) == (kind in ("dense", "slice") and C % vec == 0)


def test_table_reaches_every_record_value():
    ids = [P.row_id(r) for r in P.ROWS]
    assert len(ids) == len(set(ids))
    want = set()
    for dt in P.DTYPES:
        wide = 4 if dt == P.F32 else 8
        want |= {("ew_vec_last", 1, dt), ("ew_vec_last", wide, dt)}
        for rec in ("pool_fwd_last", "pool_bwd_last"):
            want |= {(rec, c, dt) for c in ((1, 2) if dt == P.F32 else (1, 2, 3))}
    got = P.promised()
    assert got == want, (sorted(map(str, want - got)), sorted(map(str, got - want)))


def test_table_reaches_the_layouts_channels_and_maps():
    for dt in P.DTYPES:
        rows = [r for r in P.ROWS if r[0] == dt]
        for C in (8, 40, 64, 3, 12):
            assert {(r[5], r[6]) for r in rows if r[4] == C} >= set(P.PAIRS)
        for m in P.MAPS:
            assert {P.row_vec(r) > 1 for r in rows if r[1:4] == m} == {True, False}
        assert any(r[1:5] == (3, 20, 20, 64) for r in rows)
        wide = [r for r in rows if r[4] > 256]
        assert {(P.row_vec(r) > 1, P.row_geom(r[4], P.row_vec(r))["cblocks"]) for r in wide} == {(True, 2), (False, 2)}
        assert all(r[2] * r[3] <= 9 for r in wide)
        # 12 channels: scalar in 16 bit, vector in f32; 40 channels: five vectors, which does not divide 256
        assert {P.row_vec(r) for r in rows if r[4] == 12 and r[5:] == ("dense", "dense")} == ({4} if dt == P.F32 else {1})
    # a one-row last band, H below the band height, and more than one band, on the column-walk kernels
    walk = [r for r in P.ROWS if (1, P.POOL_WALK) in P.row_forms(r)]
    assert {r[2] for r in walk} >= {1, 2, 4, 5, 6, 7, 11, 20}
    big = [r for r in P.ROWS if r[1] * r[2] * r[3] > 1200]
    assert big == [P.CAP_ROW], "nothing is larger than the grid-cap row"
    for r in P.SPPF_ROWS:
        assert P.sppf_forms(r)[0][0] == 1
    assert {P.sppf_forms(r)[0][1] for r in P.SPPF_ROWS} == {1, 2, 3}


def test_table_reaches_the_row_walk_situations():
    """copy2d: a single partial unit, an exact unit, unit + 1, the two-trip branch (2048 < blocks < 6144) and the 2048-block cap of
    the strided map; every walk visits every row exactly once.  `blocks > max_blocks` (2^20 blocks of at least 4 rows) is out of
    reach at test sizes.  The grid-cap row also passes the 2048-block cap of row_grid, the grid of the upsample and 25-way pool
    kernels."""
    seen = set()
    for r in P.ROWS:
        M, vec = r[1] * r[2] * r[3], P.row_vec(r)
        g = P.row_geom(r[4], vec)
        for row_map in (1, 0):
            w = P.copy_walk(r[0], r[4], M, vec, row_map)
            seen |= P.walk_situation(w, M)
            if r != P.CAP_ROW or row_map == 0:
                assert P.walk_rows(w, M, g["rows_pb"], 4) == list(range(M)), (P.row_id(r), row_map)
    assert seen == {"partial", "exact", "unit+1", "t2", "cap2048"}
    r = P.CAP_ROW
    M, vec = r[1] * r[2] * r[3], P.row_vec(r)
    g = P.row_geom(r[4], vec)
    assert vec == 1 and g == {"cpv": 256, "rows_pb": 1, "cblocks": 1} and M == 8281 > 8192
    assert P.row_grid(M, g["rows_pb"]) == (2048, True)
    w = P.copy_walk(r[0], r[4], M, vec, 1)
    assert w["t"] == 2 and w["chunk"] == 8 and w["grid"] == 1036 and P.walk_rows(w, M, 1, 4) == list(range(M))
    assert P.copy_walk(r[0], r[4], M, vec, 0)["grid"] == 2048
    assert all(P.row_grid(x[1] * x[2] * x[3], P.row_geom(x[4], P.row_vec(x))["rows_pb"])[1] is False for x in P.ROWS if x != r)
    # the branches themselves
    assert P.row_walk(1 << 30, 1, 4, 1, 1 << 20, 1)["over_max"] and P.row_walk(1 << 30, 1, 4, 1, 1 << 20, 1)["grid"] <= 1 << 20
    assert P.row_walk(4 * 6144, 1, 4, 1, 1 << 20, 1)["t"] == 1 and P.row_walk(4 * 6143, 1, 4, 1, 1 << 20, 1)["t"] == 3
    assert P.row_walk(4 * 2048, 1, 4, 1, 1 << 20, 1)["t"] == 1 and P.row_walk(4 * 2049, 1, 4, 1, 1 << 20, 1)["t"] == 2


# ------------------------------------------------------------------------------------------------ cast inputs
@pytest.mark.parametrize("dst", P.SIXTEEN, ids=["f16", "bf16"])
def test_cast_pool_holds_the_rounding_cases(dst):
    pool = P.cast_pool(P.F32, dst)
    out = pool.to(dst)
    assert bool(torch.isnan(pool).any()) and bool(torch.isinf(pool).any()) and bool((pool == 0).any())
    finite = torch.isfinite(pool)
    assert bool((finite & torch.isinf(out)).any()), "values at and past the overflow threshold"
    big = torch.finfo(dst).max
    assert bool((finite & (pool > big) & (out == big)).any()), "... and just below it"
    assert bool(((pool != 0) & (out == 0)).any()) and bool(((pool.abs() < torch.finfo(dst).tiny) & (out != 0)).any())
    back = out.float()
    ties = finite & torch.isfinite(back) & (back != pool)
    assert int(ties.sum()) > 60000
    raw = P._bits16(out)
    nxt = P.from_bits(((raw + 1) & 0xffff).numpy(), dst).double()
    prv = P.from_bits(((raw - 1) & 0xffff).numpy(), dst).double()
    exact_tie = ties & ((pool.double() == (back.double() + nxt) / 2) | (pool.double() == (back.double() + prv) / 2))
    assert int(exact_tie.sum()) > 20000 and bool((raw[exact_tie] & 1 == 0).all()), "exact midpoints, rounded to even"
    for src in P.SIXTEEN:
        assert sorted(P._bits16(P.cast_pool(src, dst)).tolist()) == list(range(65536))
    assert P.cast_input(P.F32, dst, 4096 * 256 + 3).numel() == 4096 * 256 + 3 > pool.numel() and P.cast_input(dst, P.F32, 1).numel() == 1
