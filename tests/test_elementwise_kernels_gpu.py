"""The NHWC data-movement kernels of csrc/elementwise.hip (copy2d_kernel, upsample2x_fwd_kernel, upsample2x_bwd_kernel,
maxpool5_fwd_kernel, maxpool5_fwd_sep_kernel, maxpool5_bwd_kernel, maxpool5_bwd_walk_kernel, cast_kernel) against the references of
tests/_pool_ref.py, with proof of which one ran: after every call "ew_vec_last" / "pool_fwd_last" / "pool_bwd_last" must equal the
restated dispatch (`vec_width`, `pool_branch`) BEFORE anything is compared, and the last test requires the (record, code, dtype)
combinations observed in the session to be exactly those that tests/test_pool_ref_cpu.py promises.

Every row of the table names a layout per tensor argument: dense, a 16-byte aligned slice of a wider sentinel buffer, a slice one
element in, a pixel stride that is no multiple of the vector; the channels next to every slice must still hold the sentinel and
every input must keep its bits.
  copy2d            plain copy bit-equal; accumulate bit-equal to (src.float() + dst.float()).to(dtype); both "row_map" values.
  upsample2x fwd    bit-equal to index replication.
  upsample2x bwd    integers: bit-equal to float64, plain and accumulating; reals: 8 e_ref + u s with the f32 reference in the
                    kernel's order.
  maxpool5 fwd      every form the dtype has ("maxpool_sep" 1 / 0): values bit-equal, window positions equal everywhere (no mask)
                    to the dtype's rule, on plateaus with zeros of both signs, negative, -inf and +inf channels, NaNs of both
                    signs, and every non-NaN 16-bit pattern; idx = None; the forms agree bit for bit; the SPPF chain inside one buffer.
  maxpool5 bwd      both forms; positions from the reference, uniformly random legal positions, and a peak that collects 25 terms;
                    integers bit-equal to float64, reals under the bar, walk == 25-way bit for bit.
  cast              nine dtype pairs x five lengths, bit-equal to torch's CPU conversion (NaN: any NaN).

MI355X when the tests were written: 1222 cases in 5.8 s, the slowest 0.2 s (the 1 x 91 x 91 x 256 grid-cap row).  Worst err / bar of
the real family: upsample2x_bwd f16 0.998, bf16 0.970, f32 0.116; maxpool5_bwd f16 0.908, bf16 0.966, f32 0.122.  The 16-bit figures
are the rounding of the stored sum (the u s term is half an ulp at the largest value); in f32 the kernels reproduce the ordered f32
reference (err / e_ref = 1.00).  Nothing is tuned to these figures.
"""
import pytest
import torch
import torch.nn.functional as F

from tests import _kernel_ref as K
from tests import _pool_ref as P
from tests.test_conv_variants_gpu import DEV, SENTINEL, View, lib, ops, options, same

pytestmark = pytest.mark.gpu

OBSERVED = set()         # (record, code, dtype) of every checked call of this session
per_row = pytest.mark.parametrize("row", P.ROWS, ids=P.row_id)


class Slice(View):
    """`View` laid out by a table layout name and filled bit for bit from an NHWC CPU tensor of the kernel's dtype."""

    def __init__(self, B, H, W, C, dtype, kind, src=None):
        ld, off = P.layout(dtype, C, kind)
        super().__init__(B, H, W, C, dtype, ld, off)
        assert self.buf.data_ptr() % 16 == 0 and ops().view_ld(self.v) == ld
        self.ld, self.dtype, self.src = ld, dtype, None
        if src is not None:
            self.put(src)
            self.src = src

    def put(self, src):
        assert src.dtype == self.dtype and tuple(src.shape) == tuple(self.v.shape)
        self.v.copy_(src.to(DEV))

    def get(self):
        return self.v.cpu().contiguous()

    def wipe(self):
        self.buf.fill_(SENTINEL)

    def assert_unchanged(self, what):
        assert_bits(self.get(), self.src, f"{what}: the input changed")
        self.assert_neighbours_untouched(what)


def assert_bits(got, ref, what):
    got, ref = got.cpu(), ref.cpu()
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, tuple(got.shape), tuple(ref.shape))
    if K.same_bits(got.float(), ref.float()):
        return
    raw = torch.int32 if got.element_size() == 4 else torch.int16
    bad = got.contiguous().view(raw) != ref.contiguous().view(raw)
    i = tuple(bad.nonzero()[0].tolist())
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ in bits, first at {i}: got {got[i].item()!r} "
                         f"({int(got.contiguous().view(raw)[i]) & 0xffffffff:#x}) want {ref[i].item()!r} ({int(ref.contiguous().view(raw)[i]) & 0xffffffff:#x})")


def assert_positions(got, ref, what):
    got, ref = got.cpu(), ref.cpu()
    bad = got != ref
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} window positions differ, first at {i}: got {int(got[i])} want {int(ref[i])}")


def note(record, dtype, want, table):
    """The library's record of the launch just made == the mirror on the real addresses == what the table promised."""
    got = lib().get_option(record)
    assert got == want == table, f"{record} = {got}, the mirror on these addresses names {want}, the table promises {table}"
    OBSERVED.add((record, got, dtype))


def pair(row, shape_a, shape_b, src_a=None, src_b=None):
    dt, _, _, _, C, ka, kb = row
    a, b = Slice(*shape_a, C, dt, ka, src_a), Slice(*shape_b, C, dt, kb, src_b)
    ptrs = (a.v.data_ptr(), b.v.data_ptr())
    return a, b, ((a.ld, b.ld), ptrs)


# ------------------------------------------------------------------------------------------------ copy2d
@per_row
def test_copy2d(row):
    dt, B, H, W, C = row[:5]
    src, old = P.reals((B, H, W, C), dt, P.row_seed(row, 1), 4.0), P.reals((B, H, W, C), dt, P.row_seed(row, 2), 4.0)
    expect = (src.float() + old.float()).to(dt)
    for row_map in (1, 0):
        what = f"copy2d {P.row_id(row)} row_map {row_map}"
        with options(row_map=row_map):
            a, b, (lds, ptrs) = pair(row, (B, H, W), (B, H, W), src)
            ops().copy2d(a.v, b.v)
            note("ew_vec_last", dt, P.vec_width(dt, C, lds, ptrs), P.row_vec(row))
            assert_bits(b.get(), src, what)
            b.assert_neighbours_untouched(what)
            b.put(old)
            ops().copy2d(a.v, b.v, accumulate=True)
            note("ew_vec_last", dt, P.vec_width(dt, C, lds, ptrs), P.row_vec(row))
            assert_bits(b.get(), expect, what + " accumulate")
            b.assert_neighbours_untouched(what + " accumulate")
            a.assert_unchanged(what)


# ------------------------------------------------------------------------------------------------ upsample
@per_row
def test_upsample2x_fwd(row):
    dt, B, H, W, C = row[:5]
    what = f"upsample2x_fwd {P.row_id(row)}"
    x = P.reals((B, H, W, C), dt, P.row_seed(row, 3), 4.0)
    a, b, (lds, ptrs) = pair(row, (B, H, W), (B, 2 * H, 2 * W), x)
    ops().upsample2x_fwd(a.v, b.v)
    note("ew_vec_last", dt, P.vec_width(dt, C, lds, ptrs), P.row_vec(row))
    assert_bits(b.get(), P.upsample_fwd_ref(x), what)
    b.assert_neighbours_untouched(what)
    a.assert_unchanged(what)


@per_row
def test_upsample2x_bwd(row):
    dt, B, H, W, C = row[:5]
    what = f"upsample2x_bwd {P.row_id(row)}"
    big, small = (B, 2 * H, 2 * W, C), (B, H, W, C)
    bars = K.Bars(what)
    for family in ("exact", "real"):
        if family == "exact":
            dy, old = P.ints(big, -16, 16, dt, P.row_seed(row, 4)), P.ints(small, -16, 16, dt, P.row_seed(row, 5))
        else:
            dy, old = P.reals(big, dt, P.row_seed(row, 6), 2.0), P.reals(small, dt, P.row_seed(row, 7), 2.0)
        a, b, (lds, ptrs) = pair(row, big[:3], small[:3], dy)
        for acc in (False, True):
            r64, r32 = P.upsample_bwd_ref(dy, old if acc else None)
            b.wipe()
            if acc:
                b.put(old)
            ops().upsample2x_bwd(a.v, b.v, accumulate=acc)
            note("ew_vec_last", dt, P.vec_width(dt, C, lds, ptrs), P.row_vec(row))
            name = f"{family}{' accumulate' if acc else ''}"
            if family == "exact":
                same(b.get(), r64, f"{what} {name}")
            else:
                bars.add(name, b.get(), r64, r32, out_dtype=dt)
            b.assert_neighbours_untouched(f"{what} {name}")
        a.assert_unchanged(what)
    bars.check()


# ------------------------------------------------------------------------------------------------ max-pool forward
def window_any(mask):
    """(B, H, W, C) bool: does the 5 x 5 window around each pixel hold a True inside the map?"""
    return (F.max_pool2d(mask.float().permute(0, 3, 1, 2), 5, 1, 2) > 0).permute(0, 2, 3, 1)


def assert_nan_rule(x, y, what):
    """The rule of the comment above maxpool5_fwd_kernel, stated on the output alone."""
    nan = torch.isnan(x)
    if x.dtype == P.F32:
        want = window_any(nan)
    else:
        neg = nan & (x.view(torch.int16) < 0)
        want = window_any(nan & ~neg) | ~window_any(~neg)          # a NaN with a clear sign bit, or nothing but NaNs with it set
    assert torch.equal(torch.isnan(y), want), f"{what}: NaN propagation differs from the stated rule"


def run_pool_fwd(what, dt, x, y, idx, forms, table_forms, lds_ptrs, ref=None):
    """Every form on one input: values and positions against the reference, idx = None, neighbours; returns the reference."""
    ref_y, ref_pos = ref if ref is not None else P.pool_fwd_ref(x.src, P.ZERO_RULE[dt])
    assert forms == table_forms, f"{what}: forms {forms} on these addresses, the table promises {table_forms}"
    for sep, code in forms:
        w = f"{what} maxpool_sep {sep} (kernel {code})"
        with options(maxpool_sep=sep):
            y.wipe()
            idx.fill_(99)
            ops().maxpool5_fwd(x.v, y.v, idx)
            note("pool_fwd_last", dt, P.pool_branch(dt, x.C, *lds_ptrs, sep), code)
            assert_positions(idx, ref_pos, w)
            assert_bits(y.get(), ref_y, w)
            y.assert_neighbours_untouched(w)
            y.wipe()
            ops().maxpool5_fwd(x.v, y.v, None)
            note("pool_fwd_last", dt, P.pool_branch(dt, x.C, *lds_ptrs, sep), code)
            assert_bits(y.get(), ref_y, w + " without idx")
            y.assert_neighbours_untouched(w + " without idx")
    x.assert_unchanged(what)
    return ref_y, ref_pos


def forms_on(dt, C, lds, ptrs):
    on, off = P.pool_branch(dt, C, lds, ptrs, 1), P.pool_branch(dt, C, lds, ptrs, 0)
    return [(1, on)] + ([(0, off)] if off != on else [])


@per_row
def test_maxpool5_fwd(row):
    """The forms are compared with one reference each, bit for bit in values and positions: they agree with each other."""
    dt, B, H, W, C = row[:5]
    inputs = [("plateaus", P.plateau_input(B, H, W, C, dt, P.row_seed(row, 8)))]
    if row != P.CAP_ROW:
        inputs.append(("NaNs", P.nan_input(B, H, W, C, dt, P.row_seed(row, 9))))
    for name, xs in inputs:
        what = f"maxpool5_fwd {P.row_id(row)} {name}"
        x, y, (lds, ptrs) = pair(row, (B, H, W), (B, H, W), xs)
        idx = torch.empty(B, H, W, C, dtype=torch.uint8, device=DEV)
        ref_y, _ = run_pool_fwd(what, dt, x, y, idx, forms_on(dt, C, lds, ptrs), P.row_forms(row), (lds, ptrs))
        if name == "NaNs":
            assert_nan_rule(xs, ref_y, what)


@pytest.mark.parametrize("dtype", P.SIXTEEN, ids=["f16", "bf16"])
@pytest.mark.parametrize("kinds", [("dense", "dense"), ("off1", "dense")], ids=["vector", "scalar"])
def test_maxpool5_fwd_every_16bit_pattern(dtype, kinds):
    """Every non-NaN bit pattern once, in a seeded permutation: the key must order all of them, subnormals and infinities included."""
    xs = P.all_patterns_input(dtype)
    row = (dtype, 1, 64, 128, 8) + kinds
    x, y, (lds, ptrs) = pair(row, (1, 64, 128), (1, 64, 128), xs)
    idx = torch.empty(1, 64, 128, 8, dtype=torch.uint8, device=DEV)
    forms = forms_on(dtype, 8, lds, ptrs)
    assert [c for _, c in forms] == ([P.POOL_WALK, P.POOL_VEC] if kinds[0] == "dense" else [P.POOL_SCALAR])
    run_pool_fwd(f"maxpool5_fwd every {P.NAME[dtype]} pattern {kinds[0]}", dtype, x, y, idx, forms, forms, (lds, ptrs))


@pytest.mark.parametrize("row", P.SPPF_ROWS, ids=P.row_id)
def test_maxpool5_fwd_sppf_chain(row):
    """SPPF: one B x H x W x 4C buffer, three chained pools from slice i into slice i + 1 (ld = 4C on both sides, the same
    allocation), with the argmax (training) and without (inference).  Each stage equals the reference of the stage before."""
    dt, B, H, W, C = row
    x0 = P.plateau_input(B, H, W, C, dt, P.row_seed(row, 10))
    refs, cur = [], x0
    for _ in range(3):
        refs.append(P.pool_fwd_ref(cur, P.ZERO_RULE[dt]))
        cur = refs[-1][0]
    for sep, code in P.sppf_forms(row):
        for with_idx in (True, False):
            what = f"SPPF {P.row_id(row)} maxpool_sep {sep} idx {with_idx}"
            buf = torch.full((B, H, W, 4 * C), SENTINEL, dtype=dt, device=DEV)
            buf[..., :C].copy_(x0.to(DEV))
            idx = [torch.full((B, H, W, C), 99, dtype=torch.uint8, device=DEV) for _ in range(3)]
            with options(maxpool_sep=sep):
                for i in range(3):
                    src, dst = buf[..., i * C:(i + 1) * C], buf[..., (i + 1) * C:(i + 2) * C]
                    assert ops().view_ld(src) == ops().view_ld(dst) == 4 * C
                    ops().maxpool5_fwd(src, dst, idx[i] if with_idx else None)
                    note("pool_fwd_last", dt, P.pool_branch(dt, C, (4 * C, 4 * C), (src.data_ptr(), dst.data_ptr()), sep), code)
                    assert (buf[..., (i + 2) * C:] == SENTINEL).all(), f"{what}: stage {i} wrote past its slice"
            out = buf.cpu()
            assert_bits(out[..., :C].contiguous(), x0, f"{what}: slice 0")
            for i in range(3):
                assert_bits(out[..., (i + 1) * C:(i + 2) * C].contiguous(), refs[i][0], f"{what}: stage {i}")
                if with_idx:
                    assert_positions(idx[i], refs[i][1], f"{what}: stage {i}")


# ------------------------------------------------------------------------------------------------ max-pool backward
@per_row
def test_maxpool5_bwd(row):
    dt, B, H, W, C = row[:5]
    shape = (B, H, W, C)
    light = row == P.CAP_ROW
    sources = [("random", P.random_legal_positions(B, H, W, C, P.row_seed(row, 11)))]
    if not light:
        sources.append(("reference", P.pool_fwd_ref(P.plateau_input(B, H, W, C, dt, P.row_seed(row, 8)), P.ZERO_RULE[dt])[1]))
        sources.append(("peak", P.pool_fwd_ref(P.peak_input(B, H, W, C, dt), P.ZERO_RULE[dt])[1]))
    bars = K.Bars(f"maxpool5_bwd {P.row_id(row)}")
    for sname, pos in sources:
        idx = pos.to(DEV)
        for family in ("exact", "real"):
            if family == "exact":
                dy, old = P.ints(shape, -4, 4, dt, P.row_seed(row, 12)), P.ints(shape, -4, 4, dt, P.row_seed(row, 13))
            else:
                dy, old = P.reals(shape, dt, P.row_seed(row, 14), 2.0), P.reals(shape, dt, P.row_seed(row, 15), 2.0)
            a, b, (lds, ptrs) = pair(row, shape[:3], shape[:3], dy)
            forms = forms_on(dt, C, lds, ptrs)
            assert forms == P.row_forms(row)
            for acc in ((False, True) if not (light and family == "real") else (False,)):
                name = f"{sname} positions, {family}{' accumulate' if acc else ''}"
                r64 = P.pool_bwd_ref(dy, pos, old if acc else None)
                r32 = P.pool_bwd_ref32(dy, pos, old if acc else None) if family == "real" else None
                first = None
                for sep, code in forms:
                    what = f"maxpool5_bwd {P.row_id(row)} {name} maxpool_sep {sep} (kernel {code})"
                    with options(maxpool_sep=sep):
                        b.wipe()
                        if acc:
                            b.put(old)
                        ops().maxpool5_bwd(a.v, idx, b.v, accumulate=acc)
                        note("pool_bwd_last", dt, P.pool_branch(dt, C, lds, ptrs, sep), code)
                    got = b.get()
                    if family == "exact":
                        same(got, r64, what)
                    else:
                        bars.add(f"{name} kernel {code}", got, r64, r32, out_dtype=dt)
                    b.assert_neighbours_untouched(what)
                    if first is None:
                        first = got
                    else:
                        assert_bits(got, first, what + ": the column walk and the 25-way kernel add in the same order")
            a.assert_unchanged(f"maxpool5_bwd {P.row_id(row)} {sname}")
        assert torch.equal(idx.cpu(), pos), "the positions changed"
    bars.check()


# ------------------------------------------------------------------------------------------------ cast
CAST_N = (1, 255, 256, 257, 4096 * 256 + 3)                   # the last one forces a second grid-stride trip


@pytest.mark.parametrize("n", CAST_N)
@pytest.mark.parametrize("dst", P.DTYPES, ids=lambda d: "to-" + P.NAME[d])
@pytest.mark.parametrize("src", P.DTYPES, ids=lambda d: P.NAME[d])
def test_cast(src, dst, n):
    o = ops()
    x = P.cast_input(src, dst, n)
    expect = x.to(dst)
    xd = x.to(DEV)
    out = torch.full((n + 64,), SENTINEL, dtype=dst, device=DEV)
    lib().call("sy11_cast", o.dt_code(src), o.dt_code(dst), n, o._p(xd), o._p(out), o._stream())
    got = out[:n].cpu()
    what = f"cast {P.NAME[src]} -> {P.NAME[dst]} n {n}"
    assert (out[n:] == SENTINEL).all(), f"{what}: wrote past the last element"
    assert_bits(xd.cpu(), x, f"{what}: the input changed")
    nan = torch.isnan(expect)
    assert torch.equal(torch.isnan(got), nan), f"{what}: NaNs differ"
    zero = torch.zeros((), dtype=dst)
    assert_bits(torch.where(nan, zero, got), torch.where(nan, zero, expect), what)


def test_every_promised_kernel_ran():
    """Needs the whole file: the (record, code, dtype) combinations that the tests above really launched, read back from the
    library, are exactly those that the CPU test of the table promises."""
    want = P.promised()
    assert OBSERVED == want, f"never ran: {sorted(map(str, want - OBSERVED))}; unexpected: {sorted(map(str, OBSERVED - want))}"
