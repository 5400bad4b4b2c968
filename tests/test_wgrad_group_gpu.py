"""The grouped filter-gradient launch (sy11_conv2d_wgrad_group, csrc/wgrad.hip wgrad16g_kernel) against the float64 reference of
tests/_conv_ref.py, with proof that the grouped kernel is what ran ("wgrad_last_cfg" == 100 before anything is compared).

Exact family: integer operands, every dW BIT-EQUAL to float64 whatever order the atomics land in.  One group holds every index
path of the kernel (EXACT_GROUP below) and runs at three workgroup targets: one split per problem / three or more splits for some
problem / more workgroups than one resident round of the chip.  Every dW of a group lives in one pool whose gaps hold a sentinel:
an add that lands outside its own dW changes a gap.

Real family: uniform operands, the element-by-element bound of `_conv_ref.real_case`, and the grouped result's worst err / bound
against the per-layer kernel's on the same inputs (see `test_group_real`).
"""
import functools

import pytest
import torch

from tests import _conv_ref as R
from tests.test_conv_variants_gpu import DEV, SENTINEL, View, close_to_scale, lib, ops, options, same

pytestmark = pytest.mark.gpu

GROUP_CFG = 100
RESIDENT_ROUND = 512          # 256 CUs x 2 workgroups of the 128-wide tile (81 920 bytes of LDS each)

# (B, C, N, H, W, k, s, p, d), x_ld / x_off, dy_ld / dy_off (None: contiguous)
EXACT_GROUP = [
    ((2, 32, 40, 5, 7, 1, 1, 0, 1), None, None),            # M = 70: not a multiple of 64, partial n-tile
    ((2, 64, 136, 6, 6, 3, 1, 1, 1), None, None),           # K = 576: partial k-tile (5 tiles), two n-tiles
    ((2, 16, 8, 9, 9, 3, 2, 1, 1), None, None),             # stride 2, 9x9 -> 5x5: borders, odd sizes, M = 50
    ((2, 16, 24, 7, 7, 1, 1, 0, 1), (40, 8), (32, 8)),      # channel slices of wider buffers, sentinel next to them
    ((2, 16, 24, 7, 7, 1, 1, 0, 1), (40, 8), (32, 8)),      # the same problem again (same x / dy), its own dw
    ((2, 8, 8, 3, 3, 1, 1, 0, 1), None, None),              # M = 18 < one stage
    ((3, 8, 16, 24, 24, 3, 1, 1, 1), None, None),           # M = 1728, 27 stages: the problem that gets pixel splits
    ((3, 1024, 1024, 20, 20, 1, 1, 0, 1), None, None),      # 64 tiles x 19 stages, three times: the workgroup count of a real fork
    ((3, 1024, 1024, 20, 20, 1, 1, 0, 1), None, None),
    ((3, 1024, 1024, 20, 20, 1, 1, 0, 1), None, None),
]
REAL_GROUP = EXACT_GROUP[:4] + EXACT_GROUP[5:6]             # the five shapes
TARGETS = [1, 300, 1000]


def mnk(case):
    B, C, N, H, W, k, s, p, d = case
    OH, OW = R.out_hw(H, W, k, s, p, d)
    return B * OH * OW, N, k * k * C


def splits_and_total(cases, target):
    M, N, K = zip(*(mnk(c) for c in cases))
    pps, start = ops().wgrad_group_plan(M, N, K, target)
    return [-(-m // q) for m, q in zip(M, pps)], start[-1]


@functools.lru_cache(maxsize=None)
def exact_ref(case):
    """Integer operands and the float64 dW of one problem, computed once (callers do not write into them).  The 1x1 problems are a
    plain matrix product; the exactness conditions of `_conv_ref.assert_exact_conditions` that concern dW are asserted here."""
    B, C, N, H, W, k, s, p, d = case
    x, w, dy = R.int_operands(B, C, N, H, W, k, s, p, d, 1)
    if k == 1 and s == 1:
        dw = torch.einsum("bnhw,bchw->nc", dy, x).reshape(N, C, 1, 1)
    else:
        dw = R.conv_ref(x, w, dy, s, p, d, 1)[2]
    M = mnk(case)[0]
    assert torch.equal(dw, dw.round()) and 2 * dw.abs().max().item() < 2 ** 24
    assert 2 * M * x.abs().max().item() * dy.abs().max().item() < 2 ** 24, "a partial sum of dw could leave the exact f32 integers"
    return {"x": x, "dy": dy, "dw": dw}


class Pool:
    """The dW tensors of a group inside one f32 buffer, 64 sentinel floats before, between and after them."""
    GAP = 64

    def __init__(self, shapes):
        n = self.GAP + sum(torch.Size(s).numel() + self.GAP for s in shapes)
        self.buf = torch.full((n,), SENTINEL, device=DEV)
        self.dws, self.gaps, at = [], [(0, self.GAP)], self.GAP
        for s in shapes:
            m = torch.Size(s).numel()
            self.dws.append(self.buf[at:at + m].view(s).zero_())
            self.gaps.append((at + m, at + m + self.GAP))
            at += m + self.GAP

    def assert_gaps_untouched(self, what):
        for a, b in self.gaps:
            assert (self.buf[a:b] == SENTINEL).all(), f"{what}: wrote outside a dw (pool floats {a}..{b})"


def device_group(cases, refs, dtype):
    """(problems for ops.conv2d_wgrad_group, pool, views): identical (case, layout) entries share their x / dy views."""
    views, problems, shapes = {}, [], []
    for (case, xl, dl), r in zip(cases, refs):
        B, C, N, H, W, k, s, p, d = case
        OH, OW = R.out_hw(H, W, k, s, p, d)
        key = (case, xl, dl)
        if key not in views:
            views[key] = (View(B, H, W, C, dtype, *(xl or (None, 0)), src=r["x"]), View(B, OH, OW, N, dtype, *(dl or (None, 0)), src=r["dy"]))
        shapes.append((N, k, k, C))
    pool = Pool(shapes)
    for (case, xl, dl), dw in zip(cases, pool.dws):
        xv, dyv = views[(case, xl, dl)]
        k, s, p, d = case[5:]
        problems.append((xv.v, dyv.v, dw, k, s, p, d))
    return problems, pool, views


def run_group(problems, target):
    """One grouped call (atomic mode: the suite's default is the ordered one, which this entry point refuses), then the proof of
    which kernel ran."""
    with options(tune=0, deterministic=0):
        ops().conv2d_wgrad_group(problems, target)
        assert lib().get_option("wgrad_last_cfg") == GROUP_CFG, "the grouped kernel did not run"


def test_targets_reach_the_three_split_regimes():
    cases = [c for c, _, _ in EXACT_GROUP]
    s1, t1 = splits_and_total(cases, TARGETS[0])
    assert max(s1) == 1 and t1 <= RESIDENT_ROUND
    s2, t2 = splits_and_total(cases, TARGETS[1])
    assert max(s2) >= 3 and t2 <= RESIDENT_ROUND
    s3, t3 = splits_and_total(cases, TARGETS[2])
    assert max(s3) >= 3 and t3 > RESIDENT_ROUND


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("target", TARGETS)
def test_group_exact(target, dtype):
    refs = [exact_ref(c) for c, _, _ in EXACT_GROUP]
    problems, pool, views = device_group(EXACT_GROUP, refs, dtype)
    for n in (1, 2):                                                     # the second call adds onto the first: exactly twice
        run_group(problems, target)
        for i, (r, dw) in enumerate(zip(refs, pool.dws)):
            same(dw.permute(0, 3, 1, 2), n * r["dw"], f"problem {i} {R.case_id(EXACT_GROUP[i][0])} target {target} dw after call {n}")
        pool.assert_gaps_untouched(f"target {target} call {n}")
    for xv, dyv in views.values():
        xv.assert_neighbours_untouched("x")
        dyv.assert_neighbours_untouched("dy")


@pytest.mark.parametrize("count", [1, 32, 33])
def test_group_sizes_through_the_wrapper(count):
    assert lib().WGRAD_GROUP_MAX == 32
    cases = [EXACT_GROUP[i % 4 if i % 4 != 1 else 5] for i in range(count)]          # a mix of the small problems
    refs = [exact_ref(c) for c, _, _ in cases]
    problems, pool, _ = device_group(cases, refs, torch.float16)
    run_group(problems, 0)                                              # 33: two launches, 32 + 1
    for i, (r, dw) in enumerate(zip(refs, pool.dws)):
        same(dw.permute(0, 3, 1, 2), r["dw"], f"count {count} problem {i}")
    pool.assert_gaps_untouched(f"count {count}")


def test_refusals_on_the_device_leave_the_library_usable():
    E = lib().Sy11Error
    refs = [exact_ref(c) for c, _, _ in EXACT_GROUP[:2]]
    problems, pool, _ = device_group(EXACT_GROUP[:2], refs, torch.float16)
    with pytest.raises(E):
        ops().conv2d_wgrad_group([])
    with options(deterministic=1), pytest.raises(E):
        ops().conv2d_wgrad_group(problems)
    assert all((dw == 0).all() for dw in pool.dws)                       # refused before anything was launched
    f32 = View(2, 5, 7, 32, torch.float32, src=refs[0]["x"]), View(2, 5, 7, 40, torch.float32, src=refs[0]["dy"])
    with pytest.raises(E):
        ops().conv2d_wgrad_group([(f32[0].v, f32[1].v, pool.dws[0], 1, 1, 0, 1)])
    run_group(problems, 0)
    for r, dw in zip(refs, pool.dws):
        same(dw.permute(0, 3, 1, 2), r["dw"], "after the refusals")


# margin of the grouped kernel's worst err / bound over the per-layer kernel's.  Both multiply exactly and add the same M products
# per element in f32, in different orders (MFMA k-steps of 16 pixels, then stages, then atomics across splits): two samples of one
# error distribution.  The worst of a few thousand such samples varies by well under 2x between two orders; 4 leaves room for the
# smallest problems, whose worst element is one or two roundings.  Measured on the per-layer kernel ITSELF (64-wide tile,
# configuration 2, against 128-wide, configuration 6, f16 / bf16): see the figures printed by the test.
REAL_MARGIN = 4.0


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_group_real(dtype):
    """Worst err / bound of dw per problem, printed: grouped, per-layer (heuristic tile), per-layer forced to the 64- and 128-wide
    tiles.  Asserted: grouped <= 1 (the bound of `_conv_ref.real_case`) and grouped <= REAL_MARGIN x per-layer.

    Measured when the test was written (MI355X): the per-layer kernel against itself, 64- against 128-wide tile, 1.00 on every
    problem — these problems are one split of at most two stages, and both tiles add the pixels in the same k-step order — and
    the grouped kernel equal to both: worst err / bound 0.0028 ... 0.0136 in f16, 0.0020 ... 0.0085 in bf16.  The margin of 4 is
    the reasoned one above, not these figures."""
    o = ops()
    cases = [c + (1,) for c, _, _ in REAL_GROUP]
    rs = [R.real_case(*c, dtype=dtype) for c in cases]
    problems, pool, _ = device_group(REAL_GROUP, rs, dtype)
    run_group(problems, 1000)

    def ratio(dw, r):
        return R.worst_ratio(dw.permute(0, 3, 1, 2).cpu(), r["dw"], r["bound_dw"])
    grouped = [ratio(dw, r) for dw, r in zip(pool.dws, rs)]
    layer = {}
    for name, forced in (("heuristic", -1), ("tile64", 2), ("tile128", 6)):
        layer[name] = []
        with options(tune=0, deterministic=0, wgrad_cfg=forced):
            for (x, dy, dw, k, s, p, d), r in zip(problems, rs):
                one = torch.zeros_like(dw)
                o.conv2d_wgrad(x, dy, one, k, s, p, d)
                assert lib().get_option("wgrad_last_cfg") != GROUP_CFG
                layer[name].append(ratio(one, r))
    for i, c in enumerate(cases):
        print(f"\nREAL group {R.case_id(c)} {str(dtype)[6:]} M={rs[i]['M']}: worst err/bound grouped={grouped[i]:.4f} " +
              " ".join(f"{n}={v[i]:.4f}" for n, v in layer.items()))
    own = max(max(a, b) / max(min(a, b), 1e-30) for a, b in zip(layer["tile64"], layer["tile128"]))
    print(f"per-layer kernel against itself (64- vs 128-wide tile), largest ratio of the two worst errors: {own:.2f}; margin {REAL_MARGIN}")
    for i, c in enumerate(cases):
        assert grouped[i] <= 1.0, f"{R.case_id(c)} {dtype}: dw error is {grouped[i]:.3f} x its bound"
        assert grouped[i] <= REAL_MARGIN * layer["heuristic"][i], (R.case_id(c), grouped[i], layer["heuristic"][i])


# yolo11s layers of the 20x20 maps at batch 64 (M = 25 600), the sizes the engine groups: (C, N, H, W, k, s)
FULL_SIZE = [(512, 512, 20, 20, 1, 1), (128, 128, 20, 20, 3, 1), (256, 512, 40, 40, 3, 2), (1024, 512, 20, 20, 1, 1), (512, 64, 20, 20, 3, 1),
             (256, 128, 20, 20, 1, 1), (128, 80, 20, 20, 1, 1)]


def test_group_full_size_layers_agree_with_the_per_layer_kernels():
    """The grouped kernel at the shapes and the workgroup count of a real fork against the per-layer kernels on the same operands.
    Both results lie within `bound_dw` = (M + 4) 2^-23 S of the exact sum (S = the same sum over absolute values, `_conv_ref.real_case`),
    so they differ by at most twice that; S comes from the per-layer kernel itself (exact to 1e-3, hence the 1.01)."""
    o, B, dt = ops(), 64, torch.float16
    gen = torch.Generator(device=DEV).manual_seed(7)
    problems, layers = [], []
    for C, N, H, W, k, s in FULL_SIZE:
        p = k // 2
        OH, OW = R.out_hw(H, W, k, s, p, 1)
        x = (torch.rand(B, H, W, C, device=DEV, generator=gen) * 2 - 1).to(dt)
        dy = (torch.rand(B, OH, OW, N, device=DEV, generator=gen) * 2 - 1).to(dt)
        problems.append((x, dy, torch.zeros(N, k, k, C, device=DEV), k, s, p, 1))
    run_group(problems, 768)
    with options(tune=0, deterministic=0):
        for x, dy, dw, k, s, p, d in problems:
            one, S = torch.zeros_like(dw), torch.zeros_like(dw)
            o.conv2d_wgrad(x, dy, one, k, s, p, d)
            o.conv2d_wgrad(x.abs(), dy.abs(), S, k, s, p, d)
            assert lib().get_option("wgrad_last_cfg") != GROUP_CFG
            M = dy.shape[0] * dy.shape[1] * dy.shape[2]
            worst = ((dw - one).abs().double() / (2 * (M + 4) * R.U23 * 1.01 * S.double())).max().item()
            print(f"\nFULL {tuple(x.shape)} -> {tuple(dy.shape)} k{k} s{s}: |grouped - per layer| / (2 x bound) = {worst:.4f}")
            assert float(one.abs().max()) > 0 and worst <= 1.0


# ------------------------------------------------------------------------------------------------------------ engine
def _stack():
    from sy11.nn.modules.block import _EngineModule
    from sy11.nn.modules.conv import Conv

    class Stack(_EngineModule):
        def __init__(self):
            super().__init__()
            self.a, self.b, self.c = Conv(16, 16, 1), Conv(16, 24, 3), Conv(24, 16, 3, 2)

        def _run(self, ec, x, out=None):
            return self.c._run(ec, self.b._run(ec, self.a._run(ec, x)))
    return Stack


def _backward_once(group, monkeypatch):
    """Filter gradients of the three-Conv stack after one backward pass, and which filter-gradient configuration ran last."""
    from sy11 import engine
    monkeypatch.setattr(engine, "_WGRAD_GROUP", group)
    monkeypatch.setattr(engine, "_SIDE_WGRAD", True)                     # the defaults, whatever the environment says
    monkeypatch.setattr(engine, "_SIDE_BATCH", 32)
    torch.manual_seed(5)
    m = _stack()()
    m._sy11_dtype = torch.float16
    m = m.to(DEV).train()
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(2, 16, 12, 12, generator=gen).to(DEV)
    gy = torch.randn(2, 16, 6, 6, generator=gen).to(DEV)
    y = m(x)
    assert tuple(y.shape) == (2, 16, 6, 6)
    (y.float() * gy).sum().backward()
    torch.cuda.synchronize()
    return [c.conv.weight.grad.detach().clone() for c in (m.a, m.b, m.c)], lib().get_option("wgrad_last_cfg")


def test_engine_groups_the_small_filter_gradients(monkeypatch):
    with options(tune=0, deterministic=0):
        per_layer, cfg0 = _backward_once(False, monkeypatch)
        assert 0 <= cfg0 < 20
        grouped, cfg1 = _backward_once(True, monkeypatch)
        assert cfg1 == GROUP_CFG, "the engine did not issue a grouped launch"
    for g, r, name in zip(grouped, per_layer, "abc"):
        assert float(r.abs().max()) > 0
        close_to_scale(g, r.double(), torch.float16, f"conv {name} filter gradient, grouped vs per layer", mult=1)


def test_engine_keeps_the_per_layer_path_in_ordered_mode(monkeypatch):
    with options(tune=0, deterministic=1):
        off, cfg0 = _backward_once(False, monkeypatch)
        on, cfg1 = _backward_once(True, monkeypatch)
    assert 0 <= cfg0 < 20 and 0 <= cfg1 < 20, "ordered mode must not run the grouped (atomic) kernel"
    for a, b in zip(on, off):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "ordered mode: gradients differ with grouping switched on"
