"""GPU: every kernel of csrc/loss.hip on its own against the stage-wise reference of tests/_loss_ref.py.

Each stage gets the DEVICE's output of the stage before it, read back, as the reference's input, so a kernel is judged alone:
decode -> metrics -> selection (exact) -> norm and tss -> loss terms -> gradient -> finish.  The terms and gradient kernels take a
hand-made assignment written into the workspace (tests/_loss_ref.py:terms_case), which puts positives on all three strides, a
clamped DFL side, an integer distance, one in the last bin pair, a near-identical and a disjoint box pair in one small shape.

Floating comparisons: Bars.add(name, gpu, r64, r32), bar = 8 * e_ref + u * scale (+ sum_bound(k, sum|terms|) for the sums, k from
the kernels' geometry: _loss_ref.terms_k / norm_k).  tests/test_loss_ref_cpu.py shows on the CPU that the inputs take the same
branches in both precisions and that this bar catches six deliberate errors.
"""
from types import SimpleNamespace

import pytest
import torch

from tests import _loss_ref as R
from tests._kernel_ref import DEV, Bars, lib, ops, reduction_mode, same_bits, sum_bound  # noqa: F401

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
FILL = 1.0e3


def dev_maps(maps, offset=False):
    """Contiguous device copies; offset: each a contiguous VIEW that starts 4 bytes into its allocation (rows not 16-byte aligned)."""
    if not offset:
        return [m.to(DEV).contiguous() for m in maps], None
    bufs = [torch.full((m.numel() + 1,), FILL, dtype=F32, device=DEV) for m in maps]
    views = [b[1:].view(m.shape) for b, m in zip(bufs, maps)]
    for v, m in zip(views, maps):
        v.copy_(m.to(DEV))
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return views, bufs


def assign_on_device(maps, gt, strides, nc, offset=False):
    d, keep = dev_maps(maps, offset)
    w = ops().det_loss_assign(d, strides, nc, gt.to(DEV))
    torch.cuda.synchronize()
    return w, keep


# ------------------------------------------------------------------------------------------------------------------- a. decode
LEVELS = {3: [(6, 5), (3, 3), (2, 1)], 1: [(6, 5)], 2: [(6, 5), (3, 3)], 4: [(6, 5), (3, 3), (2, 1), (1, 1)]}


@pytest.mark.parametrize("nc", [3, 4])                       # scalar loads / 16-byte loads
@pytest.mark.parametrize("nl", [3, 1, 2, 4])
def test_decode(nl, nc):
    hw, B = LEVELS[nl], 2
    strides = (8.0, 16.0, 32.0, 64.0)[:nl]
    base = [torch.round(m * 1024) / 1024 for m in R.rand_maps(B, hw, nc, seed=nl)]        # on a 2^-10 grid: base +- 80 is exact in f32
    peaked = [m.clone() for m in base]
    equal = [m.clone() for m in base]
    for l, (p, e) in enumerate(zip(peaked, equal)):
        f = p.view(-1, 64 + nc)
        for s in range(4):
            f[torch.arange(f.shape[0]), s * 16 + (torch.arange(f.shape[0]) * 7 + 5 * s + l) % 16] = 30.0
        e[..., :64] = 0.625
    gt = torch.zeros(B, 0, 5)
    bars = Bars(f"decode nl={nl} nc={nc}")
    out = {}
    for name, maps in (("randn", base), ("peaked", peaked), ("equal", equal), ("shift+80", [m + 80 for m in base]),
                       ("shift-80", [m - 80 for m in base])):
        w, _ = assign_on_device(maps, gt, strides, nc)
        out[name] = w.pbox.cpu()
        ref = base if name.startswith("shift") else maps                               # shift invariance: the UNSHIFTED boxes
        bars.add(name, out[name], R.decode(ref, F64), R.decode(ref, F32))
    assert torch.equal(out["equal"].double(), R.decode(equal, F64)), "equal bins: the expectation is exactly 7.5"
    assert not (w.assign.cpu() >= 0).any() and float(w.norm.abs().max()) == 0.0         # no gt: nothing assigned
    bars.check()


# ------------------------------------------------------------------------------------------------------------------ b. metrics
@pytest.mark.parametrize("nc", [3, 4])
def test_metrics(nc):
    maps, gt, strides, _ = R.metrics_case(nc)
    w, _ = assign_on_device(maps, gt, strides, nc)
    pbox = w.pbox.cpu()
    o64, a64, mask = R.metrics(pbox, maps, gt, strides, F64)
    o32, a32, _ = R.metrics(pbox, maps, gt, strides, F32)
    ov, al = w.overlap.cpu(), w.align.cpu()
    assert not ov[~mask].any() and not al[~mask].any(), "outside the box / padded gt: exactly zero"
    assert int(mask.sum()) > 40 and int(((al > 0) & mask).sum()) > 20 and int(((al == 0) & (ov > 0) & mask).sum()) > 0      # score 0 (logit -200) inside
    bars = Bars(f"metrics nc={nc}")
    bars.add("overlap", ov, o64, o32)
    bars.add("align", al, a64, a32)
    bars.check()


# --------------------------------------------------------------------------------------- c, d. selection, norm and the tss sum
def check_assignment(name, maps, gt, strides, nc, bars):
    """One run of the assign entry: selection exact on the read-back metrics, maxima exact, norm and tss within the bar."""
    w, _ = assign_on_device(maps, gt, strides, nc)
    B, G, A = gt.shape[0], gt.shape[1], w.A
    al, ov = w.align.cpu(), w.overlap.cpu()
    mask = R.in_box(gt, R.hw_of(maps), strides, F32)
    topk, assign = R.select(al, ov, mask, R.valid_gt(gt))
    assert torch.equal(w.topk.cpu(), topk), f"{name}: top-{R.TOPK}"
    assert torch.equal(w.assign.cpu(), assign), f"{name}: assign"
    n64, pa64, po64, tss64 = R.norm(al, ov, assign, F64)
    n32, _, _, tss32 = R.norm(al, ov, assign, F32)
    pos = w.pos.cpu()
    assert torch.equal(pos[:B * G].view(B, G).double(), pa64) and torch.equal(pos[B * G:].view(B, G).double(), po64), f"{name}: atomic maxima"
    bars.add(f"{name} norm", w.norm.cpu(), n64, n32)
    k = R.norm_k(B * A)
    bars.add(f"{name} tss (k={k})", w.sums.cpu().double()[:, 0].sum(), tss64, tss32.double(), extra=sum_bound(k, n64.abs().sum().item()))
    assert not w.sums.cpu()[:, 1:].any()
    return w, topk, assign, mask, al, ov


@pytest.mark.parametrize("name", ["a21", "a189", "a189-zero", "a1029", "dense"])
def test_selection_norm_tss(name, reduction_mode):
    maps, gt, strides, nc = R.assign_case(name)
    bars = Bars(f"assign {reduction_mode}")
    w, topk, assign, mask, al, ov = check_assignment(name, maps, gt, strides, nc, bars)
    cand = torch.zeros_like(mask)
    for b in range(gt.shape[0]):
        for g in range(gt.shape[1]):
            if topk[b, g, 0] >= 0:
                cand[b, g, topk[b, g].long()] = True
    conflicts = int(((cand & mask).sum(1) > 1).sum())
    if name == "a189":
        assert conflicts > 0 and not (assign[0] == 2).any() and (assign[0] == 0).any(), "identical rows 0 and 2: the lower one wins every conflict"
        assert 0 < int(mask[0, 1].sum()) < R.TOPK, "a gt with fewer than ten anchors inside"
    if name == "a189-zero":
        assert not al.any() and torch.equal(topk[0, 0], torch.arange(R.TOPK, dtype=torch.int32)), "all-zero metrics: the ten lowest indices"
        assert float(w.norm.abs().max()) == 0.0
    if name == "dense":
        assert conflicts > 5
    bars.check()


def test_selection_with_the_top_k_buffer_past_48_kb():
    bars = Bars("assign lds")
    for name in ("lds-50176", "lds-153600"):
        maps, gt, strides, nc = R.assign_case(name)
        assert 4 * maps[0].shape[1] * maps[0].shape[2] == int(name.split("-")[1]) > 48 * 1024
        w, topk, assign, *_ = check_assignment(name, maps, gt, strides, nc, bars)
        assert int((assign >= 0).sum()) >= R.TOPK
    bars.check()


def test_assign_refuses_what_the_selection_cannot_hold():
    """Refusals of the host check only: neither shape is ever launched."""
    Sy11Error = lib().Sy11Error
    gt = torch.tensor([[[0.0, 1.0, 1.0, 20.0, 20.0]]], device=DEV)
    with pytest.raises(Sy11Error):                                               # 9 anchors < top-10
        ops().det_loss_assign([torch.zeros(1, 3, 3, 65, device=DEV)], (8.0,), 1, gt)
    with pytest.raises(Sy11Error):                                               # 40000 anchors: 160 000 bytes > the 150 KB buffer
        ops().det_loss_assign([torch.zeros(1, 200, 200, 65, device=DEV)], (8.0,), 1, gt)
    w = ops().det_loss_assign([torch.zeros(1, 3, 3, 65, device=DEV)], (8.0,), 1, gt[:, :0])      # no gt: nothing to select, decode only
    torch.cuda.synchronize()
    assert not (w.assign.cpu() >= 0).any()


def test_tss_slots_wrap():
    """B * A = 2 * 8400 anchors: 66 workgroups onto the 64 slots."""
    hw, B, nc = [(80, 80), (40, 40), (20, 20)], 2, 1
    gen = torch.Generator().manual_seed(5)
    maps = R.rand_maps(B, hw, nc, seed=6)
    gt = R.pad_gt([R.rand_boxes(3, 640, 640, gen, nc, 0.2, 0.6) for _ in range(B)])
    assert -(-B * 8400 // 256) == 66
    prev = lib().get_option("deterministic")
    try:
        for mode in (1, 0):
            lib().set_option("deterministic", mode)
            bars = Bars(f"assign {'ordered' if mode else 'atomic'}")
            w, *_ = check_assignment("wrap-16800", maps, gt, R.STRIDES, nc, bars)
            if not mode:
                assert int((w.sums.cpu()[:, 0] != 0).sum()) >= 1
            bars.check()
    finally:
        lib().set_option("deterministic", prev)


# --------------------------------------------------------------------------------------------- e, f. loss terms and gradient
TERMS = [("nc1", dict(nc=1), False), ("nc3", dict(nc=3), False), ("nc4", dict(nc=4), False), ("nc4-offset", dict(nc=4), True),
         ("nc64", dict(nc=64, seed=3), False), ("nc68", dict(nc=68, seed=4), False), ("nc80", dict(nc=80, seed=1), False),
         ("nc132", dict(nc=132, seed=5), False), ("nc132-offset", dict(nc=132, seed=5), True),
         ("grid-stride", dict(nc=4, hw=((80, 80), (40, 40), (20, 20)), B=4, seed=2), False)]


def workspace_for(c, offset):
    """The assign entry on the case's maps (decode is checked on the way), then the hand-made assignment in place of the device's."""
    w, keep = assign_on_device(c["maps"], c["gt"], c["strides"], c["nc"], offset)
    w.assign.copy_(c["assign"].to(DEV))
    w.norm.copy_(c["w"].to(DEV))
    w.zero.zero_()
    return w, keep


@pytest.mark.parametrize("name,kw,offset", TERMS, ids=[t[0] for t in TERMS])
def test_terms_and_gradient(name, kw, offset, reduction_mode):
    K = ops()
    c = R.terms_case(**kw)
    B, A = c["assign"].shape
    nc, gt, asg, wt, st = c["nc"], c["gt"], c["assign"], c["w"], c["strides"]
    if name == "grid-stride":
        assert -(-B * A // 16) == 2100 > 2048
    else:
        assert (B * A) % 16 != 0
    w, keep = workspace_for(c, offset)
    bars = Bars(f"terms {name} {reduction_mode}")
    pbox = w.pbox.cpu()
    bars.add("decode", pbox, R.decode(c["maps"], F64), R.decode(c["maps"], F32))
    if offset:
        w0, _ = assign_on_device(c["maps"], gt, st, nc)
        assert same_bits(pbox, w0.pbox), "decode through the unaligned view: the same bits as through the aligned map"
    # ---- e. the three sums
    K.det_loss_terms(w)
    sums = w.sums.cpu().double().sum(0)
    assert sums[0] == 0
    with torch.no_grad():
        s64 = R.terms([m.double() for m in c["maps"]], gt, asg, wt, st, F64)
        s32 = R.terms(c["maps"], gt, asg, wt, st, F32)
    extra, k = R.terms_extra(c), R.terms_k(nc, B * A)
    for q, n in enumerate(("box", "cls", "dfl")):
        bars.add(f"sum {n} (k={k})", sums[1 + q], s64[q], s32[q].double(), extra=extra[f"sum {n}"])
    # ---- f. the gradient, branch by branch and level by level; kernel: d/d maps of upstream * B * (gains . sums)
    one = torch.ones(1, device=DEV)
    pos_w = ((asg >= 0) & (wt > 0))
    a0 = c["a0"] + [A]
    grads = {}
    for gains in R.GAIN_SETS:
        dm = K.det_loss_backward(w, one, gains)
        grads[gains] = dm
        _, g64 = R.terms_with_grad(c["maps"], gt, asg, wt, st, F64, gains, upstream=float(B))
        _, g32 = R.terms_with_grad(c["maps"], gt, asg, wt, st, F32, gains, upstream=float(B))
        for l in range(3):
            d = dm[l].cpu()
            bars.add(f"grad {gains} L{l} dist", d[..., :64], g64[l][..., :64], g32[l][..., :64])
            bars.add(f"grad {gains} L{l} cls", d[..., 64:], g64[l][..., 64:], g32[l][..., 64:])
            dist = d[..., :64].reshape(B, -1, 64)
            assert not dist[~pos_w[:, a0[l]:a0[l + 1]]].any(), "distribution channels of an unassigned or zero-weight anchor: exactly zero"
            if gains == (0.0, 1.0, 0.0):
                assert not dist.any(), "class gain only: no distribution-channel gradient"
    # ---- the upstream scalar, three ways (gains of the product)
    gains = R.GAIN_SETS[3]
    ref = [g.cpu().double() for g in grads[gains]]
    three = torch.full((1,), 3.0, device=DEV)
    d3 = K.det_loss_backward(w, three, gains)
    w.sums[0, 0] = 2.5                                                             # tss: det_loss_finish -> out[4] = 1 / 2.5
    fin = K.det_loss_finish(w, gains)
    d3t = K.det_loss_backward(w, three, gains, inv_tss=fin[4:5])
    outs = [torch.full_like(m, FILL) for m in w.maps]
    d3o = K.det_loss_backward(w, three, gains, out=outs)
    inv = float(fin[4].item())
    assert inv == R.f32(1 / 2.5)
    _, g64 = R.terms_with_grad(c["maps"], gt, asg, wt, st, F64, gains, upstream=3.0 * B)
    _, g32 = R.terms_with_grad(c["maps"], gt, asg, wt, st, F32, gains, upstream=3.0 * B)
    for l in range(3):
        bars.add(f"upstream 3 L{l}", d3[l].cpu(), g64[l], g32[l])
        bars.add(f"upstream 3 / tss L{l}", d3t[l].cpu(), g64[l] * inv, g32[l] * inv)
        assert d3o[l] is outs[l] and same_bits(d3o[l], d3[l]), "out= buffers: the same bits as fresh tensors"
        assert ref[l].abs().max() > 0
    if keep is not None:
        assert all(float(b[0]) == FILL for b in keep), "the 4 bytes in front of an offset map are untouched"
    bars.check()


# ------------------------------------------------------------------------------------------------------------------- g. finish
@pytest.mark.parametrize("tss_scale", [0.25, 40.0])                                # tss < 1: clamped to 1;  tss > 1
def test_finish(tss_scale):
    g = torch.Generator().manual_seed(9)
    sums = torch.randint(0, 64, (64, 4), generator=g).float() / 64                  # multiples of 1/64: every partial sum is exact in f32
    sums[:, 0] *= tss_scale / 32
    B, gains = 4, (7.5, 0.5, 1.5)
    tot = sums.double().sum(0)
    assert (tot[0] < 1) == (tss_scale < 1) and torch.equal(sums.sum(0).double(), tot)
    out = ops().det_loss_finish(SimpleNamespace(sums=sums.to(DEV), B=B), gains)
    bars = Bars(f"finish tss={tot[0].item():.3f}")
    r64, r32 = R.finish(tot, B, gains, F64), R.finish(tot.float(), B, gains, F32)
    for i, n in enumerate(("loss", "box", "cls", "dfl", "1/tss")):
        bars.add(n, out[i].cpu(), r64[i], r32[i])
    if tss_scale < 1:
        assert float(out[4]) == 1.0
    bars.check()
