"""Stage-wise reference of the detection criterion (csrc/loss.hip), generic in dtype, and the input builders of the kernel-level
loss tests (test_loss_ref_cpu.py checks them on the CPU, test_loss_kernels_gpu.py feeds them to the kernels).  Not a test module
and not a conftest.

One function per kernel stage, each a plain restatement of utils/loss.py, utils/tal.py and utils/metrics.py (the same lines
oracle/loss_ref.py follows) evaluated in ``dtype`` (float32 or float64):

    decode  -> pbox                      loss_decode_kernel
    metrics -> overlap, align, mask      loss_tal_metrics_kernel (the values)
    select  -> topk, assign              loss_tal_metrics_kernel (top-10) + loss_tal_resolve_kernel; integers, exact
    norm    -> w, pos_align, pos_ov, tss loss_tal_resolve_kernel (maxima) + loss_tal_norm_kernel
    terms   -> box, cls, dfl sums        loss_terms_kernel<false>; autograd of it is the reference of loss_terms_kernel<true>
    finish  -> loss, items, 1/tss        loss_finish_kernel

Maps are NHWC (B, H, W, 64 + nc) tensors, one per level; gt is (B, G, 5) [cls, x1, y1, x2, y2] in pixels with all-zero padding
rows.  Constants the kernels hold as f32 (1e-7, 1e-9, 15 - 0.01, 4 / pi^2) enter both precisions with their f32 value: that is an
input rounding, not a kernel error.
"""
import math

import numpy as np
import torch

from tests._kernel_ref import Bars, reduction_mode, rnd, same_bits, sum_bound  # noqa: F401  (re-exported to the two test files)

REG, TOPK = 16, 10
STRIDES = (8.0, 16.0, 32.0)


def f32(v):
    return float(np.float32(v))


EPS = f32(1e-7)                                              # bbox_iou's eps
EPS_TAL = f32(1e-9)                                          # the assigner's eps
DFL_MAX = float(np.float32(REG - 1) - np.float32(0.01))     # reg_max - 1 - 0.01 as the kernel forms it
C_V = f32(4 / math.pi ** 2)
MUTATIONS = ("box_scale", "clamp15", "stride0", "alpha_grad", "no_heps", "class_off")


def hw_of(maps):
    return [(m.shape[1], m.shape[2]) for m in maps]


def grid(hw, strides, dtype):
    """-> anchor centres (A, 2) in grid units (x + 0.5, y + 0.5), stride per anchor (A,), level per anchor (A,)."""
    pts, st, lv = [], [], []
    for l, ((h, w), s) in enumerate(zip(hw, strides)):
        gy, gx = torch.meshgrid(torch.arange(h, dtype=dtype) + 0.5, torch.arange(w, dtype=dtype) + 0.5, indexing="ij")
        pts.append(torch.stack((gx, gy), -1).view(-1, 2))
        st.append(torch.full((h * w,), float(s), dtype=dtype))
        lv.append(torch.full((h * w,), l, dtype=torch.long))
    return torch.cat(pts), torch.cat(st), torch.cat(lv)


def rows(maps, dtype):
    """(B, A, 64 + nc): one row per anchor, levels one after the other."""
    return torch.cat([m.reshape(m.shape[0], -1, m.shape[-1]).to(dtype) for m in maps], 1)


def expectation(dist):
    """(..., 4 * REG) logits -> (..., 4) softmax expectation of the bin index."""
    d = dist.reshape(*dist.shape[:-1], 4, REG).softmax(-1)
    return d.matmul(torch.arange(REG, dtype=dist.dtype))


def decode(maps, dtype):
    """-> pbox (B, A, 4) xyxy in grid units: anchor -/+ the softmax expectation of each side (loss.py:212-218, tal.py:dist2bbox)."""
    x = rows(maps, dtype)
    anc, _, _ = grid(hw_of(maps), STRIDES[:1] * len(maps), dtype)
    ex = expectation(x[..., :4 * REG])
    return torch.cat((anc - ex[..., :2], anc + ex[..., 2:]), -1)


def ciou(b1, b2, mutate=()):
    """bbox_iou(xywh=False, CIoU=True), metrics.py:199-228: h gets +eps, w does not; alpha under no_grad."""
    b1x1, b1y1, b1x2, b1y2 = b1.unbind(-1)
    b2x1, b2y1, b2x2, b2y2 = b2.unbind(-1)
    he = 0.0 if "no_heps" in mutate else EPS
    w1, h1 = b1x2 - b1x1, b1y2 - b1y1 + he
    w2, h2 = b2x2 - b2x1, b2y2 - b2y1 + he
    inter = (torch.minimum(b1x2, b2x2) - torch.maximum(b1x1, b2x1)).clamp(min=0) * \
            (torch.minimum(b1y2, b2y2) - torch.maximum(b1y1, b2y1)).clamp(min=0)
    union = w1 * h1 + w2 * h2 - inter + EPS
    iou = inter / union
    cw = torch.maximum(b1x2, b2x2) - torch.minimum(b1x1, b2x1)
    ch = torch.maximum(b1y2, b2y2) - torch.minimum(b1y1, b2y1)
    c2 = cw ** 2 + ch ** 2 + EPS
    rho2 = ((b2x1 + b2x2 - b1x1 - b1x2) ** 2 + (b2y1 + b2y2 - b1y1 - b1y2) ** 2) / 4
    v = C_V * (torch.atan(w2 / h2) - torch.atan(w1 / h1)) ** 2
    if "alpha_grad" in mutate:
        alpha = v / (v - iou + (1 + EPS))
    else:
        with torch.no_grad():
            alpha = v / (v - iou + (1 + EPS))
    return iou - (rho2 / c2 + v * alpha)


def valid_gt(gt):
    """mask_gt (loss.py:243) with the kernel's f32 order of the four adds."""
    b = gt[..., 1:5].float()
    return (((b[..., 0] + b[..., 1]) + b[..., 2]) + b[..., 3]) > 0


def in_box(gt, hw, strides, dtype):
    """(B, G, A): the anchor centre (pixels) lies strictly inside the gt and the gt is not padding (tal.py:242-263)."""
    anc, st, _ = grid(hw, strides, dtype)
    pts = anc * st[:, None]
    g = gt[..., 1:5].to(dtype)
    d = torch.cat((pts[None, None] - g[:, :, None, :2], g[:, :, None, 2:] - pts[None, None]), -1)
    return (d.amin(-1) > EPS_TAL) & valid_gt(gt)[..., None]


def metrics(pbox, maps, gt, strides, dtype):
    """-> overlap (B, G, A) = CIoU(gt, pred box in pixels).clamp(0), align = score^0.5 * overlap^6, both zero outside ``mask``
    (tal.py:132-155), and mask = in_box."""
    B, G = gt.shape[:2]
    x = rows(maps, dtype)
    A = x.shape[1]
    _, st, _ = grid(hw_of(maps), strides, dtype)
    mask = in_box(gt, hw_of(maps), strides, dtype)
    pb = (pbox.to(dtype) * st[:, None])[:, None].expand(B, G, A, 4)
    gb = gt[..., 1:5].to(dtype)[:, :, None].expand(B, G, A, 4)
    ov = ciou(gb, pb).clamp(min=0)
    cls = gt[..., 0].long().clamp(min=0)
    sc = x[..., 4 * REG:].sigmoid().gather(2, cls[:, None, :].expand(B, A, G)).transpose(1, 2)
    al = sc.pow(0.5) * ov.pow(6)
    zero = torch.zeros((), dtype=dtype)
    return torch.where(mask, ov, zero), torch.where(mask, al, zero), mask


def select(align, overlap, mask, valid):
    """The contract documented in loss.hip, on f32 metrics: per valid gt the TOPK anchors by align (value descending, index
    ascending), -1 rows for padded gts; an anchor is a candidate of every gt that picked it and contains it; one candidate gt ->
    that gt, several -> the FIRST maximum of overlap over ALL gts.  -> topk (B, G, TOPK) int32, assign (B, A) int32 (-1: none)."""
    al = align.detach().cpu().numpy().astype(np.float32)
    ov = overlap.detach().cpu().numpy().astype(np.float32)
    m, v = mask.cpu().numpy().astype(bool), valid.cpu().numpy().astype(bool)
    B, G, A = al.shape
    topk = -np.ones((B, G, TOPK), np.int32)
    if G == 0:
        return torch.from_numpy(topk), torch.full((B, A), -1, dtype=torch.int32)
    cand = np.zeros((B, G, A), bool)
    for b in range(B):
        for g in range(G):
            if v[b, g]:
                idx = np.argsort(-al[b, g], kind="stable")[:TOPK]
                topk[b, g] = idx
                cand[b, g, idx] = True
    cand &= m
    count, first, best = cand.sum(1), cand.argmax(1), ov.argmax(1)
    assign = np.where(count > 1, best, np.where(count == 1, first, -1)).astype(np.int32)
    return torch.from_numpy(topk), torch.from_numpy(assign)


def norm(align, overlap, assign, dtype):
    """-> w (B, A) = align * pos_ov / (pos_align + eps) of the assigned gt (tal.py:115-120; = the sum of the anchor's target
    scores), the per-gt maxima pos_align, pos_ov (B, G) over the anchors assigned to it, and tss = w.sum()."""
    al, ov = align.to(dtype), overlap.to(dtype)
    B, G, A = al.shape
    pos, idx = assign >= 0, assign.clamp(min=0).long()
    if G == 0:
        z = torch.zeros(B, A, dtype=dtype)
        return z, torch.zeros(B, 0, dtype=dtype), torch.zeros(B, 0, dtype=dtype), z.sum()
    onehot = torch.zeros(B, G, A, dtype=torch.bool).scatter_(1, idx[:, None, :], pos[:, None, :])
    zero = torch.zeros((), dtype=dtype)
    pos_align = torch.where(onehot, al, zero).amax(-1)
    pos_ov = torch.where(onehot, ov, zero).amax(-1)
    a_sel = al.gather(1, idx[:, None, :])[:, 0]
    w = torch.where(pos, a_sel * pos_ov.gather(1, idx) / (pos_align.gather(1, idx) + EPS_TAL), zero)
    return w, pos_align, pos_ov, w.sum()


def targets(gt, assign, hw, strides, dtype, mutate=()):
    """-> pos (B, A) bool, label (B, A), target boxes in grid units (B, A, 4) (loss.py:266), anchor centres (A, 2)."""
    anc, st, lv = grid(hw, strides, dtype)
    if "stride0" in mutate:
        st = torch.full_like(st, float(strides[0]))
    pos, idx = assign >= 0, assign.clamp(min=0).long()
    row = gt.to(dtype)[torch.arange(gt.shape[0])[:, None], idx] if gt.shape[1] else torch.zeros(*assign.shape, 5, dtype=dtype)
    return pos, row[..., 0].long().clamp(min=0), row[..., 1:5] / st[None, :, None], anc


def dfl_targets(anc, tbox, mutate=()):
    """bbox2dist (tal.py:361-364) + DFLoss's clamp (loss.py:77): (..., 4) target distances in [0, 14.99]."""
    hi = float(REG - 1) if "clamp15" in mutate else DFL_MAX
    return torch.cat((anc - tbox[..., :2], tbox[..., 2:] - anc), -1).clamp(0, hi)


def terms(maps, gt, assign, w, strides, dtype, mutate=()):
    """-> the three un-normalised sums (box, cls, dfl) of loss.py:250-275 / BboxLoss / DFLoss for a GIVEN assignment; differentiable
    in ``maps`` (tensors of ``dtype``).  ``mutate``: names from MUTATIONS, each one deliberate error (test_loss_ref_cpu.py)."""
    x = rows(maps, dtype)
    B, A, no = x.shape
    nc = no - 4 * REG
    pos, label, tbox, anc = targets(gt, assign, hw_of(maps), strides, dtype, mutate)
    w = torch.where(pos, w.to(dtype), torch.zeros((), dtype=dtype))
    if "class_off" in mutate:
        label = (label + 1) % nc
    t = torch.zeros(B, A, nc, dtype=dtype).scatter_(2, label[..., None], w[..., None])
    cls = torch.nn.functional.binary_cross_entropy_with_logits(x[..., 4 * REG:], t, reduction="none").sum()
    ex = expectation(x[..., :4 * REG])
    pbox = torch.cat((anc - ex[..., :2], anc + ex[..., 2:]), -1)
    wp = w[pos]
    box = ((1.0 - ciou(pbox[pos], tbox[pos], mutate)) * wp).sum()
    if "box_scale" in mutate:
        box = box * 0.999
    tgt = dfl_targets(anc, tbox, mutate)[pos]
    tl = tgt.long()
    wl = (tl + 1).to(dtype) - tgt
    wr = 1 - wl
    logp = x[..., :4 * REG].reshape(B, A, 4, REG)[pos].log_softmax(-1)
    ce_l = -logp.gather(-1, tl[..., None])[..., 0]
    ce_r = -logp.gather(-1, (tl + 1).clamp(max=REG - 1)[..., None])[..., 0]          # tl + 1 = 16 only under "clamp15", with wr = 0
    dfl = ((ce_l * wl + ce_r * wr).mean(-1) * wp).sum()
    return box, cls, dfl


def finish(sums, B, gains, dtype):
    """sums (4,) = [tss, box, cls, dfl] -> [loss, box item, cls item, dfl item, 1 / max(tss, 1)] (loss.py:268-275)."""
    s = sums.to(dtype)
    tss = s[0].clamp(min=1)
    items = s[1:] / tss * torch.tensor([f32(g) for g in gains], dtype=dtype)
    return torch.cat((((items[0] + items[1]) + items[2]).view(1) * B, items, (1 / tss).view(1)))


def terms_with_grad(maps, gt, assign, w, strides, dtype, gains, upstream=1.0, mutate=()):
    """-> (box, cls, dfl) sums and d/d maps of upstream * (gains . sums); the caller supplies the normalisation in ``upstream``."""
    leaves = [m.detach().to(dtype).clone().requires_grad_(True) for m in maps]
    s = terms(leaves, gt, assign, w, strides, dtype, mutate)
    total = (s[0] * f32(gains[0]) + s[1] * f32(gains[1]) + s[2] * f32(gains[2])) * upstream
    total.backward()
    return [v.detach() for v in s], [m.grad if m.grad is not None else torch.zeros_like(m) for m in leaves]


# ------------------------------------------------------------------------------------------------------------------ input builders
def eighths(v):
    """Round to a multiple of 1/8 pixel: exact in f32 and f64, and still exact after the division by a stride of 8, 16 or 32."""
    return torch.round(torch.as_tensor(v, dtype=torch.float64) * 8) / 8


def pad_gt(per_image):
    """list (per image) of [cls, x1, y1, x2, y2] rows -> (B, G, 5) f32 with zero rows as padding; None keeps a zero row in place."""
    G = max((len(r) for r in per_image), default=0)
    gt = torch.zeros(len(per_image), G, 5, dtype=torch.float64)
    for b, rws in enumerate(per_image):
        for g, r in enumerate(rws):
            if r is not None:
                gt[b, g] = torch.as_tensor(r, dtype=torch.float64)
    assert torch.equal(gt[..., 1:] * 64, torch.round(gt[..., 1:] * 64)), "corners on the 1/64-pixel grid at the finest: exact in f32"
    return gt.float()


def rand_boxes(n, sw, sh, gen, nc, lo=0.2, hi=0.7):
    """n rows [cls, x1, y1, x2, y2]: corners on the 1/8-pixel grid, sides between lo and hi of the image, inside the image."""
    out = []
    for _ in range(n):
        u = torch.rand(4, generator=gen, dtype=torch.float64)
        bw, bh = (lo + (hi - lo) * u[0]) * sw, (lo + (hi - lo) * u[1]) * sh
        x1, y1 = u[2] * (sw - bw), u[3] * (sh - bh)
        c = float(torch.randint(0, nc, (1,), generator=gen))
        out.append([c] + eighths(torch.stack((x1, y1, x1 + bw, y1 + bh)) + 1 / 16).tolist())
    return out


def rand_maps(B, hw, nc, seed, scale=1.5):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, h, w, 4 * REG + nc, generator=g) * scale for h, w in hw]


def metrics_case(nc=3):
    """Section b: levels (6,5),(3,3),(2,1) (a 40 x 48 image), B = 3, G = 4.  Image 0: a gt whose left and top edges pass exactly
    through anchor centres (x1 = y1 = 4 = the centre of the first stride-8 cell: dmin = 0, excluded), a padded row in the middle, a
    gt over the whole image; image 1: no gt; image 2: random boxes.  Class logits of the gts' classes are set to -200, 0, +30."""
    hw = [(6, 5), (3, 3), (2, 1)]
    gen = torch.Generator().manual_seed(11)
    maps = rand_maps(3, hw, nc, seed=12)
    gt = pad_gt([[[1, 4.0, 4.0, 36.125, 44.0], [0, 9.5, 10.25, 30.75, 40.5], None, [nc - 1, 0.125, 0.125, 39.875, 47.875]],
                 [],
                 rand_boxes(4, 40, 48, gen, nc, 0.4, 0.9)])
    for l, m in enumerate(maps):
        f = m.view(3, -1, 64 + nc)
        for k, v in enumerate((-200.0, 0.0, 30.0)):
            f[:, k::5, 64 + (k % nc)] = v
            f[0, (k + 3)::7, 64 + 1] = v
    return maps, gt, STRIDES, nc


def terms_case(nc, hw=((20, 20), (10, 10), (5, 5)), B=2, seed=0):
    """Section e: head maps, gt, a hand-made assignment and weights for the loss-terms and gradient kernels.

    gt rows per image (pixels, 1/8 grid; S = 8 * W0 wide, 8 * H0 high):
      0  nearly the whole image: ten random anchors of EVERY level (all of a level that has fewer) and the stride-8 anchor at
         gx = W0 - 1, whose left distance W0 - 0.64 > 14.99 is CLAMPED (W0 >= 16)
      1  x1 = 12, y1 = 20 (cell centres of stride 8): its stride-8 anchors have EXACTLY INTEGER left / top distances
      2  x1 = 8 * (W0 - 16): the stride-8 anchor at gx = W0 - 2 has left distance 14.5, in the LAST BIN PAIR [14, 14.99)
      3  around the stride-16 anchor (3, 2): its DFL logits put the expectation within 1e-2 (and more than 1e-3) of the target on
         every side (two-bin distributions) — the NEAR-IDENTICAL pair
      4  right of the stride-8 anchor (2, 5), whose peaked logits give a box one cell wide: DISJOINT on x (negative left distance,
         clamped to 0)
      5  padding in image 0, a random box elsewhere
      6  a square of 1/32 pixel (2^-10 grid units) centred on the stride-32 anchor (1, 1), whose two-bin logits predict a 4 x 0.8
         box: the one place where the +eps of CIoU's h (1e-7) is a visible fraction of a height (1e-4 of it), so that dropping it
         moves atan(w2 / h2) by 5e-5.  (At the near-identical pair both heights are ~4 and f32 holds the predicted edges no finer
         than the 1e-7 that eps adds.)  Its corners are on the 1/64-pixel grid, all other rows on the 1/8-pixel grid.
    w is uniform in [0.25, 1]; every seventh positive has w = 0.  Class logits +-30 and +-90 are planted on and off positives."""
    hw = [tuple(p) for p in hw]
    (H0, W0), S = hw[0], STRIDES
    assert W0 >= 18 and H0 >= 12 and len(hw) == 3
    sw, sh = 8.0 * W0, 8.0 * H0
    gen = torch.Generator().manual_seed(100 + seed)
    maps = rand_maps(B, hw, nc, seed=200 + seed)
    a0 = [0, hw[0][0] * hw[0][1], hw[0][0] * hw[0][1] + hw[1][0] * hw[1][1]]
    A = a0[2] + hw[2][0] * hw[2][1]
    near_c, near_d = (3.5, 2.5), (2.3125, 1.5625, 3.4375, 2.6875)             # stride-16 cell (3, 2); distances in grid units
    per_image, assign = [], torch.full((B, A), -1, dtype=torch.int32)
    for b in range(B):
        rws = [[b % nc, 1.125, 2.25, sw - 3.5, sh - 1.75],
               [(b + 1) % nc, 12.0, 20.0, sw - 12.5, sh - 20.25],
               [(b + 2) % nc, 8.0 * (W0 - 16), 3.375, sw - 0.625, sh - 5.125],
               [nc - 1, 16 * (near_c[0] - near_d[0]), 16 * (near_c[1] - near_d[1]), 16 * (near_c[0] + near_d[2]), 16 * (near_c[1] + near_d[3])],
               [0, 50.0, 20.5, 50.0 + 40.25, 70.75],
               None if b == 0 else rand_boxes(1, sw, sh, gen, nc)[0],
               [b % nc, 48 - 1 / 64, 48 - 1 / 64, 48 + 1 / 64, 48 + 1 / 64]]
        per_image.append(rws)
        for l, (h, w) in enumerate(hw):
            n = h * w
            pick = torch.randperm(n, generator=gen)[:min(10, n)] + a0[l]
            assign[b, pick] = 0
        y = H0 // 2
        assign[b, y * W0 + W0 - 1] = 0                                         # clamped
        for gx, gy in ((5, 6), (7, 4), (9, 8)):
            assign[b, gy * W0 + gx] = 1                                        # integer distances gx - 1, gy - 2
        assign[b, (y + 1) * W0 + W0 - 2] = 2                                   # 14.5
        assign[b, a0[1] + 2 * hw[1][1] + 3] = 3                                # near-identical
        assign[b, 5 * W0 + 2] = 4                                              # disjoint
        assign[b, a0[2] + hw[2][1] + 1] = 6                                    # tiny target
        if b > 0:
            inside = in_box(pad_gt([[rws[5]]]), hw, S, torch.float64)[0, 0].nonzero()[:, 0]
            assign[b, inside[torch.randperm(len(inside), generator=gen)[:6]]] = 5
    gt = pad_gt(per_image)
    pos = assign >= 0
    w = torch.zeros(B, A)
    w[pos] = 0.25 + 0.75 * torch.rand(int(pos.sum()), generator=gen)
    zero_w = pos.nonzero()[::7]
    w[zero_w[:, 0], zero_w[:, 1]] = 0.0
    for b in range(B):
        w[b, a0[1] + 2 * hw[1][1] + 3] = 0.75                                  # the special anchors keep a weight
        w[b, 5 * W0 + 2] = 0.5
        w[b, a0[2] + hw[2][1] + 1] = 1.0
        w[b, (H0 // 2) * W0 + W0 - 1] = 1.0
    flat = [m.view(B, -1, 4 * REG + nc) for m in maps]
    delta = (4e-3, -6e-3, 5e-3, -3e-3)
    for b in range(B):
        r = flat[1][b, 2 * hw[1][1] + 3]
        for s in range(4):
            fl, fr = int(near_d[s]), near_d[s] - int(near_d[s]) + delta[s]
            r[s * REG:(s + 1) * REG] = -30.0
            r[s * REG + fl] = 0.0
            r[s * REG + fl + 1] = math.log(fr / (1 - fr))
        r = flat[2][b, hw[2][1] + 1]
        r[:4 * REG] = -30.0
        r[0 * REG + 2] = r[2 * REG + 2] = 0.0                                  # left = right = 2
        r[1 * REG] = r[3 * REG] = 0.0
        r[1 * REG + 1] = r[3 * REG + 1] = math.log(0.4 / 0.6)                  # top = bottom = 0.4
        r = flat[0][b, 5 * W0 + 2]
        r[:4 * REG:REG] -= 2.0
        r[1:4 * REG:REG] = 20.0                                                # peaked at bin 1 on every side
    vals = (30.0, -30.0, 90.0, -90.0)
    for l in range(3):
        for b in range(B):
            n = flat[l].shape[1]
            for k, v in enumerate(vals):
                flat[l][b, (3 * k + b) % n, 4 * REG + (k % nc)] = v            # wherever they fall
            ps = (assign[b, a0[l]:a0[l] + n] >= 0).nonzero()[:, 0]
            lab = gt[b, assign[b, a0[l] + ps].long(), 0].long()
            for k, v in enumerate(vals):
                if k < len(ps):
                    flat[l][b, ps[k], 4 * REG + lab[k]] = v                    # on a positive's own class
    return {"maps": maps, "gt": gt, "assign": assign, "w": w, "strides": S, "nc": nc, "hw": hw, "a0": a0}


def kinks(case, dtype):
    """What decides a branch of the terms kernels, per positive: the six CIoU kink distances (pred - target corners, the raw
    intersection width and height), the unclamped DFL distances, and floor() of the clamped ones."""
    maps = [m.to(dtype) for m in case["maps"]]
    pos, _, tbox, anc = targets(case["gt"], case["assign"], case["hw"], case["strides"], dtype)
    p, t = decode(maps, dtype)[pos], tbox[pos]
    a = anc[None].expand(pos.shape[0], -1, -1)[pos]
    iwr = torch.minimum(p[:, 2], t[:, 2]) - torch.maximum(p[:, 0], t[:, 0])
    ihr = torch.minimum(p[:, 3], t[:, 3]) - torch.maximum(p[:, 1], t[:, 1])
    raw = torch.cat((a - t[:, :2], t[:, 2:] - a), -1)
    return torch.cat((p - t, iwr[:, None], ihr[:, None]), 1), raw, dfl_targets(a, t).floor()


def fold_depth(nb):
    """Additions a workgroup partial passes through after it leaves its workgroup, the larger of the two reduction modes.  Atomic:
    arrivals on one of 64 slots, ceil(nb / 64), then the 64-slot fold.  Ordered (csrc/det.h, sy11_fold_rows_ordered): stages of 64
    rows while more than 256 rows are left, then one stage whose four quarter-columns take up to 64 rows each, are joined by 3 adds
    and added to the output."""
    atomic = -(-nb // 64) + 64
    rows_, ordered = nb, 0
    while rows_ > 256:
        ordered += 64
        rows_ = -(-rows_ // 64)
    ordered += min(rows_, 64) + 3 + 1
    return max(atomic, ordered)


GAIN_SETS = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (7.5, 0.5, 1.5))


def terms_k(nc, BA):
    """Largest number of f32 additions a term of loss_terms_kernel<false> passes through, from the kernel's geometry:
      per lane and anchor  ceil(nc / 16) class terms (four per 16-byte round, one per tail trip: the same count), 4 DFL sides, 1 box
      grid-stride trips    ceil(ceil(BA / 16) / nb), nb = min(ceil(BA / 16), 2048) workgroups
      4 shuffles over the 16 lanes, the 16 `red` entries of the workgroup, then fold_depth(nb) between workgroups."""
    groups = -(-BA // 16)
    nb = min(groups, 2048)
    trips = -(-groups // nb)
    return max(-(-nc // 16), 4) * trips + 4 + 16 + fold_depth(nb)


def norm_k(BA):
    """loss_tal_norm_kernel: 6 shuffles over the wave, 3 adds over the 4 waves, then fold_depth(ceil(BA / 256)) between workgroups."""
    return 6 + 3 + fold_depth(-(-BA // 256))


def terms_extra(case):
    """name -> sum_bound(k, sum |terms|) for the three sums; every term is >= 0 (BCE, 1 - CIoU >= 0, cross-entropy), so the sum of
    the magnitudes is the float64 sum itself."""
    B, A = case["assign"].shape
    with torch.no_grad():
        s = terms([m.double() for m in case["maps"]], case["gt"], case["assign"], case["w"], case["strides"], torch.float64)
    k = terms_k(case["nc"], B * A)
    return {f"sum {n}": sum_bound(k, v.abs().item()) for n, v in zip(("box", "cls", "dfl"), s)}


ASSIGN_CASES = ("a21", "a189", "a189-zero", "a1029", "dense", "lds-50176", "lds-153600")


def assign_gt(name):
    """Section c inputs without the maps: -> hw, gt, strides, nc, B.
      a21         21 anchors, levels with fewer than TOPK anchors
      a189        two IDENTICAL gt rows (every overlap ties: the lower row wins each conflict), a gt with six anchors inside
      a189-zero   the same with every class logit at -200: all metrics zero, the ten lowest indices are picked
      a1029       five workgroup strides of 256 and a remainder
      dense       G = 12 overlapping gts on one 8 x 8 map
      lds-50176   one 112 x 112 level: the top-k buffer is past 48 KB;  lds-153600: 240 x 160, the largest accepted"""
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    if name == "a21":
        hw, st, nc, B = [(4, 4), (2, 2), (1, 1)], STRIDES, 3, 2
        gt = pad_gt([rand_boxes(3, 32, 32, gen, nc, 0.4, 0.9) for _ in range(B)])
    elif name.startswith("a189"):
        hw, st, nc, B = [(12, 12), (6, 6), (3, 3)], STRIDES, 4, 2
        twin = [1, 10.125, 20.25, 80.5, 70.125]
        gt = pad_gt([[twin, [0, 40.5, 40.5, 60.25, 58.125], list(twin)] + rand_boxes(2, 96, 96, gen, nc),
                     rand_boxes(4, 96, 96, gen, nc)])
    elif name == "a1029":
        hw, st, nc, B = [(28, 28), (14, 14), (7, 7)], STRIDES, 3, 1
        gt = pad_gt([rand_boxes(5, 224, 224, gen, nc)])
    elif name == "dense":
        hw, st, nc, B = [(8, 8)], STRIDES[:1], 2, 2
        gt = pad_gt([rand_boxes(12, 64, 64, gen, nc, 0.3, 0.8) for _ in range(B)])
    else:
        hw, st, nc, B = [{"lds-50176": (112, 112), "lds-153600": (240, 160)}[name]], STRIDES[:1], 1, 1
        gt = pad_gt([rand_boxes(2, 8 * hw[0][1], 8 * hw[0][0], gen, nc, 0.1, 0.3)])
    return hw, gt, st, nc, B


def assign_case(name):
    hw, gt, st, nc, B = assign_gt(name)
    maps = rand_maps(B, hw, nc, seed=sum(map(ord, name)) + 1)
    if name == "a189-zero":
        for m in maps:
            m[..., 4 * REG:] = -200.0
    return maps, gt, st, nc
