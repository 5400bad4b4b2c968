"""GPU: the batched suppression entries of csrc/detect.hip (`nms_sorted_batched`, `nms_sorted_segments`, `nms_candidates`) and
`bias_grad_cast` of csrc/elementwise.hip, each called directly.

Suppression is compared bit for bit with `oracle/nms_ref.py:nms_core` (float32 IoU, strict `>`), candidate selection with a
plain numpy restatement of `oracle/nms_ref.py:pre_nms` (strict `>` on the class scores, first maximum wins), on inputs built so
that the edges occur: box centres on a coarse grid with three sizes (many IoU ties, IoU exactly at the threshold), scores and
thresholds on a 1/64 grid (scores equal to the threshold), empty images first, in the middle and last.
"""
import numpy as np
import pytest
import torch

from oracle import nms_ref
from tests._kernel_ref import DEV, Bars, ops, rnd, sum_bound

pytestmark = pytest.mark.gpu
IOU = 0.5


def grid_boxes(n, seed, cells=24):
    """n boxes (x1, y1, x2, y2), centres on a `cells`^2 grid of step 8, square sides from {24, 32, 48}; scores on a 1/64 grid,
    sorted by (score descending, index ascending).  Two equal boxes of side 24 one step apart have IoU (16 * 24) / (2 * 576 - 384) = 0.5."""
    g = torch.Generator().manual_seed(seed)
    c = torch.randint(0, cells, (n, 2), generator=g).float() * 8
    half = torch.tensor([12.0, 16.0, 24.0])[torch.randint(0, 3, (n,), generator=g)][:, None]
    boxes = torch.cat((c - half, c + half), 1)
    scores = torch.randint(1, 64, (n,), generator=g).float() / 64
    order = torch.sort(scores, descending=True, stable=True)[1]
    return boxes[order].contiguous(), scores[order].contiguous()


def iou_f32(b):
    """Pairwise IoU in float32 with nms_core's operation order."""
    b = b.numpy().astype(np.float32)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    w = np.maximum(np.float32(0), np.minimum(b[:, None, 2], b[None, :, 2]) - np.maximum(b[:, None, 0], b[None, :, 0]))
    h = np.maximum(np.float32(0), np.minimum(b[:, None, 3], b[None, :, 3]) - np.maximum(b[:, None, 1], b[None, :, 1]))
    inter = w * h
    return inter / (area[:, None] + area[None, :] - inter)


def ref_keep(boxes, scores, max_keep):
    k = nms_ref.nms_core(boxes.numpy(), scores.numpy(), IOU)[:max_keep]
    m = np.zeros(boxes.shape[0], dtype=bool)
    m[k] = True
    return m


def test_inputs_hit_the_threshold_exactly():
    """CPU part: the seeded boxes contain pairs with IoU == threshold in f32 (and such a pair decides a keep: strict `>`)."""
    boxes, scores = grid_boxes(700, seed=5)
    iou = iou_f32(boxes)
    at = np.argwhere(np.triu(iou == np.float32(IOU), 1))
    assert len(at) >= 1, "no pair with IoU == threshold: change the seed"
    assert (np.triu((iou > 0.45) & (iou < 0.55), 1).sum()) > len(at), "ties only"


COUNTS = [[0, 1, 64, 65, 0, 700, 3000, 0], [5], [0, 0, 129, 0], [(i * 37) % 71 if i % 5 else 0 for i in range(131)]]       # 131 images: > 128 per launch


@pytest.mark.parametrize("max_keep", [1, 5, 300])
@pytest.mark.parametrize("counts", COUNTS, ids=["mixed8", "one", "empties", "131images"])
def test_nms_sorted_batched(counts, max_keep):
    per = [grid_boxes(c, seed=5 + i) for i, c in enumerate(counts)]
    assert any((iou_f32(b) == np.float32(IOU))[np.triu_indices(b.shape[0], 1)].any() for b, _ in per if b.shape[0] > 1) or sum(counts) < 50, \
        "no pair with IoU == threshold in this input: change the seed"
    boxes = torch.cat([b for b, _ in per]).to(DEV)
    ref = np.concatenate([ref_keep(b, s, max_keep) for b, s in per])
    need = [c * ((c + 63) // 64) * 8 for c in counts]
    got = {}
    for chunk in (2 << 30, 1, max(need[:4]) + 8 if len(need) > 3 else 8, sum(need) // 2 + 8):
        # 1: one launch per image, every empty image a chunk of its own; the others put chunk boundaries elsewhere
        got[chunk] = ops().nms_sorted_batched(boxes, counts, IOU, max_keep, chunk_bytes=chunk).cpu().numpy()
        assert got[chunk].dtype == np.bool_ and got[chunk].shape == ref.shape
        bad = np.flatnonzero(got[chunk] != ref)
        assert bad.size == 0, f"chunk_bytes={chunk}: keep differs at rows {bad[:10]} (of {bad.size})"
    row = 0
    for c in counts:
        assert got[1][row:row + c].sum() <= max_keep
        row += c


@pytest.mark.parametrize("max_keep", [1, 5, 300])
@pytest.mark.parametrize("layout", ["image*nc+class", "nseg>>rows", "one"])
def test_nms_sorted_segments(layout, max_keep):
    if layout == "image*nc+class":
        nc, counts = 6, [0, 1, 64, 65, 0, 700] + [0] * 6 + [3, 0, 0, 129, 0, 1500] + [0] * 5 + [2]        # 4 images x 6 classes
    elif layout == "nseg>>rows":
        counts = [0] * 1000
        for s, c in ((0, 3), (17, 20), (500, 1), (998, 26)):
            counts[s] = c
    else:
        counts = [300]
    per = [grid_boxes(c, seed=40 + i) for i, c in enumerate(counts)]
    boxes = torch.cat([b for b, _ in per]).to(DEV)
    seg = torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts)).to(DEV)
    ref = np.concatenate([ref_keep(b, s, max_keep) for b, s in per])
    got = ops().nms_sorted_segments(boxes, seg, len(counts), IOU, max_keep).cpu().numpy()
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, f"keep differs at rows {bad[:10]} (of {bad.size})"
    same = ops().nms_sorted_batched(boxes, counts, IOU, max_keep).cpu().numpy()
    assert np.array_equal(same, got)


# ------------------------------------------------------------------------------------------------ nms_candidates
def ref_candidates(pred, nc, thr, multi):
    """(image, anchor, class) order; strict `>`; best-class branch: first maximum (np.argmax), as pre_nms."""
    thr = np.float32(thr)
    img, anc, cls, sc, per = [], [], [], [], []
    for b in range(pred.shape[0]):
        s = pred[b, 4:4 + nc].T                                   # (A, nc)
        if multi and nc > 1:
            a, c = np.nonzero(s > thr)                            # row-major: anchor, then class
        else:
            c = np.argmax(s, 1)
            a = np.flatnonzero(s[np.arange(s.shape[0]), c] > thr)
            c = c[a]
        img.append(np.full(a.shape, b)); anc.append(a); cls.append(c); sc.append(s[a, c]); per.append(len(a))
    return np.concatenate(img), np.concatenate(anc), np.concatenate(cls), np.concatenate(sc).astype(np.float32), per


def make_pred(B, nc, A, extra, seed):
    g = torch.Generator().manual_seed(seed)
    pred = torch.rand(B, 4 + nc + extra, A, generator=g)
    pred[:, 4:4 + nc] = torch.randint(0, 33, (B, nc, A), generator=g).float() / 64          # scores k / 64 <= 0.5: many equal 0.25
    pred[:, 4 + nc:] = 0.9                                                               # mask coefficients: never candidates
    if B > 1:
        pred[B // 2, 4:4 + nc] = 0.25                                                    # an image with every score AT the threshold
    return pred.contiguous()


@pytest.mark.parametrize("multi", [False, True], ids=["best", "multi"])
@pytest.mark.parametrize("nc", [1, 6, 80])
@pytest.mark.parametrize("A", [1, 255, 256, 257, 8400])
def test_nms_candidates(A, nc, multi):
    thr, B = 0.25, 3
    pred = make_pred(B, nc, A, extra=3 if nc == 6 else 0, seed=A + nc)
    p = pred.numpy()
    assert (p[:, 4:4 + nc] == np.float32(thr)).any(), "no score equals the threshold"
    img, anc, cls, sc, per = ref_candidates(p, nc, thr, multi)
    assert per[B // 2] == 0, "the all-at-threshold image must have no candidate"
    if multi and nc > 1:
        rows = [nms_ref.pre_nms(pred[b].T, nc, thr, True, max_nms=10 ** 9).shape[0] for b in range(B)]
        assert rows == per, "the restatement disagrees with oracle pre_nms"
    pred_d = pred.to(DEV)
    for by_class, cap in ((False, None), (True, None), (True, max(max(per) - 1, 0))):
        key, a_d, c_d, per_d, seg_cls = ops().nms_candidates(pred_d, nc, thr, multi, segment_by_class=by_class, max_per_image=cap)
        assert per_d == per, (per_d, per)
        assert seg_cls == (by_class and (cap is None or max(per) <= cap))
        key = key.cpu().numpy()
        assert np.array_equal(a_d.cpu().numpy(), anc) and np.array_equal(c_d.cpu().numpy(), cls)
        bits = (~(key & 0xFFFFFFFF)) & 0xFFFFFFFF
        assert np.array_equal(bits.astype(np.uint32).view(np.float32), sc), "decoded score differs"
        assert np.array_equal(key >> 32, img * nc + cls if seg_cls else img), "segment id differs"


def test_nms_candidates_no_candidate_at_all():
    pred = make_pred(2, 6, 300, 0, seed=1)
    key, a, c, per, _ = ops().nms_candidates(pred.to(DEV), 6, 0.5, True)               # scores <= 0.5, strict >
    assert per == [0, 0] and key.numel() == 0 and a.numel() == 0 and c.numel() == 0


# ------------------------------------------------------------------------------------------------ bias_grad_cast
@pytest.mark.parametrize("mode", ["atomic", "partials"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=["f16", "bf16", "f32"])
@pytest.mark.parametrize("pad", ["N", "next8", "256"])
@pytest.mark.parametrize("N", [1, 5, 64, 144])
@pytest.mark.parametrize("shape,strided", [((1, 1, 1), False), ((2, 7, 9), True), ((3, 20, 20), True), ((2, 80, 80), False), ((1, 130, 131), True)],
                         ids=["1x1x1", "2x7x9-slice", "3x20x20-slice", "2x80x80", "1x130x131-slice"])
def test_bias_grad_cast(shape, strided, N, pad, dtype, mode):
    """dy is dz rounded to the dtype bit for bit, pad channels exactly zero; dbias (accumulated into a non-zero vector) against
    float64 column sums; `partials` = None adds the workgroup sums atomically, else they go through the fixed-order fold."""
    B, H, W = shape
    npad = {"N": N, "next8": -(-N // 8) * 8, "256": 256}[pad]
    dz = rnd(B, H, W, N, seed=N + H, scale=4.0)
    if strided:                                                    # N columns out of a wider f32 buffer (ld = N + 8, offset 4: stays 16-byte aligned)
        wide = torch.full((B, H, W, N + 8), 1.0e3, device=DEV)
        dz_d = wide[..., 4:4 + N]
        dz_d.copy_(dz.to(DEV))
    else:
        dz_d = dz.to(DEV)
    dy = torch.full((B, H, W, npad), 7.0, dtype=dtype, device=DEV)
    db0 = rnd(N, seed=3, scale=10.0)
    db = db0.to(DEV)
    partials = torch.full((512, N), -5.0, device=DEV) if mode == "partials" else None
    ops().bias_grad_cast(dz_d, dy, db, partials)
    torch.cuda.synchronize()
    want = torch.zeros(B, H, W, npad, dtype=dtype)
    want[..., :N] = dz.to(dtype)
    iv = {2: torch.int16, 4: torch.int32}[want.element_size()]
    assert torch.equal(dy.cpu().view(iv), want.view(iv)), "dy is not dz rounded to the dtype with zero pad channels"
    b = Bars(f"bias_grad_cast[{mode}] {B}x{H}x{W} N{N} npad{npad} {dtype}")
    # a channel's sum: a thread takes every `groups`-th row of its workgroup's run, the row groups are folded, the workgroups'
    # partials are added (atomically or by the fold kernel); signed terms, so the bound is on sum|dz| and not on the result
    M = B * H * W
    v4 = N % 4 == 0 and npad % 4 == 0 and dz_d.stride(2) % 4 == 0
    groups = 256 // (npad // 4 if v4 else npad)
    blocks = min(512, -(-M // 256))
    depth = -(-(-(-M // blocks)) // groups) + groups + blocks
    b.add("dbias(+db0)", db, db0.double() + dz.double().sum((0, 1, 2)), db0 + dz.sum((0, 1, 2)),
          extra=sum_bound(depth, dz.double().abs().sum((0, 1, 2)).max() + db0.abs().max()))
    b.check()
