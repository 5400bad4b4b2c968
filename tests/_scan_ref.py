"""TEST HELPERS for the long-capture scan: a float64 reference of the seam merge, a generator of well-separated survivor
lists, and a capture whose contents differ in every window.

``merge_ref`` is greedy suppression in STRIP coordinates (X = start[window] + x) in the order and with the strict ``>`` of
``oracle.nms_ref.nms_core``: boxes are visited by (score descending, input index ascending); a box is kept unless an
already-kept box of its class (any class when ``agnostic``) has ``metric > thres`` with it; ``metric`` is
``iou = inter / (a_i + a_j - inter)`` or ``ios = inter / min(a_i, a_j)``.  All arithmetic is float64.  The pair list is
built window by window (two boxes can only intersect when their windows start less than ``n_frames`` apart), which is
what makes W = 4 000 affordable; the visit itself is the plain greedy loop."""
from __future__ import annotations

import numpy as np


def _pair_metrics(bi, bj, metric):
    """(a, 4) x (b, 4) float64 strip boxes -> (a, b) metric matrix (nan where it is 0 / 0)."""
    iw = np.maximum(0.0, np.minimum(bi[:, None, 2], bj[None, :, 2]) - np.maximum(bi[:, None, 0], bj[None, :, 0]))
    ih = np.maximum(0.0, np.minimum(bi[:, None, 3], bj[None, :, 3]) - np.maximum(bi[:, None, 1], bj[None, :, 1]))
    inter = iw * ih
    ai = ((bi[:, 2] - bi[:, 0]) * (bi[:, 3] - bi[:, 1]))[:, None]
    aj = ((bj[:, 2] - bj[:, 0]) * (bj[:, 3] - bj[:, 1]))[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        return inter / np.minimum(ai, aj) if metric == "ios" else inter / (ai + aj - inter)


def strip_boxes(window, boxes, start):
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 4).copy()
    off = np.asarray(start, dtype=np.int64)[np.asarray(window, dtype=np.int64)].astype(np.float64)
    b[:, 0] += off
    b[:, 2] += off
    return b


def _neighbour_pairs(window, boxes, score, cls, start, n_frames, metric, agnostic):
    """Yield (rows_i, rows_j, metric matrix, same-class mask, j-outranks-i mask) per window, j over the rows of every window
    whose start is less than n_frames away."""
    window = np.asarray(window, dtype=np.int64)
    start = np.asarray(start, dtype=np.int64)
    score = np.asarray(score, dtype=np.float64)
    cls = np.asarray(cls, dtype=np.int64)
    sb = strip_boxes(window, boxes, start)
    order = np.argsort(window, kind="stable")
    bounds = np.searchsorted(window[order], np.arange(start.size + 1))
    by_start = np.argsort(start, kind="stable")
    sorted_start = start[by_start]
    for w in range(start.size):
        ri = order[bounds[w]:bounds[w + 1]]
        if ri.size == 0:
            continue
        lo = np.searchsorted(sorted_start, start[w] - n_frames, side="right")
        hi = np.searchsorted(sorted_start, start[w] + n_frames, side="left")
        rj = np.concatenate([order[bounds[v]:bounds[v + 1]] for v in by_start[lo:hi]])
        m = _pair_metrics(sb[ri], sb[rj], metric)
        same = np.ones(m.shape, dtype=bool) if agnostic else cls[ri][:, None] == cls[rj][None, :]
        better = (score[rj][None, :] > score[ri][:, None]) | ((score[rj][None, :] == score[ri][:, None]) & (rj[None, :] < ri[:, None]))
        yield ri, rj, m, same, better


def merge_ref(window, boxes, score, cls, start, n_frames, metric="ios", thres=0.5, agnostic=False):
    """-> bool keep mask (n,), float64 greedy suppression in strip coordinates."""
    n = len(window)
    keep = np.zeros(n, dtype=bool)
    if n == 0:
        return keep
    thres = float(thres)
    partners = [None] * n
    for ri, rj, m, same, better in _neighbour_pairs(window, boxes, score, cls, start, n_frames, metric, agnostic):
        hit = (m > thres) & same & better
        for a, i in enumerate(ri):
            partners[i] = rj[hit[a]]
    score = np.asarray(score, dtype=np.float64)
    for i in np.lexsort((np.arange(n), -score)):               # score descending, then input index ascending
        p = partners[i]
        keep[i] = p is None or not keep[p].any()
    return keep


def near_threshold_rows(window, boxes, score, cls, start, n_frames, metric, thres, agnostic, margin=1e-4):
    """Rows that take part in a pair able to decide anything (same class, or all when agnostic) whose float64 metric lies
    within ``margin`` of the threshold."""
    bad = []
    for ri, rj, m, same, _ in _neighbour_pairs(window, boxes, score, cls, start, n_frames, metric, agnostic):
        close = (np.abs(m - float(thres)) <= margin) & same & np.isfinite(m)
        close[ri[:, None] == rj[None, :]] = False                    # a box against itself decides nothing
        bad.append(ri[close.any(1)])
    return np.unique(np.concatenate(bad)) if bad else np.zeros(0, np.int64)


def counts_for(rng, W, max_per_window=300):
    """Boxes per window, never more than ``max_per_window`` (the predictor's max_det).  One or two windows: uniform in
    [0, max] with one window exactly full.  More: a scan's usual picture — most windows hold a handful of boxes, some are
    full (one in five of 50, one in fifty of 4 000) — which keeps the float64 reference of a 4 000-window list within
    seconds while empty, sparse and full windows all occur next to each other."""
    if W <= 2:
        c = rng.integers(0, max_per_window + 1, W)
        c[rng.integers(0, W)] = max_per_window
        return c
    c = rng.integers(0, 13, W)
    c[rng.random(W) < (0.2 if W <= 50 else 0.02)] = max_per_window
    return c


def _legal(rows, n_frames, n_mel):
    rows[:, [0, 2]] = np.clip(rows[:, [0, 2]], 0, n_frames)
    rows[:, [1, 3]] = np.clip(rows[:, [1, 3]], 0, n_mel)
    small_w, small_h = rows[:, 2] - rows[:, 0] < 2, rows[:, 3] - rows[:, 1] < 2
    rows[small_w, 0] = np.clip(rows[small_w, 2] - 2, 0, None)
    rows[small_w, 2] = rows[small_w, 0] + 2
    rows[small_h, 1] = np.clip(rows[small_h, 3] - 2, 0, None)
    rows[small_h, 3] = rows[small_h, 1] + 2
    return rows


def survivors(seed, W, stride, nc, metric, thres, agnostic, first_start=0, n_frames=640, n_mel=640, max_per_window=300):
    """A seeded survivor list -> (window int32, boxes f32 (n, 4), score f32, cls int32, start int64), at most
    ``max_per_window`` rows per window.  Emissions live in strip coordinates; every window that sees enough of one reports
    it cut to the window and jittered, so seams produce real twins (and whole boxes next to their edge-cut twins).
    Scores are distinct by construction (a permutation, checked after the cast to f32).  A list in which a deciding pair's
    float64 metric lies within 1e-4 of the threshold is rejected: the boxes of those pairs are redrawn (jittered anew) and
    the whole list is checked again, so the list that is returned has no such pair and NO case is excluded; fewer than 100
    redraws are needed (asserted)."""
    start = first_start + stride * np.arange(W, dtype=np.int64)
    rng = np.random.default_rng([seed, W, stride, nc])
    counts = counts_for(rng, W, max_per_window)
    cell_cache = {}

    def cell(c):
        if c not in cell_cache:
            g = np.random.default_rng([seed, 7, int(c)])
            m = int(g.integers(0, 40))
            x1 = c * 160 + g.uniform(0, 160, m)
            y1 = g.uniform(0, n_mel - 8, m)
            cell_cache[c] = np.stack((x1, y1, x1 + g.uniform(4, 400, m), np.minimum(y1 + g.uniform(4, 120, m), n_mel),
                                      g.integers(0, nc, m).astype(np.float64)), 1)
        return cell_cache[c]

    win, box, cl = [], [], []
    for w in range(W):
        k = int(counts[w])
        if k == 0:
            continue
        lo = int(start[w] - first_start)
        shared = np.concatenate([cell(c) for c in range(max(lo // 160 - 3, 0), (lo + n_frames) // 160 + 1)]).copy()
        shared[:, [0, 2]] -= lo                                      # window-local
        shared = shared[(np.minimum(shared[:, 2], n_frames) - np.maximum(shared[:, 0], 0)) >= 3]
        shared = shared[rng.permutation(shared.shape[0])[: k // 2]]
        shared[:, :4] += rng.uniform(-1.5, 1.5, (shared.shape[0], 4))
        m = k - shared.shape[0]
        x1 = rng.uniform(0, n_frames - 4, m)
        y1 = rng.uniform(0, n_mel - 4, m)
        own = np.stack((x1, y1, x1 + rng.uniform(3, 300, m), y1 + rng.uniform(3, 150, m), rng.integers(0, nc, m).astype(np.float64)), 1)
        rows = _legal(np.concatenate((shared, own)), n_frames, n_mel)
        win.append(np.full(rows.shape[0], w))
        box.append(rows[:, :4])
        cl.append(rows[:, 4])
    n = sum(len(x) for x in win)
    window = np.concatenate(win).astype(np.int32) if n else np.zeros(0, np.int32)
    boxes = np.concatenate(box).astype(np.float32) if n else np.zeros((0, 4), np.float32)
    cls = np.concatenate(cl).astype(np.int32) if n else np.zeros(0, np.int32)
    score = rng.permutation(n).astype(np.float64)
    score = (0.05 + 0.94 * (score + rng.uniform(0.25, 0.75, n)) / max(n, 1)).astype(np.float32)
    assert np.unique(score).size == n, "scores tie"
    for redraws in range(100):
        bad = near_threshold_rows(window, boxes, score, cls, start, n_frames, metric, thres, agnostic) if n else bad_none
        if bad.size == 0:
            assert window.size == 0 or np.bincount(window).max() <= max_per_window
            return window, boxes, score, cls, start
        again = boxes[bad].astype(np.float64) + rng.uniform(-1.5, 1.5, (bad.size, 4))
        boxes[bad] = _legal(again, n_frames, n_mel).astype(np.float32)
    raise AssertionError("the survivor generator needed 100 redraws for one list")


bad_none = np.zeros(0, np.int64)


def capture(n_windows=6.3, seed=11):
    """A seeded capture of about ``n_windows`` windows, complex64 tensor: noise plus the burst / chirp recipe of
    ``oracle.stft_ref.synthetic_iq`` laid down once per window length with per-window parameters, so that every window differs."""
    import math

    import torch

    from oracle import stft_ref as S
    n = int(S.N_SAMPLES * n_windows)
    g = torch.Generator().manual_seed(seed)
    out = ((torch.randn(n, generator=g) + 1j * torch.randn(n, generator=g)) / math.sqrt(2)).to(torch.complex64) * 0.1
    seg_len = S.N_FRAMES * S.HOP
    for b in range(n // seg_len + 1):
        o = b * seg_len
        t = torch.arange(min(seg_len, n - o), dtype=torch.float32)
        if t.numel() < 4096:
            break
        f0 = -0.3 + 0.6 * ((b * 37 + 11) % 64) / 64.0
        k = torch.arange(64, dtype=torch.float32)
        ph = torch.rand(64, generator=g) * 2 * math.pi
        freqs = f0 + (k - 32) * (0.08 / 64)
        t0, t1 = int(t.numel() * (0.1 + 0.05 * (b % 3))), int(t.numel() * (0.5 + 0.07 * (b % 4)))
        burst = torch.exp(1j * (2 * math.pi * freqs[:, None] * t[None, t0:t1] + ph[:, None])).sum(0) / 8.0
        out[o + t0:o + t1] += burst.to(torch.complex64)
        c0, c1 = -0.35 + 0.1 * (b % 5), 0.05 + 0.08 * (b % 4)
        tt = t[int(t.numel() * 0.6):]
        tt = tt - tt[0]
        phase = 2 * math.pi * (c0 * tt + 0.5 * (c1 - c0) / tt.numel() * tt * tt)
        out[o + int(t.numel() * 0.6):o + t.numel()] += (0.7 * torch.exp(1j * phase)).to(torch.complex64)
    return out
