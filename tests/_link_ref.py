"""TEST HELPERS for linking a scan's rows into tracks: a float64 numpy reference written independently of ``sy11``.

``linked`` is the relation of DESIGN.md §4 between one row and an array of rows; ``link_ref`` is union-find over a sweep by t0 (a row is
compared with the later rows whose t0 is not beyond ``t1 + gap_t``, widened by a generous slack; the predicate alone decides) and
``link_brute`` the all-pairs version it is pinned to on small inputs.  Both return, per row, the smallest row index of its component.
``tracks_ref`` builds the table of tracks from such labels; ``survivor_tf`` turns a survivor list of tests/_scan_ref.py into the
seconds / Hz rectangles a scan would report for it."""
from __future__ import annotations

import numpy as np


def linked(r, rows, c, cls, gap_t, gap_f, align, agnostic):
    """r (4,), rows (m, 4) float64 [t0, f_lo, t1, f_hi]; c, cls (m,) classes -> (m,) bool."""
    ov_t = np.minimum(r[2], rows[:, 2]) - np.maximum(r[0], rows[:, 0])
    ov_f = np.minimum(r[3], rows[:, 3]) - np.maximum(r[1], rows[:, 1])
    bw = np.minimum(r[3] - r[1], rows[:, 3] - rows[:, 1])
    hit = (ov_t >= -gap_t) & (ov_f >= align * bw)
    if gap_f is not None:
        dur = np.minimum(r[2] - r[0], rows[:, 2] - rows[:, 0])
        hit |= (ov_f >= -gap_f) & (ov_t >= align * dur)
    return hit if agnostic else hit & (cls == c)


def _find(parent, i):
    root = i
    while parent[root] != root:
        root = parent[root]
    while parent[i] != root:
        parent[i], i = root, parent[i]
    return root


def _labels(parent):
    n = len(parent)
    root = np.array([_find(parent, i) for i in range(n)], dtype=np.int64)
    first = np.full(n, n, dtype=np.int64)
    np.minimum.at(first, root, np.arange(n, dtype=np.int64))
    return first[root]


def link_ref(tf, cls, gap_t, gap_f=None, align=0.5, agnostic=False):
    """-> (n,) int64: the smallest row index of every row's component.  float64, union-find over a sweep by t0."""
    tf = np.asarray(tf, dtype=np.float64).reshape(-1, 4)
    cls = np.asarray(cls, dtype=np.int64)
    n = tf.shape[0]
    order = np.argsort(tf[:, 0], kind="stable")
    s, sc = tf[order], cls[order]
    t0 = s[:, 0]
    bound = s[:, 2] + gap_t
    bound = bound + 1e-9 * (np.abs(bound) + 1.0)               # far more than the one rounding of ov_t; only the predicate decides
    end = np.searchsorted(t0, bound, side="right")
    parent = list(range(n))
    for k in range(n):
        if end[k] <= k + 1:
            continue
        for j in np.flatnonzero(linked(s[k], s[k + 1:end[k]], sc[k], sc[k + 1:end[k]], gap_t, gap_f, align, agnostic)) + k + 1:
            a, b = _find(parent, k), _find(parent, int(j))
            if a != b:
                parent[max(a, b)] = min(a, b)
    lab = np.empty(n, dtype=np.int64)
    lab[order] = _labels(parent)                               # components, named by a sorted position
    first = np.full(n, n, dtype=np.int64)
    np.minimum.at(first, lab, np.arange(n, dtype=np.int64))
    return first[lab]


def link_brute(tf, cls, gap_t, gap_f=None, align=0.5, agnostic=False):
    """The same labels from all n (n - 1) / 2 pairs."""
    tf = np.asarray(tf, dtype=np.float64).reshape(-1, 4)
    cls = np.asarray(cls, dtype=np.int64)
    n = tf.shape[0]
    parent = list(range(n))
    for i in range(n):
        hit = linked(tf[i], tf, cls[i], cls, gap_t, gap_f, align, agnostic)
        hit[i] = False
        for j in np.flatnonzero(hit):
            a, b = _find(parent, i), _find(parent, int(j))
            if a != b:
                parent[max(a, b)] = min(a, b)
    return _labels(parent)


def tracks_ref(tf, conf, cls, label):
    """-> dict of numpy arrays: track (n,), tf (T, 4), conf, cls, count, first_row (T,), rows (list of T arrays); tracks numbered by
    their first row, cls that of the best-scored member (ties: the lowest row)."""
    tf = np.asarray(tf, dtype=np.float64).reshape(-1, 4)
    conf, cls, label = np.asarray(conf, dtype=np.float64), np.asarray(cls, dtype=np.int64), np.asarray(label, dtype=np.int64)
    groups = {}
    for i, l in enumerate(label.tolist()):
        groups.setdefault(l, []).append(i)
    members = sorted(groups.values(), key=lambda m: m[0])
    track = np.zeros(len(label), dtype=np.int64)
    out = {"tf": np.zeros((len(members), 4)), "conf": np.zeros(len(members)), "cls": np.zeros(len(members), np.int64),
           "count": np.zeros(len(members), np.int64), "first_row": np.zeros(len(members), np.int64), "rows": []}
    for k, m in enumerate(members):
        m = np.array(m, dtype=np.int64)
        track[m] = k
        out["tf"][k] = [tf[m, 0].min(), tf[m, 1].min(), tf[m, 2].max(), tf[m, 3].max()]
        out["conf"][k] = conf[m].max()
        out["cls"][k] = cls[m[np.argmax(conf[m])]]             # argmax returns the first maximum: the lowest row
        out["count"][k], out["first_row"][k] = len(m), m[0]
        out["rows"].append(m)
    out["track"] = track
    return out


def survivor_tf(window, boxes, start, fs=20e6, fc=2.4e9, hop=256, n_mel=640):
    """A survivor list of tests/_scan_ref.py -> (n, 4) float64 [t0_s, f_lo_hz, t1_s, f_hi_hz]: strip frames to seconds at ``hop / fs``
    per frame, image rows to Hz on a linear axis over ``fs`` around ``fc`` (a stand-in for the producer's warped axis: any monotone
    map serves the relation)."""
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    off = np.asarray(start, dtype=np.int64)[np.asarray(window, dtype=np.int64)].astype(np.float64)
    t0, t1 = (b[:, 0] + off) * hop / fs, (b[:, 2] + off) * hop / fs
    f0, f1 = fc - fs / 2 + b[:, 1] * (fs / n_mel), fc - fs / 2 + b[:, 3] * (fs / n_mel)
    return np.stack((t0, f0, t1, f1), 1)
