"""Link the boxes of one emission into tracks: the host side of ``csrc/link.hip``.

A scan reports one box per window (and, behind the filter bank, per band) per emission; an emission that lasts longer than a window
or is wider than a band comes back in pieces.  A TRACK is a connected component of the link relation on ``ScanResults.tf``
(float64 [t0_s, f_lo_hz, t1_s, f_hi_hz], the one coordinate system plain, resampled and channelised scans share).  With

    ov_t = min(t1_i, t1_j) - max(t0_i, t0_j)        dur = t1 - t0
    ov_f = min(fhi_i, fhi_j) - max(flo_i, flo_j)    bw  = f_hi - f_lo

rows i != j of one class (any classes: ``agnostic``) are linked when

    along time       ov_t >= -gap_t  and  ov_f >= align * min(bw_i, bw_j),    or
    along frequency  ov_f >= -gap_f  and  ov_t >= align * min(dur_i, dur_j)          (only when gap_f is not None)

all in float64.  The defaults — ``align`` = 0.5, ``gap_t`` = 8 STFT hops of the scanned rate, ``gap_f`` = 0 Hz behind a
filter bank whose neighbouring bands overlap (``oversample`` = 2) and None otherwise — are judgements, not measurements, like the seam
merge's 0.5.  ``ops.scan_link`` labels the rows on the device; the table of tracks is built there too (``unique``, ``scatter_reduce``
with ``amin`` / ``amax``: exact in float64) and comes back in one copy."""
from __future__ import annotations

import json
import math
import os

import numpy as np
import torch

DEFAULT_HOP = 256                                              # the hop of the default transform (SpectrogramProducer)
GAP_HOPS = 8                                                   # gap_t="auto": this many hops of the scanned rate


class LinkPlan:
    """The resolved arguments of one linking: ``gap_t`` seconds, ``gap_f`` Hz or None, ``align``, ``agnostic``."""

    def __init__(self, gap_t, gap_f, align, agnostic):
        self.gap_t, self.gap_f, self.align, self.agnostic = gap_t, gap_f, align, agnostic

    def __repr__(self):
        return f"LinkPlan(gap_t={self.gap_t!r}, gap_f={self.gap_f!r}, align={self.align!r}, agnostic={self.agnostic!r})"


def check_link_args(gap_t="auto", gap_f="auto", align=0.5, agnostic=False, hop=None):
    """The argument errors of ``plan_link`` that need no results (``scan(link=...)`` raises them before it scans)."""
    for name, v in (("gap_t", gap_t), ("gap_f", gap_f)):
        if isinstance(v, str):
            if v != "auto":
                raise ValueError(f"plan_link: {name} takes a number or 'auto', got {v!r}")
        elif v is None:
            if name == "gap_t":
                raise ValueError("plan_link: gap_t takes seconds or 'auto', got None")
        elif isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v) or v < 0:
            raise ValueError(f"plan_link: {name} must be finite and >= 0, got {v!r}")
    if isinstance(align, bool) or not isinstance(align, (int, float, np.integer, np.floating)) or not 0 < align <= 1:
        raise ValueError(f"plan_link: align must lie in (0, 1], got {align!r}")
    if hop is not None and (isinstance(hop, bool) or not isinstance(hop, (int, np.integer)) or hop <= 0):
        raise ValueError(f"plan_link: hop must be a positive integer, got {hop!r}")


def _host(a, dtype):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=dtype)


def plan_link(results, gap_t="auto", gap_f="auto", align=0.5, agnostic=False, hop=None):
    """The ``LinkPlan`` for ``results`` (a ``ScanResults``).  ``gap_t`` = "auto": ``8 * hop / results.sample_rate`` seconds — the rate the
    model saw, so the DDC's output rate or the bands' rate after a resampled or channelised scan; ``hop`` defaults to the one the scan
    recorded, else 256.  ``gap_f`` = "auto": 0.0 Hz when ``results.channelizer`` has ``oversample`` 2 (neighbouring bands overlap, so
    the pieces of a cut emission overlap in Hz), None (no linking along frequency) for ``oversample`` 1 and for every other scan; a
    number is allowed for any scan.  The defaults are judgements, not measurements.  Every argument error is a ``ValueError`` raised
    here, before anything touches the device: non-finite or inverted rectangles, negative or non-finite gaps, ``align`` outside
    (0, 1]."""
    check_link_args(gap_t, gap_f, align, agnostic, hop)
    tf = _host(results.tf, np.float64).reshape(-1, 4)
    if not np.isfinite(tf).all():
        raise ValueError(f"plan_link: row {int(np.flatnonzero(~np.isfinite(tf).all(1))[0])} of tf is not finite")
    bad = (tf[:, 2] < tf[:, 0]) | (tf[:, 3] < tf[:, 1])
    if bad.any():
        raise ValueError(f"plan_link: row {int(np.flatnonzero(bad)[0])} of tf is inverted (t1 < t0 or f_hi < f_lo)")
    if isinstance(gap_t, str):
        fs = float(results.sample_rate)
        if not (math.isfinite(fs) and fs > 0):
            raise ValueError(f"plan_link: gap_t='auto' needs a positive results.sample_rate, got {results.sample_rate!r}")
        gap_t = GAP_HOPS * int(hop or getattr(results, "hop", None) or DEFAULT_HOP) / fs
    if isinstance(gap_f, str):
        ch = getattr(results, "channelizer", None)
        gap_f = 0.0 if ch is not None and int(ch.oversample) == 2 else None
    return LinkPlan(float(gap_t), None if gap_f is None else float(gap_f), float(align), bool(agnostic))


class Tracks:
    """The tracks of one linked scan.  ``track`` (n,) int64: dense id 0 .. T-1 per row of the scan, tracks numbered by their first row;
    per track ``tf`` (T, 4) float64 the union rectangle [t0_s, f_lo_hz, t1_s, f_hi_hz], ``conf`` (T,) float64 the maximum over the
    members, ``cls`` (T,) int64 the class of the best-scored member (ties: the lowest row), ``count`` (T,) int64 the number of member
    rows and ``first_row`` (T,) int64 the lowest; ``rows(k)`` the member rows of track k, ascending.  ``boxes`` (T, 6) float64 holds
    NaN in columns 0-3 (a track has no strip / image-row box), ``conf`` in 4 and ``cls`` in 5: with ``tf`` and ``names`` that is all
    ``extract`` reads, so ``YOLO.extract(source, tracks, ...)`` cuts one clip per track.  ``plan`` is the ``LinkPlan`` used."""

    def __init__(self, track, tf, conf, cls, count, first_row, names=None, plan=None):
        self.track, self.tf, self.conf, self.cls, self.count, self.first_row = track, tf, conf, cls, count, first_row
        self.names, self.plan = names, plan
        self._order = torch.sort(track, stable=True)[1]        # rows grouped by track, ascending inside one
        self._offset = torch.cat((torch.zeros(1, dtype=torch.int64), torch.cumsum(count, 0)))

    def __len__(self):
        return self.tf.shape[0]

    @property
    def boxes(self):
        b = torch.full((len(self), 6), float("nan"), dtype=torch.float64)
        b[:, 4], b[:, 5] = self.conf, self.cls.to(torch.float64)
        return b

    def rows(self, k):
        k = int(k)
        if not 0 <= k < len(self):
            raise IndexError(f"track {k} of {len(self)}")
        return self._order[int(self._offset[k]):int(self._offset[k + 1])]

    def save(self, path):
        """One JSON file: the ``LinkPlan`` and, per track, rectangle, class, name, confidence, count and member rows.  -> the path."""
        path = os.fspath(path)
        tracks = []
        for k in range(len(self)):
            c = int(self.cls[k])
            tracks.append({"track": k, "tf": [float(v) for v in self.tf[k]], "class": c, "name": self.names.get(c) if self.names else None,
                           "confidence": float(self.conf[k]), "count": int(self.count[k]), "rows": [int(r) for r in self.rows(k)]})
        p = self.plan
        plan = None if p is None else {"gap_t": p.gap_t, "gap_f": p.gap_f, "align": p.align, "agnostic": p.agnostic}
        with open(path, "w") as f:
            json.dump({"link": plan, "rows": int(self.track.shape[0]), "tracks": tracks}, f, indent=1)
        return path


def build_tracks(tf, conf, cls, label, names=None, plan=None):
    """The ``Tracks`` of labelled rows: ``tf`` (n, 4) float64, ``conf`` (n,) float64, ``cls`` (n,) int64 and ``label`` (n,) int64 — any
    labelling that is constant on a track and differs between tracks — all on one device (the GPU in ``link_results``; the CPU works
    the same).  min / max / equality only: exact in float64."""
    n, dev = label.shape[0], label.device
    row = torch.arange(n, dtype=torch.int64, device=dev)
    if n == 0:
        z = torch.zeros((0,), dtype=torch.int64)
        return Tracks(z, torch.zeros((0, 4), dtype=torch.float64), torch.zeros((0,), dtype=torch.float64), z.clone(), z.clone(), z.clone(),
                      names, plan)
    _, dense = torch.unique(label, return_inverse=True)        # dense id per row, in label order
    T = int(dense.max()) + 1
    first = torch.full((T,), n, dtype=torch.int64, device=dev).scatter_reduce(0, dense, row, "amin")
    rank = torch.empty((T,), dtype=torch.int64, device=dev)
    rank[torch.sort(first)[1]] = torch.arange(T, dtype=torch.int64, device=dev)
    track = rank[dense]                                        # numbered by first row
    first = torch.sort(first)[0]
    lo = torch.full((T, 2), float("inf"), dtype=torch.float64, device=dev).scatter_reduce(0, track[:, None].expand(n, 2), tf[:, 0:2], "amin")
    hi = torch.full((T, 2), float("-inf"), dtype=torch.float64, device=dev).scatter_reduce(0, track[:, None].expand(n, 2), tf[:, 2:4], "amax")
    best = torch.full((T,), float("-inf"), dtype=torch.float64, device=dev).scatter_reduce(0, track, conf, "amax")
    at = torch.where(conf == best[track], row, torch.full_like(row, n))
    best_row = torch.full((T,), n, dtype=torch.int64, device=dev).scatter_reduce(0, track, at, "amin")
    count = torch.bincount(track, minlength=T)
    out = [t.cpu() for t in (track, torch.cat((lo, hi), 1), best, cls[best_row], count, first)]
    return Tracks(*out, names, plan)


def link_results(results, device="cuda", gap_t="auto", gap_f="auto", align=0.5, agnostic=False, hop=None):
    """``plan_link`` -> upload ``tf`` and the classes -> ``ops.scan_link`` -> ``build_tracks`` on the device -> ``Tracks`` (one copy back).
    An empty ``results`` gives an empty ``Tracks`` with no launch."""
    from .. import ops
    plan = plan_link(results, gap_t, gap_f, align, agnostic, hop)
    names = getattr(results, "names", None)
    n = len(results)
    empty = torch.zeros((0,), dtype=torch.int64)
    if n == 0:
        return build_tracks(torch.zeros((0, 4), dtype=torch.float64), torch.zeros((0,), dtype=torch.float64), empty, empty, names, plan)
    device = torch.device(device)
    boxes = torch.as_tensor(results.boxes)
    tf = torch.as_tensor(results.tf).to(torch.float64).reshape(-1, 4).to(device)
    conf = boxes[:, 4].to(torch.float64).to(device)
    cls = boxes[:, 5].to(torch.int64).to(device)
    label = ops.scan_link(tf, cls, plan.gap_t, plan.gap_f, plan.align, plan.agnostic)
    return build_tracks(tf, conf, cls, label, names, plan)
