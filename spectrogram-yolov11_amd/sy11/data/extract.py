"""Extract every detection of a scan as baseband IQ on the GPU: the host plan of ``csrc/extract.hip`` (mix -> low-pass -> decimate ->
cut in time, all clips of a staged span in ONE launch) and ``extract_capture``, which feeds it a capture chunk by chunk.

Definition.  A capture of ``n`` samples at ``fs`` Hz centred at ``fc`` and a detection ``[t0, f_lo, t1, f_hi]`` (seconds
of the capture, absolute Hz):

    band      B = (f_hi - f_lo)(1 + 2 pad_f) around the centre (f_lo + f_hi) / 2
    decimate  D = the largest power of two in {1 .. 64} with USABLE_BAND fs / D >= B (1 when none qualifies; ``decimate=`` overrides)
    filter    D >= 2: exactly ``resample.prototype(1, D)``, T = 32 D + 1 taps, centre c = 16 D;  D = 1: no filter (the one tap 1.0)
    mixer     dphi = round(-(centre - fc) / fs 2^32) mod 2^32; sample i is turned by (uint32)(i dphi), i the absolute sample index
    grid      output m sits on capture sample m D (anchored at sample 0): m_first = floor((t0 - pad_t) fs / D),
              m_last = ceil((t1 + pad_t) fs / D), both clipped to [0, (n - 1) // D], M = m_last - m_first + 1

    clip[m - m_first] = sum_{j < T} h_D[j] xm[m D + c - j],   xm = the mixed samples, zero outside the capture

which is, sample for sample and bit for bit, ``ops.iq_resample`` with ``plan_resample(fs, fs / D, centre_applied - fc)`` over the
outputs ``[m_first, m_first + M)``.  The clip starts at exactly ``m_first D / fs`` seconds, runs at ``fs / D`` Hz and is centred at the
frequency really applied (the step is a whole number of 2^-32 cycles per sample).  There is no filter state, so a clip cut into pieces
along ``m`` is bit-identical to one pass.
"""
from __future__ import annotations

import json
import math
import os

import numpy as np
import torch

from .resample import USABLE_BAND, ZERO_CROSSINGS, prototype

MAX_LOG2D = 6                                                  # D <= 64, as the DDC's MAX_RATIO
MAX_SAMPLES = 1 << 27                                          # packed complex64 samples of one extraction (1 GiB)
MIN_CHUNK = 63 * 64 + 2 * ZERO_CROSSINGS * 64 + 1              # the support of one 64-output tile at D = 64: 6081 samples

# one segment of a launch, laid out as sy11_iq_segment (include/sy11.h)
SEGMENT = np.dtype([("m0", "<i8"), ("out_off", "<i8"), ("M", "<i4"), ("log2d", "<i4"), ("dphi", "<u4"), ("reserved", "<i4")])


def taps_offset(log2d):
    """First float of the table of D = 2^log2d in the concatenated tap buffer (every table starts on a multiple of 4 floats)."""
    return 0 if log2d == 0 else (32 << log2d) - 64 + 4 * log2d


_TAPS, _TAPS_DEV = None, {}


def extract_taps():
    """-> float32 (4060,): the seven tables one after the other — [1.0] for D = 1, ``prototype(1, D)`` for D = 2 .. 64."""
    global _TAPS
    if _TAPS is None:
        t = np.zeros(taps_offset(MAX_LOG2D + 1), dtype=np.float32)
        t[0] = 1.0                                             # fmaf(1, v, 0) is exact; prototype(1, 1)'s 1e-17 side taps are not
        for l in range(1, MAX_LOG2D + 1):
            h, _ = prototype(1, 1 << l)
            t[taps_offset(l):taps_offset(l) + h.shape[0]] = h.astype(np.float32)
        _TAPS = t
    return _TAPS


def taps_on(device):
    """The tap buffer on ``device``, uploaded once per device (as ``ResamplePlan.taps_on``)."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if device not in _TAPS_DEV:
        _TAPS_DEV[device] = torch.from_numpy(extract_taps()).to(device)
    return _TAPS_DEV[device]


def support(m0, M, log2d, n):
    """Capture samples [a, b) that the outputs [m0, m0 + M) at D = 2^log2d read, clipped to the capture's n samples."""
    D = 1 << int(log2d)
    if log2d == 0:
        return int(m0), int(m0 + M)
    c = ZERO_CROSSINGS * D
    return max((int(m0) * D) - c, 0), min((int(m0) + int(M) - 1) * D + c + 1, int(n))


class ExtractPlan:
    """Per selected row of ``tf``: ``D`` / ``log2d``, ``dphi``, ``m_first``, ``M``, ``sample_rate`` (fs / D), ``center_freq`` (really applied),
    ``t0`` (seconds of the capture of the clip's first sample) and ``offset`` (k + 1 packed offsets; ``total`` = the last).  ``rows``
    are the rows of ``tf`` the clips belong to, ``tf`` their boxes; ``n`` / ``fs`` / ``fc`` describe the capture."""

    def __init__(self, n, fs, fc, rows, tf, D, dphi, m_first, M):
        self.n, self.fs, self.fc = int(n), float(fs), float(fc)
        self.rows, self.tf = rows, tf
        self.D, self.dphi, self.m_first, self.M = D, dphi, m_first, M
        self.log2d = np.round(np.log2(D)).astype(np.int32)
        signed = np.where(dphi >= 1 << 31, dphi - (1 << 32), dphi).astype(np.float64)
        self.center_freq = self.fc + (-signed / 2.0 ** 32 * self.fs)
        self.sample_rate = self.fs / D.astype(np.float64)
        self.t0 = (m_first * D).astype(np.float64) / self.fs
        self.offset = np.concatenate(([0], np.cumsum(M, dtype=np.int64))).astype(np.int64)
        self.total = int(self.offset[-1])

    def __len__(self):
        return self.rows.shape[0]

    def __repr__(self):
        return f"ExtractPlan({len(self)} clips, {self.total} samples, D in {sorted(set(self.D.tolist()))})"


def plan_extract(tf, n, sample_rate, center_freq=0.0, pad_t=0.0, pad_f=0.1, decimate="auto", rows=None, max_samples=MAX_SAMPLES):
    """The ``ExtractPlan`` of the boxes ``tf`` (k, 4) [t0_s, f_lo_hz, t1_s, f_hi_hz] (``ScanResults.tf``) on a capture of ``n`` samples at
    ``sample_rate`` Hz centred at ``center_freq`` — the capture's OWN rate and centre, whatever the scan put in front of the model.
    ``rows``: the rows to extract (default: all).  Every argument error is a ``ValueError`` raised here, before anything touches
    the device."""
    fs, fc, n = float(sample_rate), float(center_freq), int(n)
    if not (math.isfinite(fs) and fs > 0 and math.isfinite(fc)):
        raise ValueError(f"plan_extract: sample_rate must be positive and center_freq finite, got {sample_rate!r} / {center_freq!r}")
    if n <= 0:
        raise ValueError(f"plan_extract: the capture has {n} samples")
    pad_t, pad_f = float(pad_t), float(pad_f)
    if not (math.isfinite(pad_t) and pad_t >= 0 and math.isfinite(pad_f) and pad_f >= 0):
        raise ValueError(f"plan_extract: pad_t and pad_f must be finite and >= 0, got {pad_t!r} / {pad_f!r}")
    if isinstance(tf, torch.Tensor):
        tf = tf.detach().cpu().numpy()
    tf = np.asarray(tf, dtype=np.float64).reshape(-1, 4)
    if rows is None:
        rows = np.arange(tf.shape[0], dtype=np.int64)
    else:
        rows = np.asarray(rows).reshape(-1)
        if rows.size and not np.issubdtype(rows.dtype, np.integer):
            raise ValueError(f"plan_extract: rows must be integer indices, got {rows.dtype}")
        rows = rows.astype(np.int64)
        if rows.size and (rows.min() < 0 or rows.max() >= tf.shape[0]):
            raise ValueError(f"plan_extract: rows must index the {tf.shape[0]} boxes, got {int(rows.min())} .. {int(rows.max())}")
    if decimate != "auto":
        if isinstance(decimate, bool) or not isinstance(decimate, (int, np.integer)) or decimate < 1 or decimate > 1 << MAX_LOG2D \
                or decimate & (decimate - 1):
            raise ValueError(f"plan_extract: decimate must be 'auto' or a power of two <= {1 << MAX_LOG2D}, got {decimate!r}")
    box = tf[rows]
    if not np.isfinite(box).all():
        raise ValueError(f"plan_extract: box {int(rows[np.flatnonzero(~np.isfinite(box).all(1))[0]])} is not finite")
    bad = (box[:, 2] < box[:, 0]) | (box[:, 3] < box[:, 1])
    if bad.any():
        raise ValueError(f"plan_extract: box {int(rows[np.flatnonzero(bad)[0]])} is inverted (t1 < t0 or f_hi < f_lo)")
    centre = (box[:, 1] + box[:, 3]) / 2
    bad = np.abs(centre - fc) > fs / 2
    if bad.any():
        k = np.flatnonzero(bad)[0]
        raise ValueError(f"plan_extract: box {int(rows[k])} is centred at {centre[k]!r} Hz, outside the capture's {fc!r} +- {fs / 2!r} Hz")
    B = (box[:, 3] - box[:, 1]) * (1 + 2 * pad_f)
    if decimate == "auto":
        D = np.ones(box.shape[0], dtype=np.int64)
        for l in range(1, MAX_LOG2D + 1):                      # ascending: the largest D that qualifies stays
            D[USABLE_BAND * fs / (1 << l) >= B] = 1 << l
    else:
        D = np.full(box.shape[0], int(decimate), dtype=np.int64)
    dphi = np.array([int(round(-(c - fc) / fs * 2.0 ** 32)) % (1 << 32) for c in centre], dtype=np.int64)
    m_max = (n - 1) // D
    m_first = np.clip(np.floor((box[:, 0] - pad_t) * fs / D).astype(np.int64), 0, m_max)
    m_last = np.clip(np.ceil((box[:, 2] + pad_t) * fs / D).astype(np.int64), 0, m_max)
    M = m_last - m_first + 1
    total = int(M.sum())
    if total > int(max_samples):
        raise ValueError(f"plan_extract: the {box.shape[0]} clips hold {total} samples, above max_samples = {int(max_samples)}; "
                         f"extract fewer at a time with rows=")
    return ExtractPlan(n, fs, fc, rows, box, D, dphi, m_first, M)


class ExtractChunk:
    """One launch: the capture's samples [a, b) on the device, of which only the intervals ``reads`` are read from the source (the union of
    the segments' supports), ``segments`` (``SEGMENT`` records; ``out_off`` into the plan's packed buffer) and the clip each belongs to."""

    def __init__(self, a, b, reads, segments, clip):
        self.a, self.b, self.reads, self.segments, self.clip = a, b, reads, segments, clip


def plan_extract_chunks(plan, chunk_samples=1 << 24):
    """Cut an extraction into launches.  Every clip is cut along ``m`` into pieces whose support fits ``chunk_samples``; the pieces, sorted
    by first input sample, are packed into chunks [a, b) with b - a <= chunk_samples that hold every piece's clipped support, so
    overlapping detections share one copy.  -> list of ``ExtractChunk``."""
    chunk_samples = int(chunk_samples)
    if chunk_samples < MIN_CHUNK:
        raise ValueError(f"plan_extract_chunks: chunk_samples = {chunk_samples} is below the {MIN_CHUNK} samples one tile at D = 64 reads")
    pieces = []                                                # (a, b, clip, m0, M)
    for k in range(len(plan)):
        D, l, m0, left = int(plan.D[k]), int(plan.log2d[k]), int(plan.m_first[k]), int(plan.M[k])
        cap = chunk_samples if l == 0 else (chunk_samples - (2 * ZERO_CROSSINGS * D + 1)) // D + 1
        while left > 0:
            M = min(left, cap)
            a, b = support(m0, M, l, plan.n)
            pieces.append((a, b, k, m0, M))
            m0, left = m0 + M, left - M
    pieces.sort()
    chunks, cur = [], []
    a = b = 0
    for p in pieces + [None]:
        if p is not None and cur and max(b, p[1]) - a <= chunk_samples:
            cur.append(p)
            b = max(b, p[1])
            continue
        if cur:
            seg = np.zeros(len(cur), dtype=SEGMENT)
            clip = np.array([q[2] for q in cur], dtype=np.int64)
            seg["m0"] = [q[3] for q in cur]
            seg["M"] = [q[4] for q in cur]
            seg["log2d"], seg["dphi"] = plan.log2d[clip], plan.dphi[clip]
            seg["out_off"] = plan.offset[clip] + (seg["m0"] - plan.m_first[clip])
            reads = []
            for q in cur:                                      # sorted by a: merge into the union of the supports
                if reads and q[0] <= reads[-1][1]:
                    reads[-1][1] = max(reads[-1][1], q[1])
                else:
                    reads.append([q[0], q[1]])
            chunks.append(ExtractChunk(a, b, [tuple(r) for r in reads], seg, clip))
        if p is not None:
            cur, a, b = [p], p[0], p[1]
    return chunks


class Extraction:
    """The clips of one extraction: ``samples`` — a list of complex64 device views into one packed buffer (``packed``), clip i with
    ``plan.M[i]`` samples at ``sample_rate[i]`` Hz, centred at ``center_freq[i]`` Hz (really applied), first sample at ``t0[i]`` seconds of
    the capture, decimated by ``decimation[i]``; ``rows[i]`` is its row in the scan's results.  ``cls`` / ``conf`` / ``names`` come from
    the results when the predictor made the extraction."""

    def __init__(self, plan, packed, cls=None, conf=None, names=None):
        self.plan, self.packed = plan, packed
        self.samples = [packed[int(plan.offset[i]):int(plan.offset[i + 1])] for i in range(len(plan))]
        self.sample_rate, self.center_freq, self.t0 = plan.sample_rate, plan.center_freq, plan.t0
        self.decimation, self.rows = plan.D, plan.rows
        self.cls, self.conf, self.names = cls, conf, names

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, i):
        return self.samples[i]

    def save(self, directory):
        """Write ``clip_<row>.cf32`` (raw interleaved float32, what ``open_iq`` reads) per clip and one ``clips.json`` that lists, per
        clip, its file, row, rate, centre, t0, decimation, class, confidence and box.  -> the directory."""
        directory = os.fspath(directory)
        os.makedirs(directory, exist_ok=True)
        host = self.packed.cpu().numpy() if len(self) else np.zeros(0, dtype=np.complex64)
        clips = []
        for i in range(len(self)):
            row = int(self.rows[i])
            name = f"clip_{row}.cf32"
            host[int(self.plan.offset[i]):int(self.plan.offset[i + 1])].view(np.float32).tofile(os.path.join(directory, name))
            cls = None if self.cls is None else int(self.cls[i])
            clips.append({"file": name, "row": row, "samples": int(self.plan.M[i]), "sample_rate": float(self.sample_rate[i]),
                          "center_freq": float(self.center_freq[i]), "t0": float(self.t0[i]), "decimation": int(self.decimation[i]),
                          "class": cls, "name": None if cls is None or not self.names else self.names.get(cls),
                          "confidence": None if self.conf is None else float(self.conf[i]),
                          "tf": [float(v) for v in self.plan.tf[i]]})
        with open(os.path.join(directory, "clips.json"), "w") as f:
            json.dump({"capture": {"samples": self.plan.n, "sample_rate": self.plan.fs, "center_freq": self.plan.fc}, "clips": clips}, f,
                      indent=1)
        return directory


class _Stager:
    """Source samples -> device, through one pinned staging buffer (the pattern of ``ResampledCapture._to_device``); a device-tensor
    source is sliced directly."""

    def __init__(self, src, device):
        self.src, self.device = src, torch.device(device)
        self._stage, self._copied = None, None

    def __call__(self, a, b, reads):
        if isinstance(self.src, torch.Tensor) and self.src.is_cuda:
            return self.src[a:b]
        from .spectrogram import read_samples
        n = b - a
        if self._copied is not None:
            self._copied.synchronize()                         # the staging buffer is free once the previous copy is done
        if self._stage is None or self._stage.shape[0] < n:
            self._stage = torch.empty((n,), dtype=torch.complex64).pin_memory()
        host = self._stage.numpy()
        for lo, hi in reads:                                   # the gaps between supports are never read, here or by the kernel
            host[lo - a:hi - a] = read_samples(self.src, lo, hi)
        dev = torch.empty((n,), dtype=torch.complex64, device=self.device)
        dev.copy_(self._stage[:n], non_blocking=True)
        self._copied = torch.cuda.Event()
        self._copied.record()
        return dev


def extract_capture(src, plan, device="cuda", chunk_samples=1 << 24, **meta):
    """Run ``plan`` over the opened capture ``src`` (``open_iq``) -> ``Extraction``.  Per chunk of ``plan_extract_chunks`` ONE copy through
    a pinned buffer (none for a device-tensor source) and ONE launch; an empty plan launches nothing."""
    from .. import ops
    device = torch.device(device)
    if len(src) != plan.n:
        raise ValueError(f"extract_capture: the plan is for a capture of {plan.n} samples, this one has {len(src)}")
    chunks = plan_extract_chunks(plan, chunk_samples) if len(plan) else []
    packed = torch.empty((plan.total,), dtype=torch.complex64, device=device)
    if chunks:
        stage, taps = _Stager(src, device), taps_on(packed.device)
        for ch in chunks:
            ops.iq_extract(stage(ch.a, ch.b, ch.reads), ch.a, plan.n, ch.segments, taps, packed)
    return Extraction(plan, packed, **meta)


def extract_results(iq, results, sample_rate, center_freq, device, rows=None, pad_t=0.0, pad_f=0.1, decimate="auto", chunk_samples=1 << 24):
    """``extract_capture`` for the rows of a ``ScanResults``: only ``results.tf`` drives it; class, confidence and names ride along."""
    plan = plan_extract(results.tf, len(iq), sample_rate, center_freq, pad_t, pad_f, decimate, rows)
    boxes = results.boxes.detach().cpu().numpy() if isinstance(results.boxes, torch.Tensor) else np.asarray(results.boxes)
    return extract_capture(iq, plan, device, chunk_samples, cls=boxes[plan.rows, 5].astype(np.int64), conf=boxes[plan.rows, 4],
                           names=results.names)
