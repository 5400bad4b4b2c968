"""Measure every detection of a scan on the GPU: the host plan of ``csrc/measure.hip`` (Welch power spectrum of every box, all boxes of a
staged span in ONE launch, then one reduction launch) and ``measure_capture``, which feeds it a capture chunk by chunk.

Definition.  A capture of ``n`` samples at ``fs`` Hz centred at ``fc``; ``N = n_fft``, ``H = N / 2``, ``w`` the periodic Hann window
(float64, rounded once to f32), ``W2 = sum w^2`` (float64, exactly rounded).  Frame ``j`` is the samples ``[j H, j H + N)``, anchored at sample 0.
For a box ``[t0, f_lo, t1, f_hi]``:

    frames   j_first = floor(t0 fs / H), j_last = max(j_first, ceil(t1 fs / H) - 2), both clipped to [0, (n - N) // H];  J = j_last - j_first + 1
    bins     signed, k in [-N/2, N/2) at fc + k fs / N;  k_lo = ceil((f_lo - fc) N / fs), k_hi = floor((f_hi - fc) N / fs), clipped to the
             band; when that leaves nothing both are floor((centre - fc) N / fs + 1/2), clipped
    search   g = ceil(pad_f (k_hi - k_lo + 1)): [k_lo - g, k_hi + g], clipped to the band
    noise    every k outside the search span with -L <= k <= L - 1, L = floor(noise_band N / 2)
    P[k]     = (1 / (J N W2)) sum_j |FFT(w x_j)[k]|^2:  sum_k P[k] is the window-weighted mean of |x|^2

and from ``P``: ``power`` (in-box sum), ``noise_density`` (median of the noise bins, corrected to a mean), ``snr_db``, the ``beta`` occupied
``bandwidth`` and the power-weighted ``centroid`` over the search span.  All rounding of times and frequencies happens here, in float64;
the device receives integers.
"""
from __future__ import annotations

import json
import math
import os

import numpy as np
import torch

N_FFT = (64, 128, 256, 512, 1024)
MAX_FRAMES = 1 << 27                                           # packed envelope values of one measurement (512 MiB)

# laid out as sy11_psd_item / sy11_psd_box (include/sy11.h)
ITEM = np.dtype([("j0", "<i8"), ("env_off", "<i8"), ("nf", "<i4"), ("row", "<i4"), ("k_lo", "<i4"), ("k_hi", "<i4")])
BOX = np.dtype([("row0", "<i8"), ("n_rows", "<i4"), ("k_lo", "<i4"), ("k_hi", "<i4"), ("s_lo", "<i4"), ("s_hi", "<i4"), ("noise_l", "<i4"),
                ("scale", "<f8"), ("corr", "<f8")])


def group():
    """G: the frames of one group, a constant of the library's build (``sy11_iq_psd_group``)."""
    from .. import _lib
    return int(_lib.load().sy11_iq_psd_group())


def min_chunk(n_fft):
    """The smallest legal ``chunk_samples``: the support of one group, (G - 1) H + N."""
    return (group() - 1) * (n_fft // 2) + n_fft


_TABLES, _TABLES_DEV = {}, {}


def tables(n_fft):
    """-> (window float32 (N,), twiddle complex128 (N / 2,), W2 float): the periodic Hann window, e^{-2 pi i m / N} and sum w^2."""
    if n_fft not in _TABLES:
        i = np.arange(n_fft, dtype=np.float64)
        w = (0.5 - 0.5 * np.cos(2.0 * np.pi * i / n_fft)).astype(np.float32)
        ph = -2.0 * np.pi * np.arange(n_fft // 2, dtype=np.float64) / n_fft
        _TABLES[n_fft] = (w, np.cos(ph) + 1j * np.sin(ph), math.fsum((w.astype(np.float64) ** 2).tolist()))
    return _TABLES[n_fft]


def tables_on(device, n_fft):
    """The tables of ``n_fft`` on ``device``, uploaded once: (window, twiddle, nw2 = N W2)."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if (device, n_fft) not in _TABLES_DEV:
        w, tw, W2 = tables(n_fft)
        _TABLES_DEV[device, n_fft] = (torch.from_numpy(w).to(device), torch.from_numpy(tw).to(device), float(n_fft) * W2)
    return _TABLES_DEV[device, n_fft]


class MeasurePlan:
    """Per selected row of ``tf``: ``j_first`` / ``J`` (frames), ``k_lo`` / ``k_hi`` (in-box bins), ``s_lo`` / ``s_hi`` (search span), ``n_noise``;
    for all: ``noise_l``, ``frac_lo`` / ``frac_hi``, ``G``.  ``offset`` (k + 1) packs the envelopes, ``row0`` (k + 1) the partial rows (one per
    group a box touches).  ``rows`` are the rows of ``tf`` measured, ``tf`` their boxes; ``n`` / ``fs`` / ``fc`` describe the capture."""

    def __init__(self, n, fs, fc, n_fft, rows, tf, j_first, J, k_lo, k_hi, s_lo, s_hi, noise_l, beta, G):
        self.n, self.fs, self.fc, self.n_fft, self.G = int(n), float(fs), float(fc), int(n_fft), int(G)
        self.rows, self.tf = rows, tf
        self.j_first, self.J, self.k_lo, self.k_hi, self.s_lo, self.s_hi = j_first, J, k_lo, k_hi, s_lo, s_hi
        self.noise_l, self.beta = int(noise_l), float(beta)
        self.frac_lo, self.frac_hi = (1.0 - self.beta) / 2.0, (1.0 + self.beta) / 2.0
        k = np.arange(-n_fft // 2, n_fft // 2)[None, :]
        self.n_noise = ((k >= -self.noise_l) & (k <= self.noise_l - 1) & ((k < s_lo[:, None]) | (k > s_hi[:, None]))).sum(1).astype(np.int64)
        W2 = tables(n_fft)[2]
        Jf = J.astype(np.float64)
        self.scale = 1.0 / (Jf * float(n_fft) * W2)
        d = 1.0 - 1.0 / (9.0 * Jf)
        self.corr = 1.0 / (d * d * d)
        self.groups = (j_first + J - 1) // self.G - j_first // self.G + 1
        self.offset = np.concatenate(([0], np.cumsum(J, dtype=np.int64))).astype(np.int64)
        self.row0 = np.concatenate(([0], np.cumsum(self.groups, dtype=np.int64))).astype(np.int64)
        self.total_frames, self.total_rows = int(self.offset[-1]), int(self.row0[-1])

    def __len__(self):
        return self.rows.shape[0]

    def __repr__(self):
        return f"MeasurePlan({len(self)} boxes, N = {self.n_fft}, {self.total_frames} frames in {self.total_rows} groups)"

    def items(self):
        """Every (box, group) work item -> (``ITEM`` records with ``row`` / ``env_off`` into the plan's tables, the box of each)."""
        G = self.G
        box = np.repeat(np.arange(len(self), dtype=np.int64), self.groups)
        g = self.j_first[box] // G + (np.arange(self.total_rows, dtype=np.int64) - self.row0[:-1][box])
        j0 = np.maximum(self.j_first[box], g * G)
        j1 = np.minimum(self.j_first[box] + self.J[box] - 1, g * G + G - 1)
        it = np.zeros(self.total_rows, dtype=ITEM)
        it["j0"], it["nf"], it["row"] = j0, j1 - j0 + 1, np.arange(self.total_rows)
        it["env_off"] = self.offset[:-1][box] + (j0 - self.j_first[box])
        it["k_lo"], it["k_hi"] = self.k_lo[box], self.k_hi[box]
        return it, box

    def boxes(self):
        """The ``BOX`` records of the reduction."""
        bx = np.zeros(len(self), dtype=BOX)
        bx["row0"], bx["n_rows"] = self.row0[:-1], self.groups
        bx["k_lo"], bx["k_hi"], bx["s_lo"], bx["s_hi"] = self.k_lo, self.k_hi, self.s_lo, self.s_hi
        bx["noise_l"], bx["scale"], bx["corr"] = self.noise_l, self.scale, self.corr
        return bx


def plan_measure(tf, n, sample_rate, center_freq=0.0, n_fft=1024, pad_f=0.25, beta=0.99, noise_band=0.8, rows=None, max_frames=MAX_FRAMES):
    """The ``MeasurePlan`` of the boxes ``tf`` (k, 4) [t0_s, f_lo_hz, t1_s, f_hi_hz] (``ScanResults.tf`` or ``Tracks.tf``) on a capture of ``n``
    samples at ``sample_rate`` Hz centred at ``center_freq`` — the capture's OWN rate and centre.  ``rows``: the rows to measure (default:
    all).  Every argument error is a ``ValueError`` raised here, before anything touches the device."""
    fs, fc, n = float(sample_rate), float(center_freq), int(n)
    if not (math.isfinite(fs) and fs > 0 and math.isfinite(fc)):
        raise ValueError(f"plan_measure: sample_rate must be positive and center_freq finite, got {sample_rate!r} / {center_freq!r}")
    if isinstance(n_fft, bool) or not isinstance(n_fft, (int, np.integer)) or int(n_fft) not in N_FFT:
        raise ValueError(f"plan_measure: n_fft must be one of {N_FFT}, got {n_fft!r}")
    N = int(n_fft)
    H = N // 2
    if n < N:
        raise ValueError(f"plan_measure: the capture has {n} samples, fewer than one frame of n_fft = {N}")
    pad_f, beta, noise_band = float(pad_f), float(beta), float(noise_band)
    if not (math.isfinite(pad_f) and pad_f >= 0):
        raise ValueError(f"plan_measure: pad_f must be finite and >= 0, got {pad_f!r}")
    if not 0 < beta <= 1:
        raise ValueError(f"plan_measure: beta must lie in (0, 1], got {beta!r}")
    if not 0 < noise_band <= 1:
        raise ValueError(f"plan_measure: noise_band must lie in (0, 1], got {noise_band!r}")
    if isinstance(tf, torch.Tensor):
        tf = tf.detach().cpu().numpy()
    tf = np.asarray(tf, dtype=np.float64).reshape(-1, 4)
    if rows is None:
        rows = np.arange(tf.shape[0], dtype=np.int64)
    else:
        rows = np.asarray(rows).reshape(-1)
        if rows.size and not np.issubdtype(rows.dtype, np.integer):
            raise ValueError(f"plan_measure: rows must be integer indices, got {rows.dtype}")
        rows = rows.astype(np.int64)
        if rows.size and (rows.min() < 0 or rows.max() >= tf.shape[0]):
            raise ValueError(f"plan_measure: rows must index the {tf.shape[0]} boxes, got {int(rows.min())} .. {int(rows.max())}")
    box = tf[rows]
    if not np.isfinite(box).all():
        raise ValueError(f"plan_measure: box {int(rows[np.flatnonzero(~np.isfinite(box).all(1))[0]])} is not finite")
    bad = (box[:, 2] < box[:, 0]) | (box[:, 3] < box[:, 1])
    if bad.any():
        raise ValueError(f"plan_measure: box {int(rows[np.flatnonzero(bad)[0]])} is inverted (t1 < t0 or f_hi < f_lo)")
    centre = (box[:, 1] + box[:, 3]) / 2
    bad = np.abs(centre - fc) > fs / 2
    if bad.any():
        k = np.flatnonzero(bad)[0]
        raise ValueError(f"plan_measure: box {int(rows[k])} is centred at {centre[k]!r} Hz, outside the capture's {fc!r} +- {fs / 2!r} Hz")
    j_max = (n - N) // H
    j_first = np.floor(box[:, 0] * fs / H).astype(np.int64)
    j_last = np.maximum(j_first, np.ceil(box[:, 2] * fs / H).astype(np.int64) - 2)
    j_first, j_last = np.clip(j_first, 0, j_max), np.clip(j_last, 0, j_max)
    J = j_last - j_first + 1
    k_lo = np.maximum(np.ceil((box[:, 1] - fc) * N / fs).astype(np.int64), -H)
    k_hi = np.minimum(np.floor((box[:, 3] - fc) * N / fs).astype(np.int64), H - 1)
    near = np.clip(np.floor((centre - fc) * N / fs + 0.5).astype(np.int64), -H, H - 1)
    none = k_lo > k_hi
    k_lo, k_hi = np.where(none, near, k_lo), np.where(none, near, k_hi)
    g = np.ceil(pad_f * (k_hi - k_lo + 1)).astype(np.int64)
    s_lo, s_hi = np.maximum(k_lo - g, -H), np.minimum(k_hi + g, H - 1)
    if int(J.sum()) > int(max_frames):
        raise ValueError(f"plan_measure: the {box.shape[0]} boxes hold {int(J.sum())} frames, above max_frames = {int(max_frames)}; "
                         f"measure fewer at a time with rows=")
    return MeasurePlan(n, fs, fc, N, rows, box, j_first, J, k_lo, k_hi, s_lo, s_hi, math.floor(noise_band * N / 2), beta, group())


class MeasureChunk:
    """One launch: the capture's samples [a, b) on the device, of which only the intervals ``reads`` are read from the source (the union of
    the items' supports), and its ``items`` (``ITEM`` records)."""

    def __init__(self, a, b, reads, items):
        self.a, self.b, self.reads, self.items = a, b, reads, items


def plan_measure_chunks(plan, chunk_samples=1 << 24):
    """Cut a measurement into launches: the (box, group) items, sorted by first input sample, are packed into chunks [a, b) with
    b - a <= chunk_samples that hold every item's support whole, so every partial row is written exactly once and overlapping boxes
    share one copy.  -> list of ``MeasureChunk``."""
    chunk_samples = int(chunk_samples)
    if chunk_samples < min_chunk(plan.n_fft):
        raise ValueError(f"plan_measure_chunks: chunk_samples = {chunk_samples} is below the {min_chunk(plan.n_fft)} samples one group of "
                         f"{plan.G} frames at n_fft = {plan.n_fft} reads")
    if not len(plan):
        return []
    it, _ = plan.items()
    H = plan.n_fft // 2
    lo, hi = it["j0"] * H, (it["j0"] + it["nf"] - 1) * H + plan.n_fft
    order = np.lexsort((hi, lo))
    chunks, cur = [], []
    a = b = 0
    for i in list(order) + [None]:
        if i is not None and cur and max(b, int(hi[i])) - a <= chunk_samples:
            cur.append(i)
            b = max(b, int(hi[i]))
            continue
        if cur:
            reads = []
            for q in cur:                                      # sorted by lo: merge into the union of the supports
                if reads and lo[q] <= reads[-1][1]:
                    reads[-1][1] = max(reads[-1][1], int(hi[q]))
                else:
                    reads.append([int(lo[q]), int(hi[q])])
            chunks.append(MeasureChunk(a, b, [tuple(r) for r in reads], it[np.array(cur)]))
        if i is not None:
            cur, a, b = [i], int(lo[i]), int(hi[i])
    return chunks


def _db(v):
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10(v)


class Measurement:
    """The measured rows of one call, each a numpy array over the rows unless noted: ``power`` (mean |x|^2 inside the box's bins) /
    ``power_db``; ``noise_density`` (per Hz) / ``noise_db_hz``; ``snr_db`` (-inf when nothing exceeds the floor, NaN without noise bins);
    ``bandwidth`` (Hz, the ``beta`` occupied bandwidth) with its edges ``f_lo_meas`` / ``f_hi_meas``; ``centroid`` (Hz, NaN when nothing exceeds
    the floor); ``frames`` (J); ``rows`` (the rows of the results); ``tf`` (their boxes).  ``psd`` is a (len, N) float64 DEVICE tensor in
    signed-bin order, ``freqs`` (N,) the bins' frequencies.  ``raw`` keeps what the device returned (``p_in``, ``noise_median``, ``sum_c``,
    ``sum_kc``, ``k_dn``, ``k_up``, ``n_in``, ``n_noise``).  ``cls`` / ``conf`` / ``names`` come from the results when the predictor measured."""

    def __init__(self, plan, psd, out_f, out_i, env=None, cls=None, conf=None, names=None):
        self.plan, self.psd, self.env = plan, psd, env
        self.cls, self.conf, self.names = cls, conf, names
        N, fs, fc = plan.n_fft, plan.fs, plan.fc
        f, i = np.asarray(out_f, dtype=np.float64).reshape(-1, 4), np.asarray(out_i, dtype=np.int64).reshape(-1, 4)
        self.raw = {"p_in": f[:, 0], "noise_median": f[:, 1], "sum_c": f[:, 2], "sum_kc": f[:, 3], "k_dn": i[:, 0], "k_up": i[:, 1],
                    "n_in": i[:, 2], "n_noise": i[:, 3]}
        nd = f[:, 1] * plan.corr
        self.rows, self.tf, self.frames = plan.rows, plan.tf, plan.J
        self.freqs = fc + np.arange(-N // 2, N // 2, dtype=np.float64) * fs / N
        self.power, self.power_db = f[:, 0], _db(f[:, 0])
        self.noise_density = nd * N / fs
        self.noise_db_hz = _db(self.noise_density)
        with np.errstate(divide="ignore", invalid="ignore"):
            floor = i[:, 2] * nd
            self.snr_db = _db(np.maximum(f[:, 0] - floor, 0.0) / floor)
            self.snr_db[np.isnan(nd)] = np.nan
            self.centroid = fc + (f[:, 3] / f[:, 2]) * fs / N
        self.bandwidth = (i[:, 1] - i[:, 0] + 1) * fs / N
        self.f_lo_meas, self.f_hi_meas = fc + (i[:, 0] - 0.5) * fs / N, fc + (i[:, 1] + 0.5) * fs / N

    def __len__(self):
        return self.rows.shape[0]

    def __getitem__(self, i):
        """Row i as a dict of its scalars."""
        i = range(len(self))[i]
        return {k: getattr(self, k)[i].item() for k in ("power", "power_db", "noise_density", "noise_db_hz", "snr_db", "bandwidth", "f_lo_meas",
                                                        "f_hi_meas", "centroid", "frames", "rows")}

    def envelope(self, i):
        """-> (t, E): per frame of row i its centre in seconds of the capture (numpy) and the in-box power (a float32 device view)."""
        if self.env is None:
            raise ValueError("this Measurement was made with envelope=False")
        i = range(len(self))[i]
        p = self.plan
        t = ((p.j_first[i] + np.arange(p.J[i])) * (p.n_fft // 2) + p.n_fft / 2) / p.fs
        return t, self.env[int(p.offset[i]):int(p.offset[i + 1])]

    def save(self, directory):
        """Write ``measure.npz`` (every column, the spectra, the packed envelopes and their offsets) and ``measure.json``, which lists per
        row its box, class, confidence and the measured scalars.  -> the directory."""
        directory = os.fspath(directory)
        os.makedirs(directory, exist_ok=True)
        cols = ("power", "power_db", "noise_density", "noise_db_hz", "snr_db", "bandwidth", "f_lo_meas", "f_hi_meas", "centroid")
        arrays = {k: getattr(self, k) for k in cols}
        arrays.update(frames=self.frames, rows=self.rows, tf=self.tf, freqs=self.freqs, psd=self.psd.cpu().numpy(), env_offset=self.plan.offset)
        if self.env is not None:
            arrays["env"] = self.env.cpu().numpy()
        np.savez(os.path.join(directory, "measure.npz"), **arrays)
        out = []
        for i in range(len(self)):
            cls = None if self.cls is None else int(self.cls[i])
            row = {"row": int(self.rows[i]), "frames": int(self.frames[i]), "tf": [float(v) for v in self.tf[i]], "class": cls,
                   "name": None if cls is None or not self.names else self.names.get(cls),
                   "confidence": None if self.conf is None else float(self.conf[i])}
            for k in cols:
                v = float(getattr(self, k)[i])
                row[k] = v if math.isfinite(v) else None
            out.append(row)
        p = self.plan
        with open(os.path.join(directory, "measure.json"), "w") as f:
            json.dump({"capture": {"samples": p.n, "sample_rate": p.fs, "center_freq": p.fc}, "n_fft": p.n_fft, "beta": p.beta,
                       "file": "measure.npz", "rows": out}, f, indent=1)
        return directory


def measure_capture(src, plan, device="cuda", envelope=True, chunk_samples=1 << 24, **meta):
    """Run ``plan`` over the opened capture ``src`` (``open_iq``) -> ``Measurement``.  Per chunk of ``plan_measure_chunks`` ONE copy through a
    pinned buffer (none for a device-tensor source) and ONE launch, then one reduction launch; an empty plan launches nothing."""
    from .. import ops
    from .extract import _Stager
    device = torch.device(device)
    if len(src) != plan.n:
        raise ValueError(f"measure_capture: the plan is for a capture of {plan.n} samples, this one has {len(src)}")
    N = plan.n_fft
    if not len(plan):
        return Measurement(plan, torch.empty((0, N), dtype=torch.float64, device=device), np.zeros((0, 4)), np.zeros((0, 4), dtype=np.int64),
                           torch.empty((0,), dtype=torch.float32, device=device) if envelope else None, **meta)
    chunks = plan_measure_chunks(plan, chunk_samples)
    partial = torch.empty((plan.total_rows, N), dtype=torch.float32, device=device)
    env = torch.empty((plan.total_frames,), dtype=torch.float32, device=device) if envelope else None
    stage = _Stager(src, device)
    window, twiddle, nw2 = tables_on(partial.device, N)
    for ch in chunks:
        ops.iq_psd(stage(ch.a, ch.b, ch.reads), ch.a, plan.n, N, ch.items, window, twiddle, nw2, partial, env)
    psd, out_f, out_i = ops.psd_measure(partial, plan.boxes(), plan.frac_lo, plan.frac_hi)
    m = Measurement(plan, psd, out_f.cpu().numpy(), out_i.cpu().numpy(), env, **meta)
    m.partial = partial
    return m


def measure_results(iq, results, sample_rate, center_freq, device, rows=None, n_fft=1024, pad_f=0.25, beta=0.99, noise_band=0.8,
                    envelope=True, chunk_samples=1 << 24):
    """``measure_capture`` for the rows of a ``ScanResults`` or its ``Tracks``: only ``results.tf`` drives it; class, confidence and names
    ride along."""
    plan = plan_measure(results.tf, len(iq), sample_rate, center_freq, n_fft, pad_f, beta, noise_band, rows)
    boxes = results.boxes.detach().cpu().numpy() if isinstance(results.boxes, torch.Tensor) else np.asarray(results.boxes)
    return measure_capture(iq, plan, device, envelope, chunk_samples, cls=boxes[plan.rows, 5].astype(np.int64), conf=boxes[plan.rows, 4],
                           names=results.names)
