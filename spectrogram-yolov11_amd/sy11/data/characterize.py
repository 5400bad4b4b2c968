"""Characterise every clip of an extraction on the GPU: the host plan of ``csrc/cyclo.hip`` (spectral lines of |x|^2, x^2 and x^4 and the
moments behind the fourth-order cumulant, all clips in ONE launch, then one reduction launch) and ``characterize_extraction``.

Definition.  Clip ``i`` is ``x[0 .. M)`` at ``fs = sample_rate[i]`` Hz centred at ``fc = center_freq[i]``; ``N = n_fft``, ``H = N / 2``,
the window and ``W2`` are those of ``measure``.  Frame ``j`` is the clip's samples ``[j H, j H + N)``, ``j = 0 .. J - 1``, ``J = (M - N) // H + 1``; a
clip with ``M < N`` is invalid (NaN / -1 everywhere, ``valid`` False).  With ``y_0 = |x|^2``, ``y_1 = x^2``, ``y_2 = x^4``:

    P_q[k]   = (1 / (J N W2)) sum_j |FFT(w y_q,j)[k]|^2        signed bins k in [-N/2, N/2)
    search   q = 0: k in [k_min, N/2 - 1], k_min = max(3, ceil(min_rate N / fs));   q = 1, 2: every k
    peak     the first maximum of P_q over the search set, its cyclic neighbours, and the median of the search set as the floor
    moments  m20 = sum x^2, m21 = sum |x|^2, m42 = sum |x|^4 over the L = (J - 1) H + N samples the frames cover

and on the host, in float64: the parabolic refinement of each peak on ln P, ``f_q = (k + delta) / N fs``, ``line_db_q = 10 log10(P[k] /
median)``; ``symbol_rate = f_0``, ``offset2 = f_1 / 2`` (unambiguous for |offset| < fs / 4), ``offset4 = f_2 / 4`` (|offset| < fs / 8); ``power = m21
/ L``; ``c42 = (m42 / L - |m20 / L|^2 - 2 (m21 / L)^2) / (m21 / L)^2``, not corrected for noise (BPSK -2, four-phase or a bare carrier -1,
Gaussian noise 0); ``order`` 2 when ``line_db_1 >= line_db``, else 4 when ``line_db_2 >= line_db``, else 0; ``carrier = fc + offset_order`` (NaN
for order 0); ``keyed = line_db_0 >= line_db``.  The threshold ``line_db`` (13 dB by default) is a judgement, not a measurement.
"""
from __future__ import annotations

import json
import math
import os

import numpy as np
import torch

from .measure import N_FFT, tables, tables_on

MIN_BIN = 3                                                    # q = 0 never searches below it: DC and the Hann main lobe

# laid out as sy11_cyclo_item / sy11_cyclo_row (include/sy11.h)
ITEM = np.dtype([("off", "<i8"), ("len", "<i8"), ("j0", "<i4"), ("nf", "<i4"), ("row", "<i4"), ("last", "<i4")])
ROW = np.dtype([("row0", "<i8"), ("n_rows", "<i4"), ("clip", "<i4"), ("k_min", "<i4"), ("reserved", "<i4"), ("scale", "<f8")])


def group():
    """G: the frames of one group, a constant of the library's build (``sy11_iq_cyclo_group``)."""
    from .. import _lib
    return int(_lib.load().sy11_iq_cyclo_group())


class CharacterizePlan:
    """Per clip: ``M`` (samples), ``fs``, ``offset`` (first sample in the packed buffer), ``valid`` (M >= N), ``J`` (frames; 0 when invalid), ``L``
    (samples the frames cover), ``k_min``, ``groups`` and ``row0`` (k + 1 offsets into the partial table: one row per group of a valid clip);
    for all: ``n_fft``, ``min_rate``, ``G``."""

    def __init__(self, M, fs, offset, n_fft, min_rate, k_min, G):
        self.M, self.fs, self.offset, self.n_fft, self.min_rate, self.k_min, self.G = M, fs, offset, int(n_fft), float(min_rate), k_min, int(G)
        N, H = self.n_fft, self.n_fft // 2
        self.valid = M >= N
        self.J = np.where(self.valid, (M - N) // H + 1, 0).astype(np.int64)
        self.L = np.where(self.valid, (self.J - 1) * H + N, 0).astype(np.int64)
        self.groups = -(-self.J // self.G)
        self.row0 = np.concatenate(([0], np.cumsum(self.groups, dtype=np.int64))).astype(np.int64)
        self.total_rows, self.total_frames = int(self.row0[-1]), int(self.J.sum())
        with np.errstate(divide="ignore"):
            self.scale = np.where(self.valid, 1.0 / (self.J.astype(np.float64) * float(N) * tables(N)[2]), np.nan)

    def __len__(self):
        return self.M.shape[0]

    def __repr__(self):
        return f"CharacterizePlan({len(self)} clips, {int(self.valid.sum())} valid, N = {self.n_fft}, {self.total_frames} frames in {self.total_rows} groups)"

    def items(self):
        """Every (clip, group) work item -> (``ITEM`` records with ``row`` into the plan's partial table, the clip of each)."""
        G = self.G
        clip = np.repeat(np.arange(len(self), dtype=np.int64), self.groups)
        g = np.arange(self.total_rows, dtype=np.int64) - self.row0[:-1][clip]
        it = np.zeros(self.total_rows, dtype=ITEM)
        it["off"], it["len"], it["j0"] = self.offset[clip], self.M[clip], g * G
        it["nf"] = np.minimum(self.J[clip] - g * G, G)
        it["row"], it["last"] = np.arange(self.total_rows), g == self.groups[clip] - 1
        return it, clip

    def rows(self):
        """The ``ROW`` records of the reduction: one per valid clip."""
        v = np.flatnonzero(self.valid)
        r = np.zeros(v.shape[0], dtype=ROW)
        r["row0"], r["n_rows"], r["clip"], r["k_min"], r["scale"] = self.row0[:-1][v], self.groups[v], v, self.k_min[v], self.scale[v]
        return r


def plan_characterize(clips, n_fft=1024, min_rate=None):
    """The ``CharacterizePlan`` of ``clips``: an ``Extraction`` (its clips' lengths, rates and packed offsets) or a pair ``(M, sample_rate)`` of
    per-clip lengths and rates (scalars broadcast), packed one after the other.  ``min_rate`` (Hz, default 0): the lowest symbol rate
    searched.  Every argument error is a ``ValueError`` raised here, before anything touches the device."""
    if isinstance(n_fft, bool) or not isinstance(n_fft, (int, np.integer)) or int(n_fft) not in N_FFT:
        raise ValueError(f"plan_characterize: n_fft must be one of {N_FFT}, got {n_fft!r}")
    N = int(n_fft)
    if hasattr(clips, "plan") and hasattr(clips, "packed"):
        M, fs, offset = np.asarray(clips.plan.M), np.asarray(clips.sample_rate), np.asarray(clips.plan.offset)[:-1]
    else:
        try:
            M, fs = clips
        except (TypeError, ValueError):
            raise ValueError("plan_characterize: clips must be an Extraction or a pair (M, sample_rate)") from None
        M = np.atleast_1d(np.asarray(M))
        fs, offset = np.asarray(fs, dtype=np.float64), None
    if M.ndim != 1 or (M.size and not np.issubdtype(M.dtype, np.integer)) or (M.size and M.min() < 0):
        raise ValueError("plan_characterize: the clips' lengths must be a 1-D array of integers >= 0")
    M = M.astype(np.int64)
    try:
        fs = np.broadcast_to(np.asarray(fs, dtype=np.float64), M.shape).copy()
    except ValueError:
        raise ValueError(f"plan_characterize: {M.shape[0]} lengths but sample rates of shape {np.shape(fs)}") from None
    if not (np.isfinite(fs).all() and (fs > 0).all()):
        raise ValueError("plan_characterize: every sample rate must be positive and finite")
    if offset is None:
        offset = np.concatenate(([0], np.cumsum(M, dtype=np.int64)))[:-1]
    if M.size and int(M.max()) >= 2 ** 31:
        raise ValueError(f"plan_characterize: a clip of {int(M.max())} samples is not below 2^31")
    min_rate = 0.0 if min_rate is None else float(min_rate)
    if not (math.isfinite(min_rate) and min_rate >= 0):
        raise ValueError(f"plan_characterize: min_rate must be finite and >= 0, got {min_rate!r}")
    k_min = np.maximum(MIN_BIN, np.ceil(min_rate * N / fs)).astype(np.int64)
    bad = k_min > N // 2 - 2
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise ValueError(f"plan_characterize: min_rate = {min_rate!r} leaves fewer than 2 searched bins for clip {i} at {fs[i]!r} Hz "
                         f"(bins {int(k_min[i])} .. {N // 2 - 1})")
    return CharacterizePlan(M, fs, offset.astype(np.int64), N, min_rate, k_min, group())


def _check_line_db(line_db):
    line_db = float(line_db)
    if not math.isfinite(line_db):
        raise ValueError(f"characterize: line_db must be finite, got {line_db!r}")
    return line_db


def _db(v):
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10(v)


class Characterization:
    """One row per clip, each a numpy array over the clips unless noted.  ``valid``; ``frames`` (J, -1 when invalid); ``symbol_rate`` (Hz, the
    line of |x|^2) and ``keyed`` (its line reaches ``line_db``); ``offset2`` / ``offset4`` (Hz from the clip's centre, the lines of x^2 and x^4 over
    2 and 4: unambiguous for |offset| < fs / 4 and fs / 8); ``line_db`` (n, 3): the three lines above their median floors in dB; ``peak_bin``
    (n, 3) signed bins, -1 when invalid, and ``line_freq`` (n, 3) the refined line frequencies f_q; ``order`` (2, 4, 0; -1 when invalid) and
    ``carrier`` (Hz absolute, NaN for order 0); ``power`` (mean |x|^2) and ``c42``.  ``spectra`` is a (n, 3, N) float64 DEVICE tensor in signed-bin
    order (NaN rows for invalid clips), ``freqs(i, q)`` its axis.  ``rows`` / ``cls`` / ``conf`` / ``names`` come from the extraction.  ``raw`` keeps
    what the device returned (``peak``, ``left``, ``right``, ``median`` (n, 3); ``m20`` complex, ``m21``, ``m42``; ``n_search`` (n, 3))."""

    COLUMNS = ("symbol_rate", "offset2", "offset4", "carrier", "power", "c42")

    def __init__(self, plan, center_freq, spectra, out, line_db=13.0, rows=None, cls=None, conf=None, names=None):
        self.plan, self.spectra, self.threshold = plan, spectra, float(line_db)
        self.rows, self.cls, self.conf, self.names = rows, cls, conf, names
        n, N = len(plan), plan.n_fft
        fs, fc = plan.fs, np.broadcast_to(np.asarray(center_freq, dtype=np.float64), (n,)).copy()
        self.sample_rate, self.center_freq = fs, fc
        o = np.asarray(out, dtype=np.float64).reshape(n, 22)
        valid = plan.valid
        pk = o[:, 0:12].reshape(n, 3, 4)
        peak, left, right, med = pk[:, :, 0], pk[:, :, 1], pk[:, :, 2], pk[:, :, 3]
        ints = np.where(valid[:, None], o[:, 16:22], -1.0).astype(np.int64).reshape(n, 3, 2)
        self.valid, self.frames = valid, np.where(valid, plan.J, -1)
        self.peak_bin, n_search = ints[:, :, 0], ints[:, :, 1]
        self.raw = {"peak": peak, "left": left, "right": right, "median": med, "m20": o[:, 12] + 1j * o[:, 13], "m21": o[:, 14], "m42": o[:, 15],
                    "n_search": n_search}
        with np.errstate(divide="ignore", invalid="ignore"):
            ok = (left > 0) & (right > 0) & (peak > 0)
            a, b, c = (np.log(np.where(ok, v, 1.0)) for v in (left, peak, right))
            den = a - 2.0 * b + c
            delta = np.where(ok & (den != 0), 0.5 * (a - c) / np.where(den != 0, den, 1.0), 0.0)
            self.line_freq = np.where(valid[:, None], (self.peak_bin + delta) / N * fs[:, None], np.nan)
            self.line_db = np.where(valid[:, None], _db(peak / med), np.nan)
            Lf = np.where(valid, plan.L, 1).astype(np.float64)
            m21, m42, m20 = o[:, 14] / Lf, o[:, 15] / Lf, (o[:, 12] + 1j * o[:, 13]) / Lf
            self.power = np.where(valid, m21, np.nan)
            self.c42 = np.where(valid, (m42 - (m20.real * m20.real + m20.imag * m20.imag) - 2.0 * (m21 * m21)) / (m21 * m21), np.nan)
        self.symbol_rate, self.offset2, self.offset4 = self.line_freq[:, 0], self.line_freq[:, 1] / 2.0, self.line_freq[:, 2] / 4.0
        with np.errstate(invalid="ignore"):
            self.keyed = valid & (self.line_db[:, 0] >= self.threshold)
            self.order = np.where(~valid, -1, np.where(self.line_db[:, 1] >= self.threshold, 2, np.where(self.line_db[:, 2] >= self.threshold, 4, 0)))
        self.carrier = np.where(self.order == 2, fc + self.offset2, np.where(self.order == 4, fc + self.offset4, np.nan))

    def __len__(self):
        return len(self.plan)

    def __getitem__(self, i):
        """Row i as a dict of its scalars."""
        i = range(len(self))[i]
        d = {k: getattr(self, k)[i].item() for k in self.COLUMNS + ("order", "keyed", "valid", "frames")}
        d.update(rate_line_db=self.line_db[i, 0].item(), line2_db=self.line_db[i, 1].item(), line4_db=self.line_db[i, 2].item())
        return d

    def freqs(self, i, q=0):
        """The frequencies of ``spectra[i, q]``'s bins, in Hz of the transformed sequence: a line of x^2 at f is a carrier offset of f / 2, a line
        of x^4 one of f / 4."""
        i, q = range(len(self))[i], range(3)[q]
        N = self.plan.n_fft
        return np.arange(-N // 2, N // 2, dtype=np.float64) * self.plan.fs[i] / N

    def save(self, directory):
        """Write ``characterize.npz`` (every column and the spectra) and ``characterize.json``, which lists per clip its row, class,
        confidence and the derived scalars.  -> the directory."""
        directory = os.fspath(directory)
        os.makedirs(directory, exist_ok=True)
        arrays = {k: getattr(self, k) for k in self.COLUMNS + ("order", "keyed", "valid", "frames", "line_db", "line_freq", "peak_bin", "sample_rate",
                                                               "center_freq")}
        arrays.update(spectra=self.spectra.cpu().numpy(), rows=np.arange(len(self)) if self.rows is None else np.asarray(self.rows))
        np.savez(os.path.join(directory, "characterize.npz"), **arrays)
        out = []
        for i in range(len(self)):
            cls = None if self.cls is None else int(self.cls[i])
            row = {"row": int(arrays["rows"][i]), "valid": bool(self.valid[i]), "frames": int(self.frames[i]), "order": int(self.order[i]),
                   "keyed": bool(self.keyed[i]), "class": cls, "name": None if cls is None or not self.names else self.names.get(cls),
                   "confidence": None if self.conf is None else float(self.conf[i]), "sample_rate": float(self.sample_rate[i]),
                   "center_freq": float(self.center_freq[i])}
            for k, v in [(k, getattr(self, k)[i]) for k in self.COLUMNS] + list(zip(("rate_line_db", "line2_db", "line4_db"), self.line_db[i])):
                row[k] = float(v) if math.isfinite(float(v)) else None
            out.append(row)
        with open(os.path.join(directory, "characterize.json"), "w") as f:
            json.dump({"n_fft": self.plan.n_fft, "min_rate": self.plan.min_rate, "line_db": self.threshold, "file": "characterize.npz",
                       "clips": out}, f, indent=1)
        return directory


def characterize_extraction(extraction, n_fft=1024, min_rate=None, line_db=13.0):
    """Characterise every clip of ``extraction`` (``sy11.data.extract.Extraction``) -> ``Characterization``: ONE stage-1 launch over all
    clips, ONE reduction launch and one copy of its (n, 22) table to the host; an empty extraction, or one without a clip of ``n_fft``
    samples, launches nothing."""
    from .. import ops
    line_db = _check_line_db(line_db)
    plan = plan_characterize(extraction, n_fft, min_rate)
    n, N = len(plan), plan.n_fft
    packed = extraction.packed
    meta = dict(rows=extraction.rows, cls=extraction.cls, conf=extraction.conf, names=extraction.names)
    spectra = torch.full((n, 3, N), float("nan"), dtype=torch.float64, device=packed.device)
    if plan.total_rows == 0:
        return Characterization(plan, extraction.center_freq, spectra, np.full((n, 22), np.nan), line_db, **meta)
    out = torch.full((n, ops.CYCLO_OUT), float("nan"), dtype=torch.float64, device=packed.device)
    partial = torch.empty((plan.total_rows, 3, N), dtype=torch.float32, device=packed.device)
    mom = torch.empty((plan.total_rows, 4), dtype=torch.float64, device=packed.device)
    window, twiddle, _ = tables_on(packed.device, N)
    ops.iq_cyclo(packed, N, plan.items()[0], window, twiddle, partial, mom)
    ops.cyclo_peaks(partial, mom, plan.rows(), n, spectra, out)
    c = Characterization(plan, extraction.center_freq, spectra, out.cpu().numpy(), line_db, **meta)
    c.partial, c.mom = partial, mom
    return c
