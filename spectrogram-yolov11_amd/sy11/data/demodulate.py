"""Demodulate every clip of an extraction on the GPU, feed-forward: the host plan of ``csrc/demod.hip`` (de-rotation, matched filter and
timing partials in ONE launch over all clips; the symbols at the fitted instants in a second; the decisions in a third), the two small
float64 fits between the launches, and ``demodulate_extraction``.

Definition.  Clip ``i`` is ``x[0 .. M)`` at ``fs`` Hz; it comes with a symbol rate, a carrier offset (Hz from the clip's centre) and
an order (2: BPSK, 4: four-phase), from a ``Characterization`` or from the caller.  ``sps = fs / symbol_rate``, ``hw = ceil(span sps)``.

    taps      h[k] = rrc(k / sps, beta), k = -hw .. hw, float64, scaled to sum h^2 = 1, rounded once to float32
    launch 1  xr[n] = x[n] e^{-2 pi i (n Wc mod 2^64) 2^-64}, Wc = round(offset / fs 2^64);  y[n] = f32(sum_k xr[n - k] h[k]) (zeros outside)
              per tile of TILE usable samples of [hw, M - hw):  T = sum |y[n]|^2 e^{-2 pi i (n Ws mod 2^64) 2^-64}, Ws = round(2^64 / sps), and sum |y|^2
    fit       psi_b = arg T_b unwrapped; weighted line psi ~ a n_b + c over the tile centres (weights |T_b|; fewer than 3 tiles: a = 0,
              c = arg sum T_b);  1 / sps' = Ws 2^-64 + a / 2 pi;  symbol i at t_i = T0 + i STEP (Q32.32), STEP = round(sps' 2^32),
              T0 = round(((-c / 2 pi) mod 1) sps' 2^32), for every i with hw + 1 <= t_i >> 32 <= M - hw - 3
    launch 2  s_i = cubic Lagrange interpolation of y[k - 1 .. k + 2] at mu (k = t_i >> 32, mu = the top 24 bits of the fraction), rounded to f32;
              per block of ``block`` symbols:  z_b = sum s_i^order (negated at order 4), sum |s_i|^2
    track     theta_b = arg(z_b) / order unwrapped modulo 2 pi / order;  phi_i = np.interp over the block centres
    launch 3  r_i = f32(s_i e^{-i phi_i}), the decisions d_i, and per block sum |r|^2, sum Re(r conj(point(d))), n
    columns   gain A = sum Re / n, evm = sqrt(max(sum |r|^2 / n - A^2, 0)) / A, mer_db = -20 log10 evm, ...

The device computes y, s and r in float64 and rounds each ONCE to the float32 it stores.  The stream is right up to a rotation by
``2 pi / order`` (``phase_ambiguity``); that is stated, not resolved.
"""
from __future__ import annotations

import json
import math
import os

import numpy as np
import torch

SPS_MIN, SPS_MAX = 2.5, 16.0                                   # judgements: below, the cubic interpolator is not good enough; above, decimate more
MAX_TAPS = 2 * 16 * 16 + 1

# laid out as sy11_demod_item / sy11_demod_block / sy11_demod_dec (include/sy11.h)
ITEM = np.dtype([("off", "<i8"), ("len", "<i8"), ("n0", "<i8"), ("tap_off", "<i8"), ("wc", "<u8"), ("ws", "<u8"), ("cnt", "<i4"), ("hw", "<i4"),
                 ("n_taps", "<i4"), ("row", "<i4"), ("first", "<i4"), ("last", "<i4")])
BLOCK = np.dtype([("off", "<i8"), ("len", "<i8"), ("t0", "<i8"), ("step", "<i8"), ("sym_off", "<i8"), ("n", "<i4"), ("order", "<i4"), ("row", "<i4"),
                  ("reserved", "<i4")])
DEC = np.dtype([("sym_off", "<i8"), ("n_sym", "<i8"), ("row0", "<i8"), ("nb", "<i4"), ("b", "<i4"), ("block", "<i4"), ("order", "<i4")])

REASONS = {"order": "order is not 2 or 4", "keyed": "not keyed", "finite": "rate or offset not finite", "sps": "samples per symbol outside [2.5, 16]",
           "offset": "offset beyond fs / 2", "short": "too short"}


def tile():
    """TILE: the usable samples of one item of launch 1, a constant of the library's build (``sy11_iq_demod_tile``)."""
    from .. import _lib
    return int(_lib.load().sy11_iq_demod_tile())


def rrc(t, beta):
    """The root-raised-cosine pulse of roll-off ``beta`` at ``t`` symbol periods, float64."""
    t = np.asarray(t, dtype=np.float64)
    h = np.empty_like(t)
    zero = np.abs(t) < 1e-9
    sing = np.abs(np.abs(t) - 1.0 / (4.0 * beta)) < 1e-9
    rest = ~(zero | sing)
    h[zero] = 1.0 - beta + 4.0 * beta / np.pi
    h[sing] = beta / np.sqrt(2.0) * ((1.0 + 2.0 / np.pi) * np.sin(np.pi / (4.0 * beta)) + (1.0 - 2.0 / np.pi) * np.cos(np.pi / (4.0 * beta)))
    u = t[rest]
    h[rest] = (np.sin(np.pi * u * (1.0 - beta)) + 4.0 * beta * u * np.cos(np.pi * u * (1.0 + beta))) / (np.pi * u * (1.0 - (4.0 * beta * u) ** 2))
    return h


def make_taps(sps, hw, beta):
    """-> (2 hw + 1,) float32: ``rrc(k / sps, beta)`` in float64, scaled to unit energy, rounded once."""
    h = rrc(np.arange(-hw, hw + 1, dtype=np.float64) / sps, beta)
    return (h / np.sqrt(np.sum(h * h))).astype(np.float32)


class DemodPlan:
    """Per clip: ``M``, ``fs``, ``offset`` (first sample in the packed buffer), ``symbol_rate``, ``carrier_offset`` (Hz), ``order``, ``valid`` and
    ``reason`` ("" when valid), ``sps``, ``hw``, ``n_taps`` and ``tap_off`` (k + 1 offsets into ``taps``, float32), ``Wc`` / ``Ws`` (Python ints below 2^64;
    0 when invalid), ``tiles`` and ``row0`` (k + 1 offsets into the timing table: one row per tile of a valid clip); for all: ``beta``, ``span``,
    ``block``, ``TILE``."""

    def __init__(self, M, fs, offset, rate, carrier, order, valid, reason, beta, span, block, TILE):
        self.M, self.fs, self.offset, self.symbol_rate, self.carrier_offset, self.order = M, fs, offset, rate, carrier, order
        self.valid, self.reason, self.beta, self.span, self.block, self.TILE = valid, reason, float(beta), int(span), int(block), int(TILE)
        n = M.shape[0]
        self.sps = np.full(n, np.nan)
        self.hw, self.n_taps, self.tiles = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        self.Wc, self.Ws, taps = [0] * n, [0] * n, []
        for i in np.flatnonzero(valid):
            sps = float(fs[i]) / float(rate[i])
            hw = math.ceil(self.span * sps)
            self.sps[i], self.hw[i], self.n_taps[i] = sps, hw, 2 * hw + 1
            self.tiles[i] = -(-(int(M[i]) - 2 * hw) // self.TILE)
            self.Ws[i] = int(math.ldexp(float(rate[i]) / float(fs[i]), 64))
            self.Wc[i] = int(math.ldexp(float(carrier[i]) / float(fs[i]), 64)) % (1 << 64)
            taps.append(make_taps(sps, hw, self.beta))
        self.taps = np.concatenate(taps) if taps else np.zeros(0, dtype=np.float32)
        self.tap_off = np.concatenate(([0], np.cumsum(self.n_taps, dtype=np.int64))).astype(np.int64)
        self.row0 = np.concatenate(([0], np.cumsum(self.tiles, dtype=np.int64))).astype(np.int64)
        self.total_rows = int(self.row0[-1])

    def __len__(self):
        return self.M.shape[0]

    def __repr__(self):
        return f"DemodPlan({len(self)} clips, {int(self.valid.sum())} valid, {self.total_rows} tiles of {self.TILE}, {self.taps.shape[0]} taps)"

    def items(self):
        """Every (clip, tile) work item of launch 1 -> (``ITEM`` records with ``row`` into the plan's timing table, the clip of each)."""
        T = self.TILE
        clip = np.repeat(np.arange(len(self), dtype=np.int64), self.tiles)
        b = np.arange(self.total_rows, dtype=np.int64) - self.row0[:-1][clip]
        it = np.zeros(self.total_rows, dtype=ITEM)
        hw = self.hw[clip]
        it["off"], it["len"], it["n0"], it["tap_off"] = self.offset[clip], self.M[clip], hw + b * T, self.tap_off[:-1][clip]
        it["wc"] = np.array([self.Wc[c] for c in clip], dtype=np.uint64)
        it["ws"] = np.array([self.Ws[c] for c in clip], dtype=np.uint64)
        it["cnt"] = np.minimum(self.M[clip] - 2 * hw - b * T, T)
        it["hw"], it["n_taps"], it["row"] = hw, self.n_taps[clip], np.arange(self.total_rows)
        it["first"], it["last"] = b == 0, b == self.tiles[clip] - 1
        return it, clip

    def centres(self, i):
        """The tile centres of clip ``i`` (the mean sample index of every tile), float64."""
        hw, T, nt = int(self.hw[i]), self.TILE, int(self.tiles[i])
        n0 = hw + np.arange(nt, dtype=np.int64) * T
        cnt = np.minimum(int(self.M[i]) - hw - n0, T)
        return n0.astype(np.float64) + (cnt.astype(np.float64) - 1.0) / 2.0


def _per_clip(name, v, n, dtype):
    try:
        return np.broadcast_to(np.asarray(v, dtype=dtype), (n,)).copy()
    except (TypeError, ValueError):
        raise ValueError(f"plan_demodulate: {n} clips but `{name}` of shape {np.shape(v)}") from None


def plan_demodulate(clips, characterization=None, *, symbol_rate=None, offset=None, order=None, beta=0.35, span=8, block=32):
    """The ``DemodPlan`` of ``clips``: an ``Extraction`` or a pair ``(M, sample_rate)`` of per-clip lengths and rates (scalars broadcast), packed one
    after the other.  The per-clip parameters come EITHER from ``characterization`` (its ``symbol_rate``, ``order``, and ``offset2`` / ``offset4`` by
    order; a clip that is not ``keyed`` is invalid) OR from ``symbol_rate``, ``offset`` (Hz from the clip's centre) and ``order`` (scalars broadcast).
    Every argument error is a ``ValueError`` raised here, before anything touches the device; a clip that cannot be demodulated is a row with
    ``valid`` False and a ``reason``."""
    if hasattr(clips, "plan") and hasattr(clips, "packed"):
        M, fs, off = np.asarray(clips.plan.M), np.asarray(clips.sample_rate), np.asarray(clips.plan.offset)[:-1]
    else:
        try:
            M, fs = clips
        except (TypeError, ValueError):
            raise ValueError("plan_demodulate: clips must be an Extraction or a pair (M, sample_rate)") from None
        M, off = np.atleast_1d(np.asarray(M)), None
    if M.ndim != 1 or (M.size and not np.issubdtype(M.dtype, np.integer)) or (M.size and M.min() < 0):
        raise ValueError("plan_demodulate: the clips' lengths must be a 1-D array of integers >= 0")
    M = M.astype(np.int64)
    n = M.shape[0]
    fs = _per_clip("sample_rate", fs, n, np.float64)
    if not (np.isfinite(fs).all() and (fs > 0).all()):
        raise ValueError("plan_demodulate: every sample rate must be positive and finite")
    if M.size and int(M.max()) >= 2 ** 31:
        raise ValueError(f"plan_demodulate: a clip of {int(M.max())} samples is not below 2^31")
    if off is None:
        off = np.concatenate(([0], np.cumsum(M, dtype=np.int64)))[:-1]
    explicit = [v is not None for v in (symbol_rate, offset, order)]
    if characterization is not None and any(explicit):
        raise ValueError("plan_demodulate: give a characterization OR symbol_rate / offset / order, not both")
    if characterization is None and not all(explicit):
        raise ValueError("plan_demodulate: give a characterization, or all of symbol_rate, offset and order")
    for name, v, lo, hi, integer in (("beta", beta, 0.0, 1.0, False), ("span", span, 2, 16, True), ("block", block, 8, 256, True)):
        if isinstance(v, bool) or (integer and not isinstance(v, (int, np.integer))) or not isinstance(v, (int, float, np.integer, np.floating)) \
                or not math.isfinite(float(v)) or not (lo <= v <= hi) or (name == "beta" and not v > 0):
            raise ValueError(f"plan_demodulate: {name} must be {'an integer ' if integer else ''}in {'(' if name == 'beta' else '['}{lo}, {hi}], got {v!r}")
    keyed = np.ones(n, dtype=bool)
    if characterization is not None:
        c = characterization
        if len(c) != n:
            raise ValueError(f"plan_demodulate: {n} clips but a characterization of {len(c)}")
        order = np.asarray(c.order, dtype=np.int64).copy()
        rate = np.asarray(c.symbol_rate, dtype=np.float64).copy()
        carrier = np.where(order == 2, np.asarray(c.offset2, dtype=np.float64), np.where(order == 4, np.asarray(c.offset4, dtype=np.float64), np.nan))
        keyed = np.asarray(c.keyed, dtype=bool) & np.asarray(c.valid, dtype=bool)
    else:
        rate, carrier = _per_clip("symbol_rate", symbol_rate, n, np.float64), _per_clip("offset", offset, n, np.float64)
        o = np.asarray(order)
        if o.size and not (np.issubdtype(o.dtype, np.integer) or (np.issubdtype(o.dtype, np.floating) and np.isfinite(o).all() and (o == np.round(o)).all())):
            raise ValueError("plan_demodulate: `order` must hold integers")
        order = _per_clip("order", order, n, np.int64)
    TILE = tile()
    reason = np.full(n, "", dtype=object)
    for i in range(n):
        if order[i] not in (2, 4):
            reason[i] = REASONS["order"]
        elif not keyed[i]:
            reason[i] = REASONS["keyed"]
        elif not (math.isfinite(rate[i]) and math.isfinite(carrier[i])) or rate[i] <= 0:
            reason[i] = REASONS["finite"]
        elif not (SPS_MIN <= fs[i] / rate[i] <= SPS_MAX):
            reason[i] = REASONS["sps"]
        elif not abs(carrier[i]) < fs[i] / 2:
            reason[i] = REASONS["offset"]
        elif int(M[i]) - 2 * math.ceil(int(span) * (fs[i] / rate[i])) < TILE:
            reason[i] = REASONS["short"]
    valid = reason == ""
    return DemodPlan(M, fs, off.astype(np.int64), rate, carrier, order, valid, reason, beta, span, block, TILE)


# ----------------------------------------------------------------------------------------------------------------- host stages
def _unwrap(a, period):
    """Sequentially: every entry moves by the multiple of ``period`` that brings it nearest the one before."""
    out = np.array(a, dtype=np.float64)
    for b in range(1, out.shape[0]):
        out[b] += np.round((out[b - 1] - out[b]) / period) * period
    return out


def fit(T, centres, Ws, M, hw):
    """The timing fit of one clip: ``T`` (nt,) complex128 timing partials, ``centres`` (nt,) float64 -> dict: psi (unwrapped), a, c, sps, timing
    (tau in symbols), T0, STEP (Python ints, Q32.32), i_first, i_last, n_symbols."""
    T = np.asarray(T, dtype=np.complex128)
    psi = _unwrap(np.arctan2(T.imag, T.real), 2.0 * np.pi)
    w = np.abs(T)
    a, c = 0.0, 0.0
    if T.shape[0] >= 3 and np.sum(w) > 0:
        sw = np.sum(w)
        xm, ym = np.sum(w * centres) / sw, np.sum(w * psi) / sw
        dx = centres - xm
        den = np.sum(w * dx * dx)
        a = float(np.sum(w * dx * (psi - ym)) / den) if den > 0 else 0.0
        c = float(ym - a * xm)
    else:
        s = np.sum(T)
        c = float(np.arctan2(s.imag, s.real))
    inv = math.ldexp(float(Ws), -64) + a / (2.0 * np.pi)
    sps = 1.0 / inv
    tau = (-c / (2.0 * np.pi)) % 1.0
    STEP, T0 = int(round(math.ldexp(sps, 32))), int(round(math.ldexp(tau * sps, 32)))
    lo, hi = (hw + 1) << 32, ((M - hw - 2) << 32) - 1                      # hw + 1 <= t >> 32 <= M - hw - 3
    i_first = max(0, -((T0 - lo) // STEP))
    i_last = (hi - T0) // STEP
    return {"psi": psi, "a": a, "c": c, "sps": sps, "timing": tau, "T0": T0, "STEP": STEP, "i_first": i_first, "i_last": i_last,
            "n_symbols": i_last - i_first + 1}


def block_centres(n_sym, block):
    """The centres (in symbols of the clip) of the blocks of ``block`` symbols, the last one ragged."""
    nb = -(-n_sym // block)
    start = np.arange(nb, dtype=np.int64) * block
    cnt = np.minimum(n_sym - start, block)
    return start.astype(np.float64) + (cnt.astype(np.float64) - 1.0) / 2.0


def phase_track(z, order):
    """``z`` (nb,) complex128 -> theta (nb,): ``arg(z) / order`` unwrapped sequentially modulo ``2 pi / order``."""
    z = np.asarray(z, dtype=np.complex128)
    return _unwrap(np.arctan2(z.imag, z.real) / order, 2.0 * np.pi / order)


def columns(rows, theta, centres, fs_fit_rate, carrier0):
    """The host columns of one clip from its (nb, 3) decision rows, theta and the block centres -> dict: n_symbols, gain, evm, mer_db,
    carrier_fit (``carrier0`` + the slope of theta over the centres, in Hz at ``fs_fit_rate`` symbols per second)."""
    rows = np.asarray(rows, dtype=np.float64)
    n = float(np.sum(rows[:, 2]))
    e2, er = float(np.sum(rows[:, 0])), float(np.sum(rows[:, 1]))
    A = er / n
    with np.errstate(divide="ignore", invalid="ignore"):
        evm = float(np.sqrt(max(e2 / n - A * A, 0.0)) / np.float64(A))
        mer = float(-20.0 * np.log10(np.float64(evm)))
    slope = 0.0
    if theta.shape[0] >= 2:
        dx = centres - np.mean(centres)
        slope = float(np.sum(dx * (theta - np.mean(theta))) / np.sum(dx * dx))
    return {"n_symbols": int(n), "gain": A, "evm": evm, "mer_db": mer, "carrier_fit": carrier0 + slope * fs_fit_rate / (2.0 * np.pi)}


class Demodulation:
    """One row per clip, each a numpy array over the clips unless noted.  ``valid`` and ``reason``; ``n_symbols`` (-1 when invalid), ``gain``, ``evm``,
    ``mer_db``, ``timing`` (tau in symbols), ``symbol_rate_fit`` and ``carrier_fit`` (Hz), NaN when invalid; ``order`` and ``phase_ambiguity`` (= order:
    the stream is right up to a rotation by 2 pi / order).  On the DEVICE, as lists of views into packed buffers (empty views for invalid
    clips): ``symbols`` (the corrected r, complex64), ``decisions`` (uint8: Re r < 0 at order 2, 2 (Re r < 0) + (Im r < 0) at order 4) and
    ``filtered`` (y, complex64, the extraction's layout).  ``rows`` / ``cls`` / ``conf`` / ``names`` come from the extraction.  ``raw`` keeps the three
    device tables (``timing_rows``, ``z_rows``, ``decision_rows``), the pre-correction symbols ``s`` (device), ``row0`` / ``block0`` / ``sym0`` (k + 1 offsets
    of the clips into them) and per clip ``psi``, ``theta`` (lists of arrays), ``T0``, ``STEP``, ``i_first``, ``i_last`` (lists of ints)."""

    COLUMNS = ("gain", "evm", "mer_db", "timing", "symbol_rate_fit", "carrier_fit")

    def __init__(self, plan, center_freq, cols, symbols, decisions, filtered, raw, rows=None, cls=None, conf=None, names=None):
        self.plan, self.raw = plan, raw
        self.rows, self.cls, self.conf, self.names = rows, cls, conf, names
        self.valid, self.reason, self.order = plan.valid, plan.reason, plan.order
        self.phase_ambiguity = np.where(plan.valid, plan.order, -1)
        self.sample_rate, self.center_freq = plan.fs, np.broadcast_to(np.asarray(center_freq, dtype=np.float64), (len(plan),)).copy()
        self.n_symbols = cols["n_symbols"]
        for k in self.COLUMNS:
            setattr(self, k, cols[k])
        self.symbols, self.decisions, self.filtered = symbols, decisions, filtered

    def __len__(self):
        return len(self.plan)

    def __getitem__(self, i):
        """Row i as a dict of its scalars."""
        i = range(len(self))[i]
        d = {k: getattr(self, k)[i].item() for k in self.COLUMNS + ("n_symbols", "order", "valid", "phase_ambiguity")}
        d["reason"] = str(self.reason[i])
        return d

    def bits(self, i):
        """The bits of clip ``i`` on the host, uint8, 1 (order 2) or 2 (order 4, Gray-mapped from the quadrant: the sign bits of Re and Im) per
        symbol, the first symbol first."""
        i = range(len(self))[i]
        d = self.decisions[i].cpu().numpy()
        if int(self.order[i]) == 4:
            return np.stack(((d >> 1) & 1, d & 1), axis=1).reshape(-1).astype(np.uint8)
        return (d & 1).astype(np.uint8)

    def save(self, directory):
        """Write ``demodulate.npz`` (every column, and per clip its decisions), ``symbols_<row>.cf32`` (the corrected symbols, raw interleaved
        float32) per valid clip and ``demodulate.json``, which lists per clip its row, class, confidence and scalars.  -> the directory."""
        directory = os.fspath(directory)
        os.makedirs(directory, exist_ok=True)
        rows = np.arange(len(self)) if self.rows is None else np.asarray(self.rows)
        arrays = {k: getattr(self, k) for k in self.COLUMNS + ("n_symbols", "order", "valid", "phase_ambiguity", "sample_rate", "center_freq")}
        arrays.update(rows=rows, reason=np.asarray([str(r) for r in self.reason], dtype=str))
        out = []
        for i in range(len(self)):
            row, name = int(rows[i]), None
            if self.valid[i]:
                name = f"symbols_{row}.cf32"
                self.symbols[i].cpu().numpy().view(np.float32).tofile(os.path.join(directory, name))
                arrays[f"decisions_{row}"] = self.decisions[i].cpu().numpy()
            cls = None if self.cls is None else int(self.cls[i])
            rec = {"row": row, "valid": bool(self.valid[i]), "reason": str(self.reason[i]), "file": name, "order": int(self.order[i]),
                   "phase_ambiguity": int(self.phase_ambiguity[i]), "n_symbols": int(self.n_symbols[i]), "class": cls,
                   "name": None if cls is None or not self.names else self.names.get(cls),
                   "confidence": None if self.conf is None else float(self.conf[i]), "sample_rate": float(self.sample_rate[i]),
                   "center_freq": float(self.center_freq[i])}
            for k in self.COLUMNS:
                v = float(getattr(self, k)[i])
                rec[k] = v if math.isfinite(v) else None
            out.append(rec)
        np.savez(os.path.join(directory, "demodulate.npz"), **arrays)
        with open(os.path.join(directory, "demodulate.json"), "w") as f:
            json.dump({"beta": self.plan.beta, "span": self.plan.span, "block": self.plan.block, "tile": self.plan.TILE, "file": "demodulate.npz",
                       "clips": out}, f, indent=1)
        return directory


def demodulate_extraction(extraction, characterization=None, *, symbol_rate=None, offset=None, order=None, beta=0.35, span=8, block=32):
    """Demodulate every clip of ``extraction`` (``sy11.data.extract.Extraction``) -> ``Demodulation``: three launches over all clips, three small
    copies to the host (the timing rows, the block sums, the decision rows) and one to the device (theta); an extraction without a valid
    clip launches nothing."""
    from .. import ops
    plan = plan_demodulate(extraction, characterization, symbol_rate=symbol_rate, offset=offset, order=order, beta=beta, span=span, block=block)
    n, packed = len(plan), extraction.packed
    dev = packed.device
    meta = dict(rows=extraction.rows, cls=extraction.cls, conf=extraction.conf, names=extraction.names)
    cols = {k: np.full(n, np.nan) for k in Demodulation.COLUMNS}
    cols["n_symbols"] = np.full(n, -1, dtype=np.int64)
    fc = np.broadcast_to(np.asarray(extraction.center_freq, dtype=np.float64), (n,))
    empty_c, empty_u = torch.zeros(0, dtype=torch.complex64, device=dev), torch.zeros(0, dtype=torch.uint8, device=dev)
    raw = {"timing_rows": None, "z_rows": None, "decision_rows": None, "s": None, "row0": plan.row0, "block0": np.zeros(n + 1, dtype=np.int64),
           "sym0": np.zeros(n + 1, dtype=np.int64), "psi": [np.zeros(0)] * n, "theta": [np.zeros(0)] * n, "T0": [0] * n, "STEP": [0] * n,
           "i_first": [0] * n, "i_last": [-1] * n}
    if plan.total_rows == 0:
        return Demodulation(plan, fc, cols, [empty_c] * n, [empty_u] * n, [empty_c] * n, raw, **meta)
    # launch 1: de-rotation, matched filter, timing partials
    items = plan.items()[0]
    taps = torch.from_numpy(plan.taps).to(dev)
    y = torch.zeros_like(packed)
    trows = torch.empty((plan.total_rows, 3), dtype=torch.float64, device=dev)
    ops.iq_demod_filter(packed, items, taps, y, trows)
    th = trows.cpu().numpy()
    # the timing fit
    v = np.flatnonzero(plan.valid)
    fits = {}
    nsym, nblk = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for i in v:
        r = th[int(plan.row0[i]):int(plan.row0[i + 1])]
        fits[i] = f = fit(r[:, 0] + 1j * r[:, 1], plan.centres(i), plan.Ws[i], int(plan.M[i]), int(plan.hw[i]))
        nsym[i] = f["n_symbols"]
        nblk[i] = -(-f["n_symbols"] // plan.block)
        raw["psi"][i], raw["T0"][i], raw["STEP"][i], raw["i_first"][i], raw["i_last"][i] = f["psi"], f["T0"], f["STEP"], f["i_first"], f["i_last"]
        cols["timing"][i], cols["symbol_rate_fit"][i] = f["timing"], float(plan.fs[i]) / f["sps"]
    sym0 = np.concatenate(([0], np.cumsum(nsym))).astype(np.int64)
    block0 = np.concatenate(([0], np.cumsum(nblk))).astype(np.int64)
    raw["sym0"], raw["block0"] = sym0, block0
    n_sym, n_blk = int(sym0[-1]), int(block0[-1])
    # launch 2: the symbols and the block sums of s^order
    bl, de = np.zeros(n_blk, dtype=BLOCK), np.zeros(n_blk, dtype=DEC)
    for i in v:
        f, a, b = fits[i], int(block0[i]), int(block0[i + 1])
        q = np.arange(b - a, dtype=np.int64)
        bl["off"][a:b], bl["len"][a:b], bl["step"][a:b], bl["order"][a:b] = plan.offset[i], plan.M[i], f["STEP"], plan.order[i]
        bl["t0"][a:b] = [f["T0"] + (f["i_first"] + int(k) * plan.block) * f["STEP"] for k in q]
        bl["sym_off"][a:b], bl["n"][a:b], bl["row"][a:b] = sym0[i] + q * plan.block, np.minimum(nsym[i] - q * plan.block, plan.block), a + q
        de["sym_off"][a:b], de["n_sym"][a:b], de["row0"][a:b], de["nb"][a:b], de["b"][a:b] = sym0[i], nsym[i], a, b - a, q
        de["block"][a:b], de["order"][a:b] = plan.block, plan.order[i]
    s = torch.zeros(n_sym, dtype=torch.complex64, device=dev)
    zrows = torch.empty((n_blk, 3), dtype=torch.float64, device=dev)
    ops.demod_symbols(y, bl, s, zrows)
    zh = zrows.cpu().numpy()
    # the phase track
    theta = np.zeros(n_blk)
    for i in v:
        a, b = int(block0[i]), int(block0[i + 1])
        theta[a:b] = raw["theta"][i] = phase_track(zh[a:b, 0] + 1j * zh[a:b, 1], int(plan.order[i]))
    # launch 3: the decisions
    r = torch.zeros(n_sym, dtype=torch.complex64, device=dev)
    d = torch.zeros(n_sym, dtype=torch.uint8, device=dev)
    drows = torch.empty((n_blk, 3), dtype=torch.float64, device=dev)
    ops.demod_decide(s, de, torch.from_numpy(theta).to(dev), r, d, drows)
    dh = drows.cpu().numpy()
    for i in v:
        a, b = int(block0[i]), int(block0[i + 1])
        c = columns(dh[a:b], theta[a:b], block_centres(int(nsym[i]), plan.block), cols["symbol_rate_fit"][i], float(fc[i]) + float(plan.carrier_offset[i]))
        for k in ("n_symbols", "gain", "evm", "mer_db", "carrier_fit"):
            cols[k][i] = c[k]
    raw.update(timing_rows=trows, z_rows=zrows, decision_rows=drows, s=s)
    off = plan.offset
    symbols = [r[int(sym0[i]):int(sym0[i + 1])] for i in range(n)]
    decisions = [d[int(sym0[i]):int(sym0[i + 1])] for i in range(n)]
    filtered = [y[int(off[i]):int(off[i]) + int(plan.M[i])] if plan.valid[i] else empty_c for i in range(n)]
    return Demodulation(plan, fc, cols, symbols, decisions, filtered, raw, **meta)
