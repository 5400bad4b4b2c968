"""Demodulate every frequency-keyed clip (2-FSK / GFSK / GMSK) of an extraction on the GPU, feed-forward: the host plan of ``csrc/demod_fsk.hip``
(discriminator, post-detection filter and timing partials in ONE launch over all clips; the symbols at the fitted instants and the level sums in
a second; the symbols scaled to +-1 and the decisions in a third), the two small float64 fits between the launches, and
``demodulate_fsk_extraction``.  The result is a ``Demodulation`` at order 2, so ``find_frames``, ``equalize``, ``decode``, ``decode_ldpc`` and ``correct`` take it as it is.

Definition.  Clip ``i`` is ``x[0 .. M)`` at ``fs`` Hz with ``sps = fs / symbol_rate``; SPS_MIN, SPS_MAX and TILE are those of ``demodulate``.

    taps      gauss: h[k] = exp(-2 pi^2 bt^2 (k / sps)^2 / ln 2);  rect: h[k] = |[k - 1/2, k + 1/2] n [-sps/2, sps/2]|
              k = -hw .. hw, float64, scaled to sum h = 1, rounded once to float32;  hw = ceil(span sps) (gauss) or ceil(sps / 2) (rect; span ignored)
    launch 1  f[n] = arg(x[n] conj(x[n-1]) e^{-2 pi i Wc 2^-64}) / 2 pi  (cycles per sample, 1 <= n < M), Wc = round(offset / fs 2^64)
              y[n] = f32(sum_k f[n - k] h[k]) on the usable span hw + 1 <= n < M - hw;  y = 0 elsewhere
              per tile of TILE usable samples, one row of 8 float64, w = e^{-2 pi i (n Ws mod 2^64) 2^-64}:
                  sum y^2 w (Re, Im), sum y w (Re, Im), sum w (Re, Im), sum y, sum y^2
    fit       m = sum(sum y) / (usable samples);  T_b = (sum y^2 w) - 2 m (sum y w) + m^2 (sum w): the line of (y - m)^2
              then ``demodulate.fit`` on T_b and the tile centres, with hw + 1 for its half width (the first usable sample): hw + 2 <= t_i >> 32 <= M - hw - 4
    launch 2  s_i = f32(cubic Lagrange of y[k - 1 .. k + 2] at mu);  per block of ``block`` symbols: n_hi = #(s_i >= m), sum s_i over s_i >= m,
              sum s_i over s_i < m, sum s_i^2
    levels    c_hi, c_lo = the two level means over the clip;  f0 = (c_hi + c_lo) / 2;  dev = (c_hi - c_lo) / 2;  n_hi = 0 or n_lo = 0: "one tone"
    launch 3  r_i = f32((s_i - f0) / dev), stored as complex64 (r_i, 0);  d_i = (r_i < 0);  per block: sum r^2, sum |r|, n
    columns   gain, evm, mer_db by ``demodulate.columns``' rule;  timing, symbol_rate_fit;  carrier_fit = fc + offset + f0 fs;  deviation = dev fs (Hz);
              mod_index = 2 deviation / symbol_rate_fit

The level MIDPOINT is used, not the mean, so that an unbalanced bit stream does not bias ``f0``.  ``f0`` and ``dev`` are constants of the clip.  Which
tone is "1" is not known: ``phase_ambiguity`` is 2, and ``find_frames``' rotation q = 1 is the inverted polarity.

Out of scope: a pre-detection filter (``extract``'s low-pass is the one), 4-FSK, estimating the symbol rate of a frequency-keyed clip in
``characterize`` (the caller gives it), coherent MSK detection, and tracking a carrier that drifts over the clip.
"""
from __future__ import annotations

import json
import math
import os

import numpy as np
import torch

from .demodulate import MAX_TAPS, SPS_MAX, SPS_MIN, Demodulation, _per_clip, block_centres, columns, fit, tile

# laid out as sy11_fsk_item / sy11_fsk_block / sy11_fsk_dec (include/sy11.h)
ITEM = np.dtype([("off", "<i8"), ("len", "<i8"), ("n0", "<i8"), ("tap_off", "<i8"), ("wc", "<u8"), ("ws", "<u8"), ("cnt", "<i4"), ("hw", "<i4"),
                 ("n_taps", "<i4"), ("row", "<i4"), ("first", "<i4"), ("last", "<i4")])
BLOCK = np.dtype([("off", "<i8"), ("len", "<i8"), ("t0", "<i8"), ("step", "<i8"), ("sym_off", "<i8"), ("m", "<f8"), ("n", "<i4"), ("row", "<i4")])
DEC = np.dtype([("sym_off", "<i8"), ("f0", "<f8"), ("dev", "<f8"), ("n", "<i4"), ("row", "<i4")])

PULSES = ("gauss", "rect")
REASONS = {"finite": "rate or offset not finite", "sps": "samples per symbol outside [2.5, 16]", "offset": "offset beyond fs / 2", "short": "too short",
           "tone": "one tone"}


def half_width(sps, pulse, span):
    """hw: ``ceil(span sps)`` for the Gaussian pulse, ``ceil(sps / 2)`` for the rectangular one."""
    return math.ceil(span * sps) if pulse == "gauss" else math.ceil(sps / 2.0)


def make_taps(sps, hw, pulse="gauss", bt=0.5):
    """-> (2 hw + 1,) float32: the post-detection filter in float64, scaled to unit sum, rounded once.  "gauss": the Gaussian of bandwidth-time
    product ``bt``; "rect": the overlap of [k - 1/2, k + 1/2] with the symbol [-sps / 2, sps / 2] (integrate and dump)."""
    k = np.arange(-hw, hw + 1, dtype=np.float64)
    if pulse == "gauss":
        h = np.exp(-2.0 * np.pi ** 2 * bt ** 2 * (k / sps) ** 2 / math.log(2.0))
    else:
        h = np.maximum(np.minimum(k + 0.5, sps / 2.0) - np.maximum(k - 0.5, -sps / 2.0), 0.0)
    return (h / np.sum(h)).astype(np.float32)


class FskPlan:
    """Per clip: ``M``, ``fs``, ``offset`` (first sample in the packed buffer), ``symbol_rate``, ``carrier_offset`` (Hz), ``order`` (2), ``valid`` and ``reason`` (""
    when valid), ``sps``, ``hw``, ``n_taps`` and ``tap_off`` (k + 1 offsets into ``taps``, float32), ``Wc`` / ``Ws`` (Python ints below 2^64; 0 when invalid), ``tiles``
    and ``row0`` (k + 1 offsets into the timing table: one row per tile of a valid clip), ``pulse``, ``bt``, ``span`` (Python lists over the clips); for all:
    ``block``, ``TILE`` (``beta`` is None: the field of ``DemodPlan`` that ``Demodulation.save`` writes)."""

    def __init__(self, M, fs, offset, rate, carrier, valid, reason, pulse, bt, span, block, TILE):
        self.M, self.fs, self.offset, self.symbol_rate, self.carrier_offset = M, fs, offset, rate, carrier
        self.valid, self.reason, self.block, self.TILE = valid, reason, int(block), int(TILE)
        self.pulse, self.bt, self.span = [str(v) for v in pulse], [float(v) for v in bt], [int(v) for v in span]
        self.beta = None
        n = M.shape[0]
        self.order = np.full(n, 2, dtype=np.int64)
        self.sps = np.full(n, np.nan)
        self.hw, self.n_taps, self.tiles = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        self.Wc, self.Ws, taps = [0] * n, [0] * n, []
        for i in np.flatnonzero(valid):
            sps = float(fs[i]) / float(rate[i])
            hw = half_width(sps, self.pulse[i], self.span[i])
            self.sps[i], self.hw[i], self.n_taps[i] = sps, hw, 2 * hw + 1
            self.tiles[i] = -(-(int(M[i]) - 2 * hw - 1) // self.TILE)
            self.Ws[i] = int(math.ldexp(float(rate[i]) / float(fs[i]), 64))
            self.Wc[i] = int(math.ldexp(float(carrier[i]) / float(fs[i]), 64)) % (1 << 64)
            taps.append(make_taps(sps, hw, self.pulse[i], self.bt[i]))
        self.taps = np.concatenate(taps) if taps else np.zeros(0, dtype=np.float32)
        self.tap_off = np.concatenate(([0], np.cumsum(self.n_taps, dtype=np.int64))).astype(np.int64)
        self.row0 = np.concatenate(([0], np.cumsum(self.tiles, dtype=np.int64))).astype(np.int64)
        self.total_rows = int(self.row0[-1])

    def __len__(self):
        return self.M.shape[0]

    def __repr__(self):
        return f"FskPlan({len(self)} clips, {int(self.valid.sum())} valid, {self.total_rows} tiles of {self.TILE}, {self.taps.shape[0]} taps)"

    def items(self):
        """Every (clip, tile) work item of launch 1 -> (``ITEM`` records with ``row`` into the plan's timing table, the clip of each)."""
        T = self.TILE
        clip = np.repeat(np.arange(len(self), dtype=np.int64), self.tiles)
        b = np.arange(self.total_rows, dtype=np.int64) - self.row0[:-1][clip]
        it = np.zeros(self.total_rows, dtype=ITEM)
        hw = self.hw[clip]
        it["off"], it["len"], it["n0"], it["tap_off"] = self.offset[clip], self.M[clip], hw + 1 + b * T, self.tap_off[:-1][clip]
        it["wc"] = np.array([self.Wc[c] for c in clip], dtype=np.uint64)
        it["ws"] = np.array([self.Ws[c] for c in clip], dtype=np.uint64)
        it["cnt"] = np.minimum(self.M[clip] - 2 * hw - 1 - b * T, T)
        it["hw"], it["n_taps"], it["row"] = hw, self.n_taps[clip], np.arange(self.total_rows)
        it["first"], it["last"] = b == 0, b == self.tiles[clip] - 1
        return it, clip

    def centres(self, i):
        """The tile centres of clip ``i`` (the mean sample index of every tile), float64."""
        hw, T, nt = int(self.hw[i]), self.TILE, int(self.tiles[i])
        n0 = hw + 1 + np.arange(nt, dtype=np.int64) * T
        cnt = np.minimum(int(self.M[i]) - hw - n0, T)
        return n0.astype(np.float64) + (cnt.astype(np.float64) - 1.0) / 2.0


def plan_demodulate_fsk(clips, *, symbol_rate, offset=0.0, pulse="gauss", bt=0.5, span=2, block=32):
    """The ``FskPlan`` of ``clips``: an ``Extraction`` or a pair ``(M, sample_rate)`` of per-clip lengths and rates (scalars broadcast), packed one after the
    other.  ``symbol_rate``, ``offset`` (Hz from the clip's centre), ``pulse``, ``bt`` and ``span``: per clip, scalars broadcast.  ``pulse``: "gauss" (``bt`` in (0, 1],
    ``span`` symbols each side, an integer in [1, 16]) or "rect".  Every argument error is a ``ValueError`` raised here, before anything touches the device; a clip that
    cannot be demodulated is a row with ``valid`` False and a ``reason``."""
    what = "plan_demodulate_fsk"
    if hasattr(clips, "plan") and hasattr(clips, "packed"):
        M, fs, off = np.asarray(clips.plan.M), np.asarray(clips.sample_rate), np.asarray(clips.plan.offset)[:-1]
    else:
        try:
            M, fs = clips
        except (TypeError, ValueError):
            raise ValueError(f"{what}: clips must be an Extraction or a pair (M, sample_rate)") from None
        M, off = np.atleast_1d(np.asarray(M)), None
    if M.ndim != 1 or (M.size and not np.issubdtype(M.dtype, np.integer)) or (M.size and M.min() < 0):
        raise ValueError(f"{what}: the clips' lengths must be a 1-D array of integers >= 0")
    M = M.astype(np.int64)
    n = M.shape[0]
    try:
        fs = _per_clip("sample_rate", fs, n, np.float64)
        if symbol_rate is None or offset is None:
            raise ValueError("plan_demodulate: `symbol_rate` and `offset` must be given")
        rate, carrier = _per_clip("symbol_rate", symbol_rate, n, np.float64), _per_clip("offset", offset, n, np.float64)
    except ValueError as e:
        raise ValueError(str(e).replace("plan_demodulate:", f"{what}:")) from None
    if not (np.isfinite(fs).all() and (fs > 0).all()):
        raise ValueError(f"{what}: every sample rate must be positive and finite")
    if M.size and int(M.max()) >= 2 ** 31:
        raise ValueError(f"{what}: a clip of {int(M.max())} samples is not below 2^31")
    if off is None:
        off = np.concatenate(([0], np.cumsum(M, dtype=np.int64)))[:-1]
    try:
        pulse = np.broadcast_to(np.asarray(pulse, dtype=object), (n,)).copy()
    except ValueError:
        raise ValueError(f"{what}: {n} clips but `pulse` of shape {np.shape(pulse)}") from None
    if not all(isinstance(v, str) and v in PULSES for v in pulse):
        raise ValueError(f"{what}: pulse must be one of {PULSES}, got {pulse.tolist()!r}")

    def number(name, v, lo, hi, integer):
        a = np.asarray(v)
        ok = a.dtype != bool and (np.issubdtype(a.dtype, np.integer) if integer else np.issubdtype(a.dtype, np.integer) or np.issubdtype(a.dtype, np.floating))
        ok = ok and bool(np.isfinite(a.astype(np.float64)).all()) and bool(((a >= lo) & (a <= hi)).all()) and (name != "bt" or bool((a > 0).all()))
        if not ok:
            raise ValueError(f"{what}: {name} must be {'an integer ' if integer else ''}in {'(' if name == 'bt' else '['}{lo}, {hi}], got {v!r}")
        return a
    if np.ndim(block) != 0:
        raise ValueError(f"{what}: block must be one integer in [8, 256], got {block!r}")
    bt, span, block = number("bt", bt, 0.0, 1.0, False), number("span", span, 1, 16, True), int(number("block", block, 8, 256, True))
    try:
        bt, span = _per_clip("bt", bt, n, np.float64), _per_clip("span", span, n, np.int64)
    except ValueError as e:
        raise ValueError(str(e).replace("plan_demodulate:", f"{what}:")) from None
    TILE = tile()
    reason = np.full(n, "", dtype=object)
    for i in range(n):
        if not (math.isfinite(rate[i]) and math.isfinite(carrier[i])) or rate[i] <= 0:
            reason[i] = REASONS["finite"]
        elif not (SPS_MIN <= fs[i] / rate[i] <= SPS_MAX):
            reason[i] = REASONS["sps"]
        elif not abs(carrier[i]) < fs[i] / 2:
            reason[i] = REASONS["offset"]
        elif int(M[i]) < 2 * half_width(fs[i] / rate[i], pulse[i], int(span[i])) + 1 + TILE:
            reason[i] = REASONS["short"]
    valid = reason == ""
    plan = FskPlan(M, fs, off.astype(np.int64), rate, carrier, valid, reason, pulse, bt, span, block, TILE)
    assert int(plan.n_taps.max(initial=0)) <= MAX_TAPS                   # sps <= 16 and span <= 16
    return plan


# ----------------------------------------------------------------------------------------------------------------- host stages
def mean_and_line(rows, usable):
    """A clip's (tiles, 8) rows of launch 1 and its number of usable samples -> (m, T): ``m = sum(sum y) / usable`` and per tile
    ``T_b = (sum y^2 w) - 2 m (sum y w) + m^2 (sum w)``, complex128: the symbol-rate line of ``(y - m)^2``."""
    rows = np.asarray(rows, dtype=np.float64)
    m = float(np.sum(rows[:, 6]) / float(usable))
    A, B, Cw = rows[:, 0] + 1j * rows[:, 1], rows[:, 2] + 1j * rows[:, 3], rows[:, 4] + 1j * rows[:, 5]
    return m, A - 2.0 * m * B + (m * m) * Cw


def level_fit(rows, n_symbols):
    """A clip's (blocks, 4) rows of launch 2 and its number of symbols -> dict: n_hi, n_lo, c_hi, c_lo, f0, dev (cycles per sample), one_tone.  With
    ``one_tone`` (no symbol at or above the mean, or none below it) the levels are NaN."""
    rows = np.asarray(rows, dtype=np.float64)
    n_hi = int(round(float(np.sum(rows[:, 0]))))
    n_lo = int(n_symbols) - n_hi
    if n_hi <= 0 or n_lo <= 0:
        return {"n_hi": n_hi, "n_lo": n_lo, "c_hi": math.nan, "c_lo": math.nan, "f0": math.nan, "dev": math.nan, "one_tone": True}
    c_hi, c_lo = float(np.sum(rows[:, 1])) / n_hi, float(np.sum(rows[:, 2])) / n_lo
    return {"n_hi": n_hi, "n_lo": n_lo, "c_hi": c_hi, "c_lo": c_lo, "f0": (c_hi + c_lo) / 2.0, "dev": (c_hi - c_lo) / 2.0, "one_tone": False}


class FskDemodulation(Demodulation):
    """A ``Demodulation`` at order 2 (every field of it, with the same meaning) whose symbols are real: ``symbols`` holds ``(r, 0)`` around +-1 as complex64,
    ``decisions`` is ``r < 0``, ``filtered`` holds the REAL float32 ``y`` (the filtered discriminator, cycles per sample).  ``valid`` / ``reason`` also
    cover the clips that launch 2 found to hold one tone.  ``phase_ambiguity`` is 2: which tone is "1" is not known.  More columns: ``deviation`` (Hz, half
    the distance of the two tones), ``mod_index`` (``2 deviation / symbol_rate_fit``); ``carrier_fit`` is the midpoint of the two tones.  ``raw`` keeps the
    three device tables (``timing_rows`` (tiles, 8), ``level_rows`` (blocks, 4), ``decision_rows`` (blocks, 3)), the packed ``y`` and the symbols before scaling ``s`` (device,
    float32), ``row0`` / ``block0`` / ``sym0``, per clip ``psi`` (list of arrays), ``T0``, ``STEP``, ``i_first``, ``i_last`` (lists of ints) and ``m``, ``f0``, ``dev`` (arrays,
    cycles per sample, NaN where not known)."""

    COLUMNS = Demodulation.COLUMNS + ("deviation", "mod_index")

    def __init__(self, plan, valid, reason, center_freq, cols, symbols, decisions, filtered, raw, rows=None, cls=None, conf=None, names=None):
        super().__init__(plan, center_freq, cols, symbols, decisions, filtered, raw, rows=rows, cls=cls, conf=conf, names=names)
        self.valid, self.reason = valid, reason
        self.phase_ambiguity = np.where(valid, 2, -1)

    def save(self, directory):
        """What ``Demodulation.save`` writes (``demodulate.npz``, ``symbols_<row>.cf32`` per valid clip, ``demodulate.json``), with the columns ``deviation`` and
        ``mod_index`` in both files and ``pulse`` / ``bt`` in the index.  -> the directory."""
        directory = super().save(directory)
        path = os.path.join(directory, "demodulate.json")
        with open(path) as f:
            index = json.load(f)
        index.update(modulation="fsk", pulse=self.plan.pulse, bt=self.plan.bt)
        with open(path, "w") as f:
            json.dump(index, f, indent=1)
        return directory


def demodulate_fsk_extraction(extraction, *, symbol_rate, offset=0.0, pulse="gauss", bt=0.5, span=2, block=32):
    """Demodulate every clip of ``extraction`` (``sy11.data.extract.Extraction``) as 2-FSK / GFSK / GMSK -> ``FskDemodulation``: three launches over all
    clips, three small copies to the host (the timing rows, the level rows, the decision rows); an extraction without a valid clip launches
    nothing, one whose clips all hold one tone skips the third launch."""
    from .. import ops
    plan = plan_demodulate_fsk(extraction, symbol_rate=symbol_rate, offset=offset, pulse=pulse, bt=bt, span=span, block=block)
    n, packed = len(plan), extraction.packed
    dev = packed.device
    meta = dict(rows=extraction.rows, cls=extraction.cls, conf=extraction.conf, names=extraction.names)
    cols = {k: np.full(n, np.nan) for k in FskDemodulation.COLUMNS}
    cols["n_symbols"] = np.full(n, -1, dtype=np.int64)
    fc = np.broadcast_to(np.asarray(extraction.center_freq, dtype=np.float64), (n,))
    valid, reason = plan.valid.copy(), plan.reason.copy()
    empty_c, empty_u, empty_f = (torch.zeros(0, dtype=t, device=dev) for t in (torch.complex64, torch.uint8, torch.float32))
    raw = {"timing_rows": None, "level_rows": None, "decision_rows": None, "y": None, "s": None, "row0": plan.row0, "block0": np.zeros(n + 1, dtype=np.int64),
           "sym0": np.zeros(n + 1, dtype=np.int64), "psi": [np.zeros(0)] * n, "T0": [0] * n, "STEP": [0] * n, "i_first": [0] * n, "i_last": [-1] * n,
           "m": np.full(n, np.nan), "f0": np.full(n, np.nan), "dev": np.full(n, np.nan)}
    if plan.total_rows == 0:
        return FskDemodulation(plan, valid, reason, fc, cols, [empty_c] * n, [empty_u] * n, [empty_f] * n, raw, **meta)
    # launch 1: discriminator, post-detection filter, timing partials
    taps = torch.from_numpy(plan.taps).to(dev)
    y = torch.zeros(packed.shape[0], dtype=torch.float32, device=dev)
    trows = torch.empty((plan.total_rows, 8), dtype=torch.float64, device=dev)
    ops.iq_fsk_filter(packed, plan.items()[0], taps, y, trows)
    th = trows.cpu().numpy()
    # the mean and the timing fit
    v = np.flatnonzero(plan.valid)
    fits = {}
    nsym, nblk = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for i in v:
        hw, M = int(plan.hw[i]), int(plan.M[i])
        m, T = mean_and_line(th[int(plan.row0[i]):int(plan.row0[i + 1])], M - 2 * hw - 1)
        fits[i] = f = fit(T, plan.centres(i), plan.Ws[i], M, hw + 1)
        nsym[i], nblk[i], raw["m"][i] = f["n_symbols"], -(-f["n_symbols"] // plan.block), m
        raw["psi"][i], raw["T0"][i], raw["STEP"][i], raw["i_first"][i], raw["i_last"][i] = f["psi"], f["T0"], f["STEP"], f["i_first"], f["i_last"]
    sym0 = np.concatenate(([0], np.cumsum(nsym))).astype(np.int64)
    block0 = np.concatenate(([0], np.cumsum(nblk))).astype(np.int64)
    raw["sym0"], raw["block0"] = sym0, block0
    n_sym, n_blk = int(sym0[-1]), int(block0[-1])
    # launch 2: the symbols and the level sums
    bl = np.zeros(n_blk, dtype=BLOCK)
    for i in v:
        f, a, b = fits[i], int(block0[i]), int(block0[i + 1])
        q = np.arange(b - a, dtype=np.int64)
        bl["off"][a:b], bl["len"][a:b], bl["step"][a:b], bl["m"][a:b] = plan.offset[i], plan.M[i], f["STEP"], raw["m"][i]
        bl["t0"][a:b] = [f["T0"] + (f["i_first"] + int(k) * plan.block) * f["STEP"] for k in q]
        bl["sym_off"][a:b], bl["n"][a:b], bl["row"][a:b] = sym0[i] + q * plan.block, np.minimum(nsym[i] - q * plan.block, plan.block), a + q
    s = torch.zeros(n_sym, dtype=torch.float32, device=dev)
    lrows = torch.empty((n_blk, 4), dtype=torch.float64, device=dev)
    ops.fsk_symbols(y, bl, s, lrows)
    lh = lrows.cpu().numpy()
    # the two levels
    live = []
    for i in v:
        lv = level_fit(lh[int(block0[i]):int(block0[i + 1])], int(nsym[i]))
        if lv["one_tone"]:
            valid[i], reason[i] = False, REASONS["tone"]
        else:
            raw["f0"][i], raw["dev"][i] = lv["f0"], lv["dev"]
            live.append(i)
    # launch 3: the decisions (the rows of a clip of one tone stay zero)
    r = torch.zeros(n_sym, dtype=torch.complex64, device=dev)
    d = torch.zeros(n_sym, dtype=torch.uint8, device=dev)
    drows = torch.zeros((n_blk, 3), dtype=torch.float64, device=dev)
    if live:
        de = np.zeros(int(sum(nblk[i] for i in live)), dtype=DEC)
        at = 0
        for i in live:
            a, b = int(block0[i]), int(block0[i + 1])
            k = slice(at, at + b - a)
            de["sym_off"][k], de["n"][k], de["row"][k], de["f0"][k], de["dev"][k] = bl["sym_off"][a:b], bl["n"][a:b], bl["row"][a:b], raw["f0"][i], raw["dev"][i]
            at += b - a
        ops.fsk_decide(s, de, r, d, drows)
        dh = drows.cpu().numpy()
        for i in live:
            a, b = int(block0[i]), int(block0[i + 1])
            f, fs = fits[i], float(plan.fs[i])
            rate_fit = fs / f["sps"]
            c = columns(dh[a:b], np.zeros(b - a), block_centres(int(nsym[i]), plan.block), rate_fit, float(fc[i]) + float(plan.carrier_offset[i]) + raw["f0"][i] * fs)
            for k in ("n_symbols", "gain", "evm", "mer_db", "carrier_fit"):
                cols[k][i] = c[k]
            cols["timing"][i], cols["symbol_rate_fit"][i] = f["timing"], rate_fit
            cols["deviation"][i] = raw["dev"][i] * fs
            cols["mod_index"][i] = 2.0 * cols["deviation"][i] / rate_fit
    raw.update(timing_rows=trows, level_rows=lrows, decision_rows=drows, y=y, s=s)
    off = plan.offset
    symbols = [r[int(sym0[i]):int(sym0[i + 1])] if valid[i] else empty_c for i in range(n)]
    decisions = [d[int(sym0[i]):int(sym0[i + 1])] if valid[i] else empty_u for i in range(n)]
    filtered = [y[int(off[i]):int(off[i]) + int(plan.M[i])] if valid[i] else empty_f for i in range(n)]
    return FskDemodulation(plan, valid, reason, fc, cols, symbols, decisions, filtered, raw, **meta)
