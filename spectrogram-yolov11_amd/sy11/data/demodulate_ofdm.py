"""Demodulate every cyclic-prefix OFDM clip of an extraction on the GPU, feed-forward: the host plan of ``csrc/demod_ofdm.hip`` (the prefix correlation
folded over the OFDM period in ONE launch over all clips; the de-rotated FFT of every OFDM symbol, its used carriers, pilot rows and power in a second; the
data carriers turned by the pilots' fit and the decisions in a third), the two small float64 fits between the launches, and
``demodulate_ofdm_extraction``.  The result is a ``Demodulation`` at the clips' order, so ``find_frames``, ``equalize``, ``decode``, ``decode_ldpc`` and ``correct``
take it as it is.

Definition.  Clip ``i`` is ``x[0 .. M)`` at ``fs = N df`` Hz: FFT size ``N``, prefix ``G``, period ``S = N + G``, ``L = (M - N) // S`` whole periods,
advance ``a`` (the samples the FFT window starts inside the prefix).

    launch 1  per residue r of the period, the periods in ascending order:  F[r] = sum_m x[r + m S + N] conj(x[r + m S]),
              E[r] = sum_m (|x[r + m S]|^2 + |x[r + m S + N]|^2) / 2;  the periods are split FOLD_PERIODS at a time: one partial row per split, added here in ascending order
    fit 1     Gamma[r] = sum_{j < G} F[(r + j) mod S], Phi likewise from E;  theta = the first argmax |Gamma|;  eps = arg(Gamma[theta]) / 2 pi (carrier spacings; with an
              ``offset`` the turn e^{-2 pi i N offset / fs} is taken off Gamma[theta] first);  cp_corr = |Gamma[theta]| / Phi[theta] (0 when Phi = 0)
              W = round((offset / fs + eps / N) 2^64) mod 2^64;  OFDM symbol m, any integer, starts at theta + G - a + m S where that window lies inside the clip
    launch 2  v[q] = x[start + q] e^{-2 pi i ((start + q) W mod 2^64) 2^-64};  Y[k] = FFT_N(v)[k] e^{+2 pi i k a / N};  Yc = f32(Y) on the used carriers (ascending k),
              u_p = Y[k_p] c_p (float64),  sum over the used carriers of |Y|^2 (float64)
    fit 2     beta = arg(sum_m sum_p u_{m,p+1} conj(u_{m,p})) / d;  z_m = sum_p u_{m,p} e^{-i beta k_p};  phi_m = arg z_m;  active_m = |z_m| >= max |z| / 2;
              A = mean |u| over the active symbols;  rho_m = e^{-i phi_m} / A (0 when A = 0);  tau_j = e^{-i beta k_j}
    launch 3  r = f32((Yc rho_m) tau_j) on the data carriers, the decisions of ``demodulate``, per OFDM symbol sum |r|^2, sum Re(r conj(point(d))), n_data
    columns   gain, evm, mer_db by ``demodulate.columns``' rule over the ACTIVE symbols;  timing = theta;  cfo = eps;  carrier_fit = fc + offset + eps df;  cp_corr;
              slope = beta;  n_ofdm, n_active;  symbol_rate_fit = n_data fs / S

The pilots fix the phase: ``phase_ambiguity`` is 1, and ``find_frames`` finds a frame at rotation 0.

Out of scope: pilots that change from OFDM symbol to OFDM symbol, non-uniform pilot spacing, a per-carrier channel estimate and frequency-selective
equalisation, a search over whole carrier spacings, sampling-clock offset and clip rates other than ``N df``, 16-QAM and above, interleaver and scrambler, N
above 1024, and the two fits on the device.
"""
from __future__ import annotations

import json
import math
import os
from collections.abc import Mapping

import numpy as np
import torch

from .demodulate import Demodulation, _per_clip, columns

FOLD_TILE, FOLD_PERIODS, FFT_SLOTS = 64, 16, 1024             # constants of csrc/demod_ofdm.hip; its entries refuse a table that breaks them
N_FFT = (64, 128, 256, 512, 1024)

# laid out as sy11_ofdm_fold_item / sy11_ofdm_bin / sy11_ofdm_fft_item / sy11_ofdm_car / sy11_ofdm_dec (include/sy11.h)
FOLD = np.dtype([("off", "<i8"), ("len", "<i8"), ("out_off", "<i8"), ("n_fft", "<i4"), ("S", "<i4"), ("r0", "<i4"), ("cnt_r", "<i4"), ("m0", "<i4"), ("cnt_m", "<i4")])
BIN = np.dtype([("k", "<i4"), ("pil", "<i4")])
FFT = np.dtype([("off", "<i8"), ("len", "<i8"), ("start", "<i8"), ("w", "<u8"), ("yc_off", "<i8"), ("pil_off", "<i8"), ("pow_off", "<i8"), ("n_fft", "<i4"), ("S", "<i4"),
                ("a", "<i4"), ("nf", "<i4"), ("bin_off", "<i4"), ("n_used", "<i4"), ("n_pil", "<i4"), ("reserved", "<i4")])
CAR = np.dtype([("idx", "<i4"), ("reserved", "<i4"), ("tr", "<f8"), ("ti", "<f8")])
DEC = np.dtype([("yc_off", "<i8"), ("sym_off", "<i8"), ("rho_r", "<f8"), ("rho_i", "<f8"), ("car_off", "<i4"), ("n_data", "<i4"), ("n_used", "<i4"), ("order", "<i4"),
                ("row", "<i4"), ("reserved", "<i4")])

REASONS = ("order", "rate", "offset", "short")


def twiddle_table():
    """e^{-2 pi i m / 1024}, m < 512, complex128: the table of every N is a stride of it."""
    m = np.arange(FFT_SLOTS // 2, dtype=np.float64)
    return np.cos(2.0 * np.pi * m / FFT_SLOTS) - 1j * np.sin(2.0 * np.pi * m / FFT_SLOTS)


class OfdmLayout:
    """One carrier layout: ``n_fft``, ``cp``, ``S``, ``advance``, ``carriers`` (the data carriers, signed, ascending), ``pilot_k`` / ``pilot_c`` (ascending k, values
    +-1), ``d`` (the pilots' spacing), ``used`` (data and pilots, ascending), ``data_idx`` / ``pilot_idx`` (their places in ``used``), ``bins`` (``BIN`` records)."""

    def __init__(self, n_fft, cp, advance, carriers, pilot_k, pilot_c):
        self.n_fft, self.cp, self.S, self.advance = int(n_fft), int(cp), int(n_fft) + int(cp), int(advance)
        self.carriers, self.pilot_k, self.pilot_c = carriers, pilot_k, pilot_c
        self.d = int(pilot_k[1] - pilot_k[0])
        self.used = np.sort(np.concatenate((carriers, pilot_k)))
        self.data_idx, self.pilot_idx = np.searchsorted(self.used, carriers), np.searchsorted(self.used, pilot_k)
        self.n_data, self.n_pil, self.n_used = carriers.shape[0], pilot_k.shape[0], self.used.shape[0]
        self.bins = np.zeros(self.n_used, dtype=BIN)
        self.bins["k"] = self.used
        self.bins["pil"][self.pilot_idx] = (np.arange(self.n_pil) + 1) * pilot_c
        self.group = FFT_SLOTS // self.n_fft                                  # OFDM symbols per item of launch 2

    def key(self):
        return (self.n_fft, self.cp, self.advance, self.carriers.tobytes(), self.pilot_k.tobytes(), self.pilot_c.tobytes())


def _integer(what, name, v, lo, hi):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError(f"{what}: {name} must be an integer in [{lo}, {hi}], got {v!r}")
    return int(v)


def _int_vector(what, name, v):
    a = np.asarray(v)
    if a.ndim != 1 or a.size == 0 or a.dtype == bool or not (np.issubdtype(a.dtype, np.integer) or (np.issubdtype(a.dtype, np.floating) and np.isfinite(a).all() and
                                                                                                  (a == np.round(a)).all())):
        raise ValueError(f"{what}: {name} must be a non-empty 1-D array of integers, got {v!r}")
    return a.astype(np.int64)


def make_layout(n_fft, cp, carriers, pilots, advance=None, what="plan_demodulate_ofdm"):
    """Check one layout's arguments (a ``ValueError`` names the first that is wrong) -> ``OfdmLayout``."""
    if isinstance(n_fft, (bool, np.bool_)) or not isinstance(n_fft, (int, np.integer)) or int(n_fft) not in N_FFT:
        raise ValueError(f"{what}: n_fft must be one of {N_FFT}, got {n_fft!r}")
    N = int(n_fft)
    G = _integer(what, "cp", cp, 1, N // 2)
    a = G // 4 if advance is None else _integer(what, "advance", advance, 0, G)
    k = _int_vector(what, "carriers", carriers)
    if np.unique(k).shape[0] != k.shape[0] or k.min() <= -N // 2 or k.max() >= N // 2:
        raise ValueError(f"{what}: carriers must be unique and inside (-{N // 2}, {N // 2})")
    if isinstance(pilots, Mapping):
        pk, pc = list(pilots.keys()), list(pilots.values())
    else:
        try:
            pk, pc = pilots
        except (TypeError, ValueError):
            raise ValueError(f"{what}: pilots must be a mapping k -> +-1 or a pair of arrays (k_p, c_p)") from None
    pk, pc = _int_vector(what, "the pilots' carriers", pk), _int_vector(what, "the pilots' values", pc)
    if pk.shape != pc.shape or pk.shape[0] < 2:
        raise ValueError(f"{what}: need at least 2 pilots, each with a value; got {pk.shape[0]} carriers and {pc.shape[0]} values")
    if not np.isin(pc, (1, -1)).all():
        raise ValueError(f"{what}: every pilot value must be +1 or -1, got {pc.tolist()!r}")
    o = np.argsort(pk, kind="stable")
    pk, pc = pk[o], pc[o]
    if np.unique(pk).shape[0] != pk.shape[0] or pk.min() <= -N // 2 or pk.max() >= N // 2:
        raise ValueError(f"{what}: the pilots' carriers must be unique and inside (-{N // 2}, {N // 2})")
    if np.isin(pk, k).any():
        raise ValueError(f"{what}: carriers {pk[np.isin(pk, k)].tolist()} are both data and pilot")
    step = np.diff(pk)
    if not (step == step[0]).all():
        raise ValueError(f"{what}: the pilots must be uniformly spaced, got the steps {step.tolist()}")
    return OfdmLayout(N, G, a, np.sort(k), pk, pc)


def _is_pair(p):
    try:
        return not isinstance(p, Mapping) and len(p) == 2 and all(np.ndim(v) == 1 for v in p) and all(np.ndim(e) == 0 for v in p for e in v)
    except TypeError:
        return False


class OfdmPlan:
    """Per clip: ``M``, ``fs``, ``offset`` (first sample in the packed buffer), ``carrier_offset`` (Hz), ``order``, ``valid`` and ``reason`` ("" when valid), ``layout`` (index into
    ``layouts``), ``periods`` (L), ``splits`` (= ceil(L / FOLD_PERIODS): the split rule of launch 1 depends on the clip alone) and ``tiles`` (= ceil(S / FOLD_TILE)), ``fold0`` (k + 1
    offsets into the fold table, in triples: ``splits * S`` per valid clip); ``layouts``: the distinct ``OfdmLayout``s, ``bin0``: their k + 1 offsets into ``bins``."""

    def __init__(self, M, fs, offset, carrier, order, valid, reason, layouts, layout):
        self.M, self.fs, self.offset, self.carrier_offset, self.order = M, fs, offset, carrier, order
        self.valid, self.reason, self.layouts, self.layout = valid, reason, layouts, layout
        n = M.shape[0]
        self.periods, self.splits, self.tiles = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        rows = np.zeros(n, dtype=np.int64)
        for i in np.flatnonzero(valid):
            lay = layouts[layout[i]]
            self.periods[i] = (int(M[i]) - lay.n_fft) // lay.S
            self.splits[i], self.tiles[i] = -(-int(self.periods[i]) // FOLD_PERIODS), -(-lay.S // FOLD_TILE)
            rows[i] = self.splits[i] * lay.S
        self.fold0 = np.concatenate(([0], np.cumsum(rows))).astype(np.int64)
        self.total_triples = int(self.fold0[-1])
        self.bins = np.concatenate([lay.bins for lay in layouts]) if layouts else np.zeros(0, dtype=BIN)
        self.bin0 = np.concatenate(([0], np.cumsum([lay.n_used for lay in layouts]))).astype(np.int64)

    def __len__(self):
        return self.M.shape[0]

    def __repr__(self):
        return f"OfdmPlan({len(self)} clips, {int(self.valid.sum())} valid, {len(self.layouts)} layouts, {self.total_triples} fold triples)"

    def lay(self, i):
        return self.layouts[self.layout[i]]

    def items(self):
        """Every (clip, split, tile) work item of launch 1 -> ``FOLD`` records with ``out_off`` into the plan's fold table."""
        out = []
        for i in np.flatnonzero(self.valid):
            lay, L = self.lay(i), int(self.periods[i])
            sp, tl = np.meshgrid(np.arange(self.splits[i]), np.arange(self.tiles[i]), indexing="ij")
            sp, tl = sp.reshape(-1), tl.reshape(-1)
            it = np.zeros(sp.shape[0], dtype=FOLD)
            it["off"], it["len"], it["n_fft"], it["S"] = self.offset[i], self.M[i], lay.n_fft, lay.S
            it["r0"], it["cnt_r"] = tl * FOLD_TILE, np.minimum(lay.S - tl * FOLD_TILE, FOLD_TILE)
            it["m0"], it["cnt_m"] = sp * FOLD_PERIODS, np.minimum(L - sp * FOLD_PERIODS, FOLD_PERIODS)
            it["out_off"] = self.fold0[i] + sp * lay.S + tl * FOLD_TILE
            out.append(it)
        return np.concatenate(out) if out else np.zeros(0, dtype=FOLD)


def plan_demodulate_ofdm(clips, *, n_fft, cp, carriers, pilots, order=4, offset=0.0, spacing=None, advance=None):
    """The ``OfdmPlan`` of ``clips``: an ``Extraction`` or a pair ``(M, sample_rate)`` of per-clip lengths and rates (scalars broadcast), packed one after the other.
    ``n_fft``, ``cp``, ``advance`` (default ``cp // 4``): integers, or one per clip.  ``carriers``: the data carriers, signed integers, or one array per clip (a list).
    ``pilots``: a mapping k -> +-1 or a pair ``(k_p, c_p)``, at least 2, uniformly spaced, disjoint from the carriers; or one of those per clip (a list).  ``order`` (2 or 4) and
    ``offset`` (Hz from the clip's centre, right to within half a carrier spacing): per clip, scalars broadcast.  ``spacing``: the carrier spacing in Hz; when given, a clip whose rate
    is not ``n_fft * spacing`` to 1e-6 is invalid.  Every argument error is a ``ValueError`` raised here, before anything touches the device; a clip that cannot be demodulated is a
    row with ``valid`` False and a ``reason``: "order", "rate", "offset" (|offset| >= fs / 2) or "short" (fewer than 2 whole periods)."""
    what = "plan_demodulate_ofdm"
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
        if offset is None or order is None:
            raise ValueError("plan_demodulate: `order` and `offset` must be given")
        carrier = _per_clip("offset", offset, n, np.float64)
        o = np.asarray(order)
        if o.dtype == bool or (o.size and not (np.issubdtype(o.dtype, np.integer) or (np.issubdtype(o.dtype, np.floating) and np.isfinite(o).all() and (o == np.round(o)).all()))):
            raise ValueError("plan_demodulate: `order` must hold integers")
        order = _per_clip("order", order, n, np.int64)
        sp = None if spacing is None else _per_clip("spacing", spacing, n, np.float64)
    except ValueError as e:
        raise ValueError(str(e).replace("plan_demodulate:", f"{what}:")) from None
    if not (np.isfinite(fs).all() and (fs > 0).all()):
        raise ValueError(f"{what}: every sample rate must be positive and finite")
    if not np.isfinite(carrier).all():
        raise ValueError(f"{what}: every offset must be finite")
    if sp is not None and not (np.isfinite(sp).all() and (sp > 0).all()):
        raise ValueError(f"{what}: every spacing must be positive and finite")
    if M.size and int(M.max()) >= 2 ** 31:
        raise ValueError(f"{what}: a clip of {int(M.max())} samples is not below 2^31")
    if off is None:
        off = np.concatenate(([0], np.cumsum(M, dtype=np.int64)))[:-1]

    def each(name, v, scalar):
        """``v`` for every clip: itself where it is one value (``scalar`` says so), else one entry per clip."""
        if scalar(v):
            return [v] * n
        try:
            v = list(v)
        except TypeError:
            v = None
        if v is None or len(v) != n:
            raise ValueError(f"{what}: {n} clips but `{name}` is neither one value nor one per clip")
        return v
    one_number = lambda v: np.ndim(v) == 0                                    # noqa: E731
    nf, cps = each("n_fft", n_fft, one_number), each("cp", cp, one_number)
    adv = each("advance", advance, lambda v: v is None or np.ndim(v) == 0)
    car = each("carriers", carriers, lambda v: not isinstance(v, (list, tuple)) or len(v) == 0 or np.ndim(v[0]) == 0)
    pil = each("pilots", pilots, lambda v: isinstance(v, Mapping) or _is_pair(v) or not isinstance(v, (list, tuple)))
    layouts, layout, known, checked = [], np.zeros(n, dtype=np.int64), {}, {}
    for i in range(n):
        ident = (id(nf[i]), id(cps[i]), id(adv[i]), id(car[i]), id(pil[i]))      # the shared arguments are checked once
        if ident not in checked:
            lay = make_layout(nf[i], cps[i], car[i], pil[i], adv[i], what)
            checked[ident] = known.setdefault(lay.key(), len(layouts))
            if checked[ident] == len(layouts):
                layouts.append(lay)
        layout[i] = checked[ident]
    reason = np.full(n, "", dtype=object)
    for i in range(n):
        lay = layouts[layout[i]]
        if order[i] not in (2, 4):
            reason[i] = "order"
        elif sp is not None and abs(fs[i] / (lay.n_fft * sp[i]) - 1.0) > 1e-6:
            reason[i] = "rate"
        elif not abs(carrier[i]) < fs[i] / 2:
            reason[i] = "offset"
        elif (int(M[i]) - lay.n_fft) // lay.S < 2:
            reason[i] = "short"
    return OfdmPlan(M, fs, off.astype(np.int64), carrier, order, reason == "", reason, layouts, layout)


# ----------------------------------------------------------------------------------------------------------------- host stages
def fold_rows(partial):
    """A clip's (splits, S, 3) partial rows of launch 1 -> (F (S,) complex128, E (S,) float64): the rows added in ascending order."""
    partial = np.asarray(partial, dtype=np.float64)
    acc = partial[0].copy()
    for row in partial[1:]:
        acc = acc + row
    return acc[:, 0] + 1j * acc[:, 1], acc[:, 2].copy()


def fit1(F, E, n_fft, cp, offset_cycles=0.0):
    """The prefix fit of one clip: ``F`` (S,) complex128, ``E`` (S,) float64 -> dict: Gamma, Phi (S,), theta (int), eps (carrier spacings), cp_corr.  ``offset_cycles``: the
    caller's offset in cycles per sample; its turn over N samples is taken off Gamma[theta] before the angle is read (nothing is done for 0)."""
    F, E = np.asarray(F, dtype=np.complex128), np.asarray(E, dtype=np.float64)
    S = F.shape[0]
    gam, phi = np.zeros(S, dtype=np.complex128), np.zeros(S, dtype=np.float64)
    idx = np.arange(S)
    for j in range(int(cp)):                                                  # ascending j
        gam = gam + F[(idx + j) % S]
        phi = phi + E[(idx + j) % S]
    theta = int(np.argmax(np.abs(gam)))                                       # the first maximum
    g = complex(gam[theta])
    if offset_cycles != 0.0:
        t = -2.0 * math.pi * ((offset_cycles * n_fft) % 1.0)
        g = g * complex(math.cos(t), math.sin(t))
    eps = math.atan2(g.imag, g.real) / (2.0 * math.pi)
    corr = float(abs(gam[theta]) / phi[theta]) if phi[theta] > 0 else 0.0
    return {"Gamma": gam, "Phi": phi, "theta": theta, "eps": eps, "cp_corr": corr}


def carrier_word(offset_cycles, eps, n_fft):
    """W = round((offset / fs + eps / N) 2^64) mod 2^64, a Python int."""
    return int(round(math.ldexp(offset_cycles + eps / n_fft, 64))) % (1 << 64)


def symbol_starts(theta, M, lay):
    """-> (start of the first FFT window, n_ofdm): every integer m with 0 <= theta + G - a + m S and that + N <= M."""
    base = int(theta) + lay.cp - lay.advance
    first = base % lay.S
    return first, (int(M) - lay.n_fft - first) // lay.S + 1


def fit2(u, lay):
    """The pilot fit of one clip: ``u`` (n_ofdm, P) complex128 -> dict: beta, z, phi, active (n_ofdm,), A, rho (n_ofdm,) complex128, tau (n_data,) complex128."""
    u = np.asarray(u, dtype=np.complex128)
    kp, kd = lay.pilot_k.astype(np.float64), lay.carriers.astype(np.float64)
    c = complex(np.sum(u[:, 1:] * np.conj(u[:, :-1])))
    beta = math.atan2(c.imag, c.real) / lay.d
    z = np.sum(u * np.exp(-1j * beta * kp)[None, :], axis=1)
    phi, mag = np.arctan2(z.imag, z.real), np.abs(z)
    active = mag >= 0.5 * np.max(mag)
    A = float(np.mean(np.abs(u[active])))
    rho = np.exp(-1j * phi) / A if A > 0 else np.zeros(u.shape[0], dtype=np.complex128)
    return {"beta": beta, "z": z, "phi": phi, "active": active, "A": A, "rho": rho, "tau": np.exp(-1j * beta * kd)}


class OfdmDemodulation(Demodulation):
    """A ``Demodulation`` at the clips' ``order`` (every field of it, with the same meaning).  ``symbols[i]`` / ``decisions[i]`` hold ``n_ofdm * n_data`` entries: OFDM symbol after
    OFDM symbol, the data carriers ascending, the inactive symbols included, so that a position still maps to a time.  ``filtered[i]`` is the clip's ``(n_ofdm, n_used)`` view of
    ``Yc``.  ``phase_ambiguity`` is 1: the pilots fix the phase.  ``timing`` is theta (samples).  More columns: ``cfo`` (eps, carrier spacings), ``cp_corr``, ``slope`` (beta, radians per
    carrier), ``n_ofdm``, ``n_active``.  ``raw``: the device buffers ``fold`` (triples), ``yc``, ``pilots`` (complex128), ``power``, ``decision_rows`` (one row per OFDM symbol), ``bins``,
    ``cars``, ``twiddle``, and ``tables``: the host copies of the five item and carrier tables the launches were given; ``fold0`` / ``yc0`` / ``pil0`` / ``pow0`` / ``sym0`` (k + 1 offsets of the clips into them); per clip ``F``, ``E``, ``phi``, ``active``, ``z`` (lists of arrays),
    ``start`` (the first FFT window), ``W``, ``T0``, ``STEP``, ``i_first`` (lists of ints) and ``theta``, ``eps``, ``beta``, ``A`` (arrays)."""

    COLUMNS = Demodulation.COLUMNS + ("cfo", "cp_corr", "slope", "n_ofdm", "n_active")

    def __init__(self, plan, center_freq, cols, symbols, decisions, filtered, raw, rows=None, cls=None, conf=None, names=None):
        super().__init__(plan, center_freq, cols, symbols, decisions, filtered, raw, rows=rows, cls=cls, conf=conf, names=names)
        self.phase_ambiguity = np.where(plan.valid, 1, -1)

    def save(self, directory):
        """Write ``demodulate_ofdm.npz`` (every column, and per valid clip its decisions and ``active``), ``symbols_<row>.cf32`` (raw interleaved float32) per valid clip and
        ``demodulate_ofdm.json``, which lists per clip its row, class, confidence, layout and scalars.  -> the directory."""
        directory = os.fspath(directory)
        os.makedirs(directory, exist_ok=True)
        rows = np.arange(len(self)) if self.rows is None else np.asarray(self.rows)
        arrays = {k: getattr(self, k) for k in self.COLUMNS + ("n_symbols", "order", "valid", "phase_ambiguity", "sample_rate", "center_freq")}
        arrays.update(rows=rows, reason=np.asarray([str(r) for r in self.reason], dtype=str))
        out = []
        for i in range(len(self)):
            row, name, lay = int(rows[i]), None, self.plan.lay(i)
            if self.valid[i]:
                name = f"symbols_{row}.cf32"
                self.symbols[i].cpu().numpy().view(np.float32).tofile(os.path.join(directory, name))
                arrays[f"decisions_{row}"] = self.decisions[i].cpu().numpy()
                arrays[f"active_{row}"] = np.asarray(self.raw["active"][i])
            cls = None if self.cls is None else int(self.cls[i])
            rec = {"row": row, "valid": bool(self.valid[i]), "reason": str(self.reason[i]), "file": name, "order": int(self.order[i]),
                   "phase_ambiguity": int(self.phase_ambiguity[i]), "n_symbols": int(self.n_symbols[i]), "class": cls,
                   "name": None if cls is None or not self.names else self.names.get(cls),
                   "confidence": None if self.conf is None else float(self.conf[i]), "sample_rate": float(self.sample_rate[i]),
                   "center_freq": float(self.center_freq[i]), "n_fft": lay.n_fft, "cp": lay.cp, "advance": lay.advance, "n_data": lay.n_data, "n_pilots": lay.n_pil}
            for k in self.COLUMNS:
                v = float(getattr(self, k)[i])
                rec[k] = v if math.isfinite(v) else None
            out.append(rec)
        np.savez(os.path.join(directory, "demodulate_ofdm.npz"), **arrays)
        with open(os.path.join(directory, "demodulate_ofdm.json"), "w") as f:
            json.dump({"modulation": "ofdm", "fold_tile": FOLD_TILE, "fold_periods": FOLD_PERIODS, "file": "demodulate_ofdm.npz", "clips": out}, f, indent=1)
        return directory


def demodulate_ofdm_extraction(extraction, *, n_fft, cp, carriers, pilots, order=4, offset=0.0, spacing=None, advance=None):
    """Demodulate every clip of ``extraction`` (``sy11.data.extract.Extraction``) as cyclic-prefix OFDM -> ``OfdmDemodulation``: three launches over all clips, two small
    copies to the host between them (the fold rows, the pilot rows) and one after (the decision rows); an extraction without a valid clip launches nothing."""
    from .. import ops
    plan = plan_demodulate_ofdm(extraction, n_fft=n_fft, cp=cp, carriers=carriers, pilots=pilots, order=order, offset=offset, spacing=spacing, advance=advance)
    n, packed = len(plan), extraction.packed
    dev = packed.device
    meta = dict(rows=extraction.rows, cls=extraction.cls, conf=extraction.conf, names=extraction.names)
    cols = {k: np.full(n, np.nan) for k in OfdmDemodulation.COLUMNS}
    for k in ("n_symbols", "n_ofdm", "n_active"):
        cols[k] = np.full(n, -1, dtype=np.int64)
    fc = np.broadcast_to(np.asarray(extraction.center_freq, dtype=np.float64), (n,))
    empty_c, empty_u = torch.zeros(0, dtype=torch.complex64, device=dev), torch.zeros(0, dtype=torch.uint8, device=dev)
    zeros = lambda: np.zeros(n + 1, dtype=np.int64)                           # noqa: E731
    raw = {"fold": None, "yc": None, "pilots": None, "power": None, "decision_rows": None, "bins": None, "cars": None, "twiddle": None, "tables": None, "fold0": plan.fold0, "yc0": zeros(),
           "pil0": zeros(), "pow0": zeros(), "sym0": zeros(), "F": [np.zeros(0, dtype=np.complex128)] * n, "E": [np.zeros(0)] * n, "phi": [np.zeros(0)] * n,
           "active": [np.zeros(0, dtype=bool)] * n, "z": [np.zeros(0, dtype=np.complex128)] * n, "start": [0] * n, "W": [0] * n, "T0": [0] * n, "STEP": [0] * n,
           "i_first": [0] * n, "theta": np.full(n, -1, dtype=np.int64), "eps": np.full(n, np.nan), "beta": np.full(n, np.nan), "A": np.full(n, np.nan)}
    if plan.total_triples == 0:
        return OfdmDemodulation(plan, fc, cols, [empty_c] * n, [empty_u] * n, [empty_c] * n, raw, **meta)
    v = np.flatnonzero(plan.valid)
    # launch 1: the prefix correlation and the energy, folded over the period
    fold = torch.empty((plan.total_triples, 3), dtype=torch.float64, device=dev)
    fold_items = plan.items()
    ops.iq_ofdm_fold(packed, fold_items, fold)
    fh = fold.cpu().numpy()
    # fit 1: where the prefix starts, the fractional carrier offset, the OFDM symbols
    n_ofdm = np.zeros(n, dtype=np.int64)
    for i in v:
        lay, fs = plan.lay(i), float(plan.fs[i])
        F, E = fold_rows(fh[int(plan.fold0[i]):int(plan.fold0[i + 1])].reshape(int(plan.splits[i]), lay.S, 3))
        cyc = float(plan.carrier_offset[i]) / fs
        f = fit1(F, E, lay.n_fft, lay.cp, cyc)
        raw["F"][i], raw["E"][i], raw["theta"][i], raw["eps"][i], raw["W"][i] = F, E, f["theta"], f["eps"], carrier_word(cyc, f["eps"], lay.n_fft)
        raw["start"][i], n_ofdm[i] = symbol_starts(f["theta"], plan.M[i], lay)
        raw["T0"][i], raw["STEP"][i] = raw["start"][i] << 32, int(round(math.ldexp(lay.S / lay.n_data, 32)))
        cols["timing"][i], cols["cfo"][i], cols["cp_corr"][i], cols["n_ofdm"][i] = f["theta"], f["eps"], f["cp_corr"], n_ofdm[i]
        cols["carrier_fit"][i], cols["symbol_rate_fit"][i] = float(fc[i]) + float(plan.carrier_offset[i]) + f["eps"] * fs / lay.n_fft, lay.n_data * fs / lay.S
    per = lambda key: np.array([getattr(plan.lay(i), key) if plan.valid[i] else 0 for i in range(n)], dtype=np.int64)      # noqa: E731
    n_used, n_pil, n_data = per("n_used"), per("n_pil"), per("n_data")
    offsets = lambda w: np.concatenate(([0], np.cumsum(n_ofdm * w))).astype(np.int64)      # noqa: E731
    yc0, pil0, pow0, sym0 = offsets(n_used), offsets(n_pil), offsets(1), offsets(n_data)
    raw.update(yc0=yc0, pil0=pil0, pow0=pow0, sym0=sym0)
    # launch 2: the FFT of every OFDM symbol
    items = []
    for i in v:
        lay = plan.lay(i)
        g = np.arange(-(-int(n_ofdm[i]) // lay.group), dtype=np.int64)
        it = np.zeros(g.shape[0], dtype=FFT)
        it["off"], it["len"], it["w"], it["n_fft"], it["S"], it["a"] = plan.offset[i], plan.M[i], np.uint64(raw["W"][i]), lay.n_fft, lay.S, lay.advance
        it["start"], it["nf"] = raw["start"][i] + g * lay.group * lay.S, np.minimum(n_ofdm[i] - g * lay.group, lay.group)
        it["yc_off"], it["pil_off"], it["pow_off"] = yc0[i] + g * lay.group * lay.n_used, pil0[i] + g * lay.group * lay.n_pil, pow0[i] + g * lay.group
        it["bin_off"], it["n_used"], it["n_pil"] = plan.bin0[plan.layout[i]], lay.n_used, lay.n_pil
        items.append(it)
    tw = torch.view_as_real(torch.from_numpy(twiddle_table())).contiguous().to(dev)
    yc = torch.zeros(int(yc0[-1]), dtype=torch.complex64, device=dev)
    pilots_d = torch.zeros(int(pil0[-1]), dtype=torch.complex128, device=dev)
    power = torch.zeros(int(pow0[-1]), dtype=torch.float64, device=dev)
    fft_items = np.concatenate(items)
    bins_d = ops.ofdm_fft(packed, fft_items, plan.bins, tw, yc, pilots_d, power)
    ph = pilots_d.cpu().numpy()
    # fit 2: the pilots' slope, phase and amplitude
    decs, cars, car_at, n_act = [], [], 0, np.zeros(n, dtype=np.int64)
    for i in v:
        lay, m = plan.lay(i), int(n_ofdm[i])
        f = fit2(ph[int(pil0[i]):int(pil0[i + 1])].reshape(m, lay.n_pil), lay)
        raw["phi"][i], raw["active"][i], raw["z"][i], raw["beta"][i], raw["A"][i] = f["phi"], f["active"], f["z"], f["beta"], f["A"]
        cols["slope"][i], cols["n_active"][i], n_act[i] = f["beta"], int(f["active"].sum()), int(f["active"].sum())
        c = np.zeros(lay.n_data, dtype=CAR)
        c["idx"], c["tr"], c["ti"] = lay.data_idx, f["tau"].real, f["tau"].imag
        q = np.arange(m, dtype=np.int64)
        de = np.zeros(m, dtype=DEC)
        de["yc_off"], de["sym_off"], de["rho_r"], de["rho_i"] = yc0[i] + q * lay.n_used, sym0[i] + q * lay.n_data, f["rho"].real, f["rho"].imag
        de["car_off"], de["n_data"], de["n_used"], de["order"], de["row"] = car_at, lay.n_data, lay.n_used, plan.order[i], pow0[i] + q
        car_at += lay.n_data
        decs.append(de)
        cars.append(c)
    # launch 3: the data carriers, corrected, and the decisions
    n_sym = int(sym0[-1])
    r = torch.zeros(n_sym, dtype=torch.complex64, device=dev)
    d = torch.zeros(n_sym, dtype=torch.uint8, device=dev)
    drows = torch.zeros((int(pow0[-1]), 3), dtype=torch.float64, device=dev)
    dec_items, car_table = np.concatenate(decs), np.concatenate(cars)
    cars_d = ops.ofdm_decide(yc, dec_items, car_table, r, d, drows)
    dh = drows.cpu().numpy()
    for i in v:
        act = dh[int(pow0[i]):int(pow0[i + 1])][raw["active"][i]]
        c = columns(act, np.zeros(1), np.zeros(1), 0.0, 0.0)
        cols["gain"][i], cols["evm"][i], cols["mer_db"][i] = c["gain"], c["evm"], c["mer_db"]
        cols["n_symbols"][i] = int(n_ofdm[i]) * int(n_data[i])
    raw.update(fold=fold, yc=yc, pilots=pilots_d, power=power, decision_rows=drows, bins=bins_d, cars=cars_d, twiddle=tw,
               tables={"fold": fold_items, "fft": fft_items, "bins": plan.bins, "dec": dec_items, "cars": car_table})
    symbols = [r[int(sym0[i]):int(sym0[i + 1])] if plan.valid[i] else empty_c for i in range(n)]
    decisions = [d[int(sym0[i]):int(sym0[i + 1])] if plan.valid[i] else empty_u for i in range(n)]
    filtered = [yc[int(yc0[i]):int(yc0[i + 1])].view(int(n_ofdm[i]), int(n_used[i])) if plan.valid[i] else empty_c for i in range(n)]
    return OfdmDemodulation(plan, fc, cols, symbols, decisions, filtered, raw, **meta)
