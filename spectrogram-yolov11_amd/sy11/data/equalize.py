"""Equalise the frames the frame search found on the GPU: the host plan of ``csrc/equalize.hip`` (the least-squares taps of every frame, trained on its
sync word, in ONE launch; the taps of each frame over the symbols it owns, and a copy of every other symbol, in a second; both once more when the
taps are refined on the decisions of the first pass), ``equalize_frames`` and the ``Equalized`` result, which ``find_frames`` and ``decode`` take in place of the
``Demodulation``.  Feed-forward: the frame search says where each known word sits and at which rotation, so no loop runs along the clip.

Definition.  Clip ``i`` has ``N_i`` corrected symbols ``r`` (``Demodulation.symbols[i]``, 0 outside the clip), order ``o`` and gain ``A``; frame ``f`` sits in it at
position ``p`` with word length ``L``, rotation ``q`` and ``n_payload``; ``taps = N`` is odd, 3 .. 15, ``D = (N - 1) / 2``.

    target    t[k] = A point(word[k]) turned FORWARD by q steps of 2 pi / o (k < L);  A point(decide(e1[p + k])) of the first pass's output (L <= k < Lt)
    launch 1  float64, k ascending:  u_k[j] = r[p + k + D - j];  R = sum_k conj(u_k) u_k^T,  z = sum_k conj(u_k) t[k],  k < Lt;  R += reg (tr R / N) I;
              R = G G^H,  w = R^-1 z;  pivot_min = min_a G[a][a]^2 / (tr R / N);  a pivot not finite and positive: "singular", w = the unit impulse at D
              mse_before = sum_(k<L) |r[p + k] - t[k]|^2 / (L A^2),  mse_after the same with w^T u_k for r[p + k]
    owner     of symbol m: among the valid frames of the clip with p <= m < p + L + n_payload the one of the greatest p, of equal ones the first
    launch 2  e[m] = f32(sum_j w[j] r[m + D - j]), j ascending, re += (wr a) - (wi b), im += (wr b) + (wi a), every product and sum rounded on its own;
              without an owner e[m] = r[m] bit for bit;  decisions[m] as the demodulator decides e[m]
    refine    > L: launches 1 and 2 again with Lt = min(refine, L + n_payload) and the targets beyond the word from the first pass's decisions
"""
from __future__ import annotations

import json
import math
import os

import numpy as np
import torch

TAPS_MIN, TAPS_MAX = 3, 15                                     # odd
L_MAX = 256                                                    # symbols of a word (the frame search's)
LT_MAX = 4096                                                  # training symbols of a frame; `refine` at the most

# laid out as sy11_eq_frame / sy11_eq_segment / sy11_eq_item (include/sy11.h)
EQFRAME = np.dtype([("sym_off", "<i8"), ("n_sym", "<i8"), ("word_off", "<i8"), ("p", "<i8"), ("L", "<i4"), ("Lt", "<i4"), ("order", "<i4"), ("q", "<i4"), ("row", "<i4"),
                    ("reserved", "<i4"), ("gain", "<f8")])
EQSEGMENT = np.dtype([("sym_off", "<i8"), ("n_sym", "<i8"), ("start", "<i8"), ("end", "<i8"), ("frame", "<i4"), ("order", "<i4")])
EQITEM = np.dtype([("seg", "<i4"), ("tile", "<i4")])

REASONS = ("clip", "gain", "word", "singular")                 # the clip is not valid; its gain is not a positive number; L < 2 taps; a pivot of the Cholesky failed


def tile():
    """TILE: the symbols of one item of launch 2, a constant of the library's build (``sy11_eq_tile``)."""
    from .. import _lib
    return int(_lib.load().sy11_eq_tile())


class EqualizePlan:
    """The arguments, checked: ``taps``, ``reg``, ``refine``, ``TILE``; per clip ``n_symbols`` (0 when invalid), ``order``, ``clip_valid``, ``sym_off`` and ``gain``; per frame of the
    ``Frames``: ``valid``, ``reason`` ("" when valid), ``clip``, ``word``, ``position``, ``L``, ``rotation``, ``n_payload``, ``word_off`` (into ``word_buf``) and ``n_train`` (the training symbols of the
    last pass, 0 when invalid); ``second``: whether a second pass runs; ``segments``: the ``EQSEGMENT`` table of the ownership rule, covering every symbol of
    every clip once."""

    def __init__(self, taps, reg, refine, TILE, n_symbols, order, clip_valid, sym_off, gain, clip, word, position, L, rotation, n_payload, word_off, word_buf):
        self.taps, self.reg, self.refine, self.TILE = taps, reg, refine, int(TILE)
        self.n_symbols, self.order, self.clip_valid, self.sym_off, self.gain = n_symbols, order, clip_valid, sym_off, gain
        self.clip, self.word, self.position, self.L, self.rotation, self.n_payload, self.word_off, self.word_buf = clip, word, position, L, rotation, n_payload, word_off, word_buf
        n = clip.shape[0]
        self.reason = np.full(n, "", dtype=object)
        self.reason[L < 2 * taps] = "word"
        with np.errstate(invalid="ignore"):
            self.reason[~(np.isfinite(gain[clip]) & (gain[clip] > 0))] = "gain"
        self.reason[~clip_valid[clip]] = "clip"
        self.valid = self.reason == ""
        Lt = np.where(refine > L, np.minimum(refine, L + n_payload), L)
        self.n_train = np.where(self.valid, Lt, 0).astype(np.int64)
        self.second = bool((self.n_train > L).any())
        self.segments = self._segments()

    def __len__(self):
        return self.clip.shape[0]

    def __repr__(self):
        return f"EqualizePlan({len(self)} frames, {int(self.valid.sum())} valid, taps={self.taps}, reg={self.reg}, refine={self.refine}, {self.segments.shape[0]} segments)"

    def _segments(self):
        """The ownership rule as a table: per clip the sorted boundaries of the valid frames' spans cut it into intervals, each with the owner of its first
        symbol; neighbours of one owner are joined."""
        out = []
        for i in np.flatnonzero(self.n_symbols > 0):
            N = int(self.n_symbols[i])
            fs = np.flatnonzero(self.valid & (self.clip == i))
            p = self.position[fs]
            e = np.minimum(p + self.L[fs] + self.n_payload[fs], N)
            b = np.unique(np.concatenate(([0, N], p, e)))
            b = b[(b >= 0) & (b <= N)]
            lo = b[:-1]
            owner = np.full(lo.shape[0], -1, dtype=np.int64)
            if fs.shape[0]:
                cover = (p[None, :] <= lo[:, None]) & (lo[:, None] < e[None, :])
                key = np.where(cover, p[None, :], -1)
                best = key.max(1)
                first = np.argmax(cover & (key == best[:, None]), axis=1)            # of equal p the first in the Frames' order
                owner = np.where(best >= 0, fs[first], -1)
            keep = np.concatenate(([True], owner[1:] != owner[:-1]))
            start = lo[keep]
            sg = np.zeros(start.shape[0], dtype=EQSEGMENT)
            sg["sym_off"], sg["n_sym"], sg["start"], sg["end"], sg["frame"], sg["order"] = self.sym_off[i], N, start, np.concatenate((start[1:], [N])), owner[keep], self.order[i]
            out.append(sg)
        return np.concatenate(out) if out else np.zeros(0, dtype=EQSEGMENT)

    def items(self):
        """Every (segment, tile) work item of launch 2 -> ``EQITEM`` records."""
        sg = self.segments
        tiles = -(-(sg["end"] - sg["start"]) // self.TILE)
        seg = np.repeat(np.arange(sg.shape[0], dtype=np.int64), tiles)
        first = np.concatenate(([0], np.cumsum(tiles)))[:-1]
        it = np.zeros(seg.shape[0], dtype=EQITEM)
        it["seg"], it["tile"] = seg, np.arange(seg.shape[0], dtype=np.int64) - first[seg]
        return it

    def table(self, second=False):
        """The ``EQFRAME`` records of the valid frames, each writing the row of its index; the first pass trains on the word, the second on ``n_train``."""
        at = np.flatnonzero(self.valid)
        c = self.clip[at]
        fr = np.zeros(at.shape[0], dtype=EQFRAME)
        fr["sym_off"], fr["n_sym"], fr["word_off"], fr["p"], fr["L"] = self.sym_off[c], self.n_symbols[c], self.word_off[at], self.position[at], self.L[at]
        fr["Lt"], fr["order"], fr["q"], fr["row"], fr["gain"] = self.n_train[at] if second else self.L[at], self.order[c], self.rotation[at], at, self.gain[c]
        return fr


def plan_equalize(frames, demodulation, *, taps=7, reg=1e-3, refine=0):
    """The ``EqualizePlan`` of ``frames`` (a ``Frames``) on ``demodulation`` (the ``Demodulation`` it was found in, or an ``Equalized`` of it).  Every argument error is a
    ``ValueError`` raised here, before anything touches the device; a frame that cannot be equalised is an entry with ``valid`` False and a ``reason``."""
    what = "plan_equalize"
    f, d = frames, demodulation
    if not all(hasattr(f, k) for k in ("plan", "clip", "word", "position", "rotation", "n_payload")) or not all(hasattr(d, k) for k in ("gain", "n_symbols", "order", "valid", "raw")):
        raise ValueError(f"{what}: give the Frames of find_frames and the Demodulation they were found in")
    fp = f.plan
    if np.asarray(d.n_symbols).shape != fp.n_symbols.shape or np.asarray(d.gain).shape != fp.n_symbols.shape or not np.array_equal(np.asarray(d.n_symbols, dtype=np.int64), fp.n_symbols) or not np.array_equal(np.asarray(d.order, dtype=np.int64), fp.order):
        raise ValueError(f"{what}: the frames were not found in this demodulation (the clips' count, n_symbols or order differ)")
    if isinstance(taps, (bool, np.bool_)) or not isinstance(taps, (int, np.integer)) or not TAPS_MIN <= taps <= TAPS_MAX or taps % 2 == 0:
        raise ValueError(f"{what}: taps must be an odd integer in [{TAPS_MIN}, {TAPS_MAX}], got {taps!r}")
    if isinstance(reg, (bool, np.bool_)) or not isinstance(reg, (int, float, np.integer, np.floating)) or not math.isfinite(float(reg)) or not 0.0 <= float(reg) <= 1.0:
        raise ValueError(f"{what}: reg must be finite and in [0, 1], got {reg!r}")
    if isinstance(refine, (bool, np.bool_)) or not isinstance(refine, (int, np.integer)) or not 0 <= refine <= LT_MAX:
        raise ValueError(f"{what}: refine must be 0 or an integer in (0, {LT_MAX}], got {refine!r}")
    n_symbols = np.maximum(np.asarray(d.n_symbols, dtype=np.int64), 0)
    order = np.asarray(d.order, dtype=np.int64).copy()
    clip_valid = np.asarray(d.valid, dtype=bool) & (n_symbols >= 1) & ((order == 2) | (order == 4))
    n_symbols = np.where(clip_valid, n_symbols, 0)
    sym_off = np.asarray(d.raw["sym0"], dtype=np.int64)[:-1].copy()
    if not np.array_equal(sym_off, fp.sym_off):
        raise ValueError(f"{what}: the frames were not found in this demodulation (the clips lie elsewhere in the packed symbols)")
    clip, word = np.asarray(f.clip, dtype=np.int64).copy(), np.asarray(f.word, dtype=np.int64).copy()
    return EqualizePlan(int(taps), float(reg), int(refine), tile(), n_symbols, order, clip_valid, sym_off, np.asarray(d.gain, dtype=np.float64).copy(), clip, word,
                        np.asarray(f.position, dtype=np.int64).copy(), fp.L[clip, word].astype(np.int64), np.asarray(f.rotation, dtype=np.int64).copy(),
                        np.asarray(f.n_payload, dtype=np.int64).copy(), fp.word_off[clip, word].astype(np.int64), fp.word_buf)


class FrameRows:
    """One row per frame of the ``Frames``, in its order, each a numpy array over the frames: ``valid`` and ``reason`` ("word": the word is shorter than 2 taps; "gain": the
    clip's gain is not a positive number; "clip": the clip is not valid; "singular": a pivot of the Cholesky was not finite and positive), ``clip``, ``word``,
    ``position``, ``n_train`` (the training symbols of the last pass), ``mse_before`` and ``mse_after`` (over the word, relative to the gain squared), ``pivot_min``; NaN and
    ``n_train`` 0 for a frame that was not solved."""

    COLUMNS = ("valid", "clip", "word", "position", "n_train", "mse_before", "mse_after", "pivot_min")

    def __init__(self, cols, reason):
        self.reason = reason
        for k in self.COLUMNS:
            setattr(self, k, cols[k])

    def __len__(self):
        return self.valid.shape[0]

    def __getitem__(self, k):
        """Frame k as a dict of its scalars."""
        k = range(len(self))[k]
        d = {c: getattr(self, c)[k].item() for c in self.COLUMNS}
        d["reason"] = str(self.reason[k])
        return d


class Equalized:
    """What ``find_frames`` and ``decode`` read of a ``Demodulation``, with the equalised symbols in its place.  On the DEVICE, as lists of views into ONE packed buffer
    each with the demodulation's layout (``raw["sym0"]``): ``symbols`` (complex64) and ``decisions`` (uint8).  Per clip, taken over from the demodulation: ``valid``,
    ``n_symbols``, ``order``, ``gain``, ``phase_ambiguity``, ``sample_rate``, ``center_freq``; the equalised symbols keep the clip's rotation and gain.  ``frames``: the ``FrameRows``, one row
    per frame of the ``Frames`` (per-frame ``valid`` is ``frames.valid``: ``valid`` is the clips', which the frame search reads); ``w``: (frames, taps) complex128 on the host,
    the unit impulse for a frame that is not valid.  ``rows`` / ``cls`` / ``conf`` / ``names`` come from the demodulation.  ``raw``: ``sym0``, ``T0``, ``STEP``, ``i_first`` (the
    demodulation's), the packed device buffers ``symbols`` and ``decisions``, and ``w`` (frames, 15) complex128 / ``solve_rows`` (frames, 4) float64 on the device
    (None when nothing was launched)."""

    def __init__(self, plan, demodulation, packed, decided, frames, w, raw):
        d = demodulation
        self.plan, self.raw, self.frames, self.w = plan, raw, frames, w
        self.rows, self.cls, self.conf, self.names = d.rows, d.cls, d.conf, d.names
        self.valid, self.n_symbols, self.order = np.asarray(d.valid, dtype=bool).copy(), np.asarray(d.n_symbols).copy(), np.asarray(d.order).copy()
        self.gain, self.phase_ambiguity = np.asarray(d.gain, dtype=np.float64).copy(), np.asarray(d.phase_ambiguity).copy()
        self.sample_rate, self.center_freq = getattr(d, "sample_rate", None), getattr(d, "center_freq", None)
        self.symbols = [packed[int(a):int(a) + int(n)] for a, n in zip(plan.sym_off, plan.n_symbols)]
        self.decisions = [decided[int(a):int(a) + int(n)] for a, n in zip(plan.sym_off, plan.n_symbols)]

    def __len__(self):
        return self.valid.shape[0]

    def save(self, directory):
        """Write ``equalize.npz`` (every column of ``frames``, the reasons, ``w``, the clips' columns, ``sym0`` and the packed symbols and decisions) and ``equalize.json`` (the
        arguments and one record per frame).  -> the directory."""
        directory = os.fspath(directory)
        os.makedirs(directory, exist_ok=True)
        fr, p = self.frames, self.plan
        arrays = {k: getattr(fr, k) for k in fr.COLUMNS}
        arrays.update(reason=np.asarray([str(r) for r in fr.reason], dtype=str), w=self.w, clip_valid=self.valid, n_symbols=self.n_symbols, order=self.order, gain=self.gain,
                      phase_ambiguity=self.phase_ambiguity, sym0=np.asarray(self.raw["sym0"], dtype=np.int64), symbols=self.raw["symbols"].cpu().numpy(),
                      decisions=self.raw["decisions"].cpu().numpy(), rows=np.arange(len(self)) if self.rows is None else np.asarray(self.rows))
        np.savez(os.path.join(directory, "equalize.npz"), **arrays)
        out = []
        for k in range(len(fr)):
            rec = fr[k]
            for c in ("mse_before", "mse_after", "pivot_min"):
                rec[c] = rec[c] if math.isfinite(rec[c]) else None
            cls = None if self.cls is None else int(self.cls[int(fr.clip[k])])
            rec.update(row=int(arrays["rows"][int(fr.clip[k])]), name=None if cls is None or not self.names else self.names.get(cls),
                       w=[[float(v.real), float(v.imag)] for v in self.w[k]])
            rec["class"] = cls
            out.append(rec)
        with open(os.path.join(directory, "equalize.json"), "w") as f:
            json.dump({"taps": p.taps, "reg": p.reg, "refine": p.refine, "tile": p.TILE, "file": "equalize.npz", "frames": out}, f, indent=1)
        return directory


def _packed_decisions(d, plan, dev):
    total = int(np.asarray(d.raw["sym0"])[-1])
    out = torch.zeros(total, dtype=torch.uint8, device=dev)
    for i in range(len(plan.n_symbols)):
        if d.decisions[i].numel():
            out[int(plan.sym_off[i]):int(plan.sym_off[i]) + d.decisions[i].shape[0]] = d.decisions[i]
    return out


def equalize_frames(frames, demodulation, *, taps=7, reg=1e-3, refine=0):
    """Equalise every frame of ``frames`` (``sy11.data.frames.Frames``, found in ``demodulation``) -> ``Equalized``: two launches over all frames and clips, four with a ``refine``
    beyond a word's length, and one copy of the frames' rows and taps to the host.  ``taps``: the length of the symbol-spaced FIR; ``reg``: the diagonal loading,
    relative to the mean diagonal of R; ``refine``: train a second pass on this many symbols of each frame, those after the word decided by the first pass.
    Without a valid frame nothing is launched and the symbols are the demodulation's, copied."""
    from .. import ops
    from .frames import _packed_symbols
    f, d = frames, demodulation
    plan = plan_equalize(f, d, taps=taps, reg=reg, refine=refine)
    n, N = len(plan), plan.taps
    dev = f.payload.device if hasattr(f, "payload") and f.payload is not None else (d.symbols[0].device if len(d.symbols) else torch.device("cpu"))
    total = int(np.asarray(d.raw["sym0"])[-1])
    cols = {"valid": plan.valid.copy(), "clip": plan.clip.copy(), "word": plan.word.copy(), "position": plan.position.copy(), "n_train": plan.n_train.copy(),
            "mse_before": np.full(n, np.nan), "mse_after": np.full(n, np.nan), "pivot_min": np.full(n, np.nan)}
    reason = plan.reason.copy()
    w = np.zeros((n, N), dtype=np.complex128)
    w[:, (N - 1) // 2] = 1.0
    raw = {k: d.raw[k] for k in ("sym0", "T0", "STEP", "i_first") if k in d.raw}
    raw.update(symbols=None, decisions=None, w=None, solve_rows=None)
    sym = _packed_symbols(d, f.plan) if total and any(s.numel() for s in d.symbols) else torch.zeros(0, dtype=torch.complex64, device=dev)
    if not plan.valid.any():
        raw.update(symbols=sym.clone(), decisions=_packed_decisions(d, plan, dev))
        return Equalized(plan, d, raw["symbols"], raw["decisions"], FrameRows(cols, reason), w, raw)
    if int((plan.segments["end"] - plan.segments["start"]).sum()) == sym.shape[0]:             # the segments write every symbol
        out, dec = torch.empty_like(sym), torch.empty(sym.shape[0], dtype=torch.uint8, device=dev)
    else:                                                                                       # symbols of a clip that is not valid: as they are
        out, dec = sym.clone(), _packed_decisions(d, plan, dev)
    wd = torch.zeros((n, TAPS_MAX), dtype=torch.complex128, device=dev)
    rows = torch.zeros((n, 4), dtype=torch.float64, device=dev)
    wbuf = torch.from_numpy(plan.word_buf).to(dev)
    items = plan.items()
    ops.eq_solve(sym, plan.table(False), wbuf, N, plan.reg, wd, rows)
    ops.eq_apply(sym, items, plan.segments, N, wd, out, dec)
    if plan.second:
        ops.eq_solve(sym, plan.table(True), wbuf, N, plan.reg, wd, rows, decisions=dec)
        ops.eq_apply(sym, items, plan.segments, N, wd, out, dec)
    raw.update(symbols=out, decisions=dec, w=wd, solve_rows=rows)
    h = torch.cat((rows, torch.view_as_real(wd).reshape(n, 2 * TAPS_MAX)), 1).cpu().numpy()        # one copy: the rows and the taps
    v = plan.valid
    ok = v & (h[:, 3] != 0.0)
    cols["mse_before"][v], cols["mse_after"][v], cols["pivot_min"][v] = h[v, 0], h[v, 1], h[v, 2]
    cols["valid"] = ok
    reason[v & ~ok] = "singular"
    w[v] = (h[v, 4::2] + 1j * h[v, 5::2])[:, :N]
    return Equalized(plan, d, out, dec, FrameRows(cols, reason), w, raw)
