"""Find framed data in the demodulated clips on the GPU: the host plan of ``csrc/framesync.hip`` (the correlation of every clip's corrected
symbols with every sync word at every position in ONE launch; its peaks in a second; the word errors and the packed payload bits of every
hit in a third), ``find_frames`` and the ``Frames`` result.  The peak says where a frame starts, its argument which of the ``order`` rotations
the demodulator landed on.

Definition.  Clip ``i`` has ``N`` corrected symbols ``r`` (``Demodulation.symbols[i]``) and order ``o``; a word is a bit sequence, first bit
first, ``L = len(bits) / log2(o)`` symbols whose decisions ``w`` are mapped as ``Demodulation.bits`` maps them (order 2: the bit; order 4: ``2 b0 + b1``
of each pair) and name the un-normalised points ``c = 1 - 2 w`` (order 2) or ``(1 - 2 (w >> 1)) + i (1 - 2 (w & 1))`` (order 4), ``|c|^2 = o / 2``.

    pairs     (clip, word) is valid when the clip is, the bit count is divisible by log2(o), 8 <= L <= 256 and L <= N;  P = N - L + 1 positions
    launch 1  float64 from the stored float32 symbols, k ascending, every product and sum rounded on its own:
              Cr += re[p+k] Re c[k] + im[p+k] Im c[k];  Ci += im[p+k] Re c[k] - re[p+k] Im c[k];  E += re[p+k]^2 + im[p+k]^2
              rho2[p] = (Cr Cr + Ci Ci) / ((o / 2) L E), 0 where E == 0;  q[p] = Cr < 0 (order 2), argmax of (Cr, Ci, -Cr, -Ci), lowest on a tie (order 4)
    launch 2  hit[p] = rho2[p] >= threshold^2, no p' in [p - L + 1, p) with rho2[p'] >= rho2[p], none in (p, p + L - 1] with rho2[p'] > rho2[p]
    compact   torch.nonzero(hit): the hits in (clip, word, position) order
    launch 3  v[k] = r[p + k] turned back by q steps of 2 pi / o, decided as the demodulator decides, k in [0, L + n_payload),
              n_payload = min(payload, N - p - L);  row = (errors, bit_errors, n_payload);  the payload bits packed MSB first
"""
from __future__ import annotations

import json
import math
import os

import numpy as np
import torch

L_MIN, L_MAX = 8, 256                                          # symbols of a word: below, random data matches too often; above, correlate by FFT
PAYLOAD_MAX = 1 << 20                                          # payload symbols, exclusive

# laid out as sy11_sync_item / sy11_sync_frame (include/sy11.h)
ITEM = np.dtype([("sym_off", "<i8"), ("n_sym", "<i8"), ("word_off", "<i8"), ("pos_off", "<i8"), ("p0", "<i8"), ("cnt", "<i4"), ("L", "<i4"), ("order", "<i4"),
                 ("reserved", "<i4")])
FRAME = np.dtype([("sym_off", "<i8"), ("n_sym", "<i8"), ("word_off", "<i8"), ("p", "<i8"), ("L", "<i4"), ("order", "<i4"), ("q", "<i4"), ("payload", "<i4"),
                  ("row", "<i4"), ("reserved", "<i4")])

REASONS = {"clip": "clip not valid", "bits": "bit count not divisible by log2(order)", "length": "word outside [8, 256] symbols", "short": "clip shorter than the word"}


def tile():
    """TILE: the positions of one item of launches 1 and 2, a constant of the library's build (``sy11_sync_tile``)."""
    from .. import _lib
    return int(_lib.load().sy11_sync_tile())


def word_decisions(bits, order):
    """The decisions of a word of 0/1 ``bits`` on a clip of ``order``, uint8, as ``Demodulation.decisions`` holds them; None when the bit count is
    not divisible by log2(order)."""
    bits = np.asarray(bits, dtype=np.uint8)
    if order == 2:
        return bits.copy()
    if bits.shape[0] % 2:
        return None
    return (2 * bits[0::2] + bits[1::2]).astype(np.uint8)


class FramePlan:
    """Per clip ``n_symbols``, ``order``, ``clip_valid`` and ``sym_off`` (first symbol in the packed buffer); ``words`` (uint8 bit arrays), ``payload``,
    ``threshold``, ``max_errors``, ``t0``; per pair (clip, word), as (clips, words) arrays: ``valid``, ``reason`` ("" when valid), ``L``, ``P`` (positions, 0 when
    invalid), ``word_off`` (into ``word_buf``, the packed decisions of every word at every order it can be sent at); ``pos0``: clips * words + 1
    offsets of the pairs, clip-major, into the position buffers; ``TILE``."""

    def __init__(self, n_symbols, order, clip_valid, sym_off, words, payload, threshold, max_errors, t0, TILE):
        self.n_symbols, self.order, self.clip_valid, self.sym_off = n_symbols, order, clip_valid, sym_off
        self.words, self.payload, self.threshold, self.max_errors, self.t0, self.TILE = words, int(payload), float(threshold), max_errors, t0, int(TILE)
        n, W = n_symbols.shape[0], len(words)
        buf, at, off = [], {}, 0
        for j, b in enumerate(words):
            for o in (2, 4):
                w = word_decisions(b, o)
                if w is not None:
                    at[j, o] = off
                    buf.append(w)
                    off += w.shape[0]
        self.word_buf = np.concatenate(buf)
        self.valid, self.reason = np.zeros((n, W), dtype=bool), np.full((n, W), "", dtype=object)
        self.L, self.P, self.word_off = np.zeros((n, W), dtype=np.int64), np.zeros((n, W), dtype=np.int64), np.zeros((n, W), dtype=np.int64)
        for i in range(n):
            for j, b in enumerate(words):
                o = int(order[i])
                if not clip_valid[i]:
                    self.reason[i, j] = REASONS["clip"]
                    continue
                if (j, o) not in at:
                    self.reason[i, j] = REASONS["bits"]
                    continue
                L = b.shape[0] // (o // 2)
                self.L[i, j] = L
                if not L_MIN <= L <= L_MAX:
                    self.reason[i, j] = REASONS["length"]
                elif L > int(n_symbols[i]):
                    self.reason[i, j] = REASONS["short"]
                else:
                    self.valid[i, j], self.P[i, j], self.word_off[i, j] = True, int(n_symbols[i]) - L + 1, at[j, o]
        self.pos0 = np.concatenate(([0], np.cumsum(self.P.reshape(-1), dtype=np.int64))).astype(np.int64)
        self.total_positions = int(self.pos0[-1])

    def __len__(self):
        return self.n_symbols.shape[0]

    def __repr__(self):
        return f"FramePlan({len(self)} clips x {len(self.words)} words, {int(self.valid.sum())} valid pairs, {self.total_positions} positions in tiles of {self.TILE})"

    def items(self):
        """Every (pair, tile) work item of launches 1 and 2 -> (``ITEM`` records, the flat pair index ``clip * words + word`` of each)."""
        T, W = self.TILE, len(self.words)
        tiles = -(-self.P.reshape(-1) // T)
        pair = np.repeat(np.arange(tiles.shape[0], dtype=np.int64), tiles)
        first = np.concatenate(([0], np.cumsum(tiles)))[:-1]
        b = np.arange(pair.shape[0], dtype=np.int64) - first[pair]
        clip = pair // W
        it = np.zeros(pair.shape[0], dtype=ITEM)
        it["sym_off"], it["n_sym"], it["word_off"], it["pos_off"] = self.sym_off[clip], self.n_symbols[clip], self.word_off.reshape(-1)[pair], self.pos0[:-1][pair]
        it["p0"], it["cnt"] = b * T, np.minimum(self.P.reshape(-1)[pair] - b * T, T)
        it["L"], it["order"] = self.L.reshape(-1)[pair], self.order[clip]
        return it, pair


def _is_number(v, integer=False):
    if isinstance(v, bool):
        return False
    return isinstance(v, (int, np.integer)) or (not integer and isinstance(v, (float, np.floating)))


def plan_frames(demodulation, words, payload=0, threshold=0.8, *, max_errors=None, t0=None):
    """The ``FramePlan`` of ``demodulation``: a ``Demodulation`` or a pair ``(n_symbols, order)`` of per-clip symbol counts and orders (a clip with an order
    other than 2 or 4, or without symbols, is not valid), packed one after the other.  ``words``: a non-empty sequence of sequences of 0/1
    integers.  Every argument error is a ``ValueError`` raised here, before anything touches the device; a pair that cannot be searched is an
    entry with ``valid`` False and a ``reason``."""
    what = "plan_frames"
    if hasattr(demodulation, "symbols") and hasattr(demodulation, "raw"):
        d = demodulation
        n_symbols, order = np.asarray(d.n_symbols, dtype=np.int64).copy(), np.asarray(d.order, dtype=np.int64).copy()
        clip_valid, sym_off = np.asarray(d.valid, dtype=bool) & (n_symbols >= 1), np.asarray(d.raw["sym0"], dtype=np.int64)[:-1].copy()
    else:
        try:
            n_symbols, order = demodulation
            n_symbols, order = np.atleast_1d(np.asarray(n_symbols)), np.asarray(order)
        except (TypeError, ValueError):
            raise ValueError(f"{what}: give a Demodulation or a pair (n_symbols, order)") from None
        if n_symbols.ndim != 1 or (n_symbols.size and not np.issubdtype(n_symbols.dtype, np.integer)) or (order.size and not np.issubdtype(order.dtype, np.integer)):
            raise ValueError(f"{what}: the clips' symbol counts and orders must be integers, the counts 1-D")
        n_symbols = n_symbols.astype(np.int64)
        try:
            order = np.broadcast_to(order.astype(np.int64), n_symbols.shape).copy()
        except ValueError:
            raise ValueError(f"{what}: {n_symbols.shape[0]} clips but `order` of shape {order.shape}") from None
        if n_symbols.size and int(n_symbols.max()) >= 2 ** 31:
            raise ValueError(f"{what}: a clip of {int(n_symbols.max())} symbols is not below 2^31")
        clip_valid = ((order == 2) | (order == 4)) & (n_symbols >= 1)
        sym_off = np.concatenate(([0], np.cumsum(np.where(clip_valid, n_symbols, 0), dtype=np.int64)))[:-1].astype(np.int64)
    n = n_symbols.shape[0]
    if isinstance(words, (str, bytes)) or not hasattr(words, "__len__") or len(words) == 0:
        raise ValueError(f"{what}: `words` must be a non-empty sequence of bit sequences")
    ws = []
    for j, b in enumerate(words):
        try:
            a = np.asarray(b)
        except (TypeError, ValueError):
            a = np.zeros(0, dtype=object)
        if a.ndim != 1 or a.shape[0] == 0 or a.dtype == bool or not np.issubdtype(a.dtype, np.integer) or not ((a == 0) | (a == 1)).all():
            raise ValueError(f"{what}: word {j} must be a non-empty 1-D sequence of the integers 0 and 1")
        ws.append(a.astype(np.uint8))
    if not _is_number(payload, integer=True) or not 0 <= payload < PAYLOAD_MAX:
        raise ValueError(f"{what}: payload must be an integer in [0, 2^20), got {payload!r}")
    if not _is_number(threshold) or not math.isfinite(float(threshold)) or not 0.0 < threshold <= 1.0:
        raise ValueError(f"{what}: threshold must be in (0, 1], got {threshold!r}")
    if max_errors is not None and (not _is_number(max_errors, integer=True) or max_errors < 0):
        raise ValueError(f"{what}: max_errors must be None or an integer >= 0, got {max_errors!r}")
    if t0 is not None:
        try:
            t0 = np.asarray(t0, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"{what}: `t0` must hold one time per clip") from None
        if t0.shape != (n,):
            raise ValueError(f"{what}: {n} clips but `t0` of shape {t0.shape}")
    return FramePlan(n_symbols, order, clip_valid, sym_off, ws, payload, threshold, None if max_errors is None else int(max_errors), t0, tile())


class Frames:
    """One row per frame, sorted by (clip, word, position), each a numpy array over the frames: ``clip``, ``word``, ``position`` (the symbol of the clip at
    which the word starts), ``rotation`` (the symbols are ahead by this many steps of 2 pi / order), ``rho`` (the normalised correlation, 0 .. 1),
    ``errors`` and ``bit_errors`` (of the word, after turning back), ``n_payload`` (symbols), ``sample`` (of the clip, float64:
    ``(T0 + (i_first + position) STEP) 2^-32``) and ``time`` (``sample / fs``, plus ``t0[clip]`` when given).  ``payload``: (frames, bytes) uint8 on the DEVICE,
    the payload bits packed MSB first; ``payload_bits(k)`` unpacks a row on the host.  Per clip: ``clip_rotation`` (the rotation of its best-``rho``
    frame, -1 without one) and ``n_frames``.  ``pairs``: ``{"valid", "reason"}``, (clips, words) arrays.  ``rows`` / ``cls`` / ``conf`` / ``names`` come from the
    demodulation.  ``raw`` keeps the device buffers ``rho2``, ``q``, ``hit`` (None when nothing was launched) and ``pos0`` (the pairs' offsets into them)."""

    COLUMNS = ("clip", "word", "position", "rotation", "rho", "errors", "bit_errors", "n_payload", "sample", "time")

    def __init__(self, plan, cols, payload, raw, rows=None, cls=None, conf=None, names=None):
        self.plan, self.raw, self.payload = plan, raw, payload
        self.rows, self.cls, self.conf, self.names = rows, cls, conf, names
        for k in self.COLUMNS:
            setattr(self, k, cols[k])
        self.pairs = {"valid": plan.valid, "reason": plan.reason}
        n = len(plan)
        self.n_frames = np.bincount(self.clip, minlength=n).astype(np.int64)[:n] if n else np.zeros(0, dtype=np.int64)
        self.clip_rotation = np.full(n, -1, dtype=np.int64)
        for k in np.argsort(-self.rho, kind="stable")[::-1]:                # the best of a clip is written last; of equal ones the first frame
            self.clip_rotation[self.clip[k]] = self.rotation[k]

    def __len__(self):
        return self.clip.shape[0]

    def __getitem__(self, k):
        """Frame k as a dict of its scalars."""
        k = range(len(self))[k]
        return {c: getattr(self, c)[k].item() for c in self.COLUMNS}

    def payload_bits(self, k):
        """The payload bits of frame ``k`` on the host, uint8, ``n_payload`` symbols' worth, the first bit first."""
        k = range(len(self))[k]
        n = int(self.n_payload[k]) * (int(self.plan.order[self.clip[k]]) // 2)
        return np.unpackbits(self.payload[k].cpu().numpy())[:n].astype(np.uint8)

    def save(self, directory):
        """Write ``frames.npz`` (every column, the packed payload, ``clip_rotation``, ``n_frames`` and the pairs' validity) and ``frames.json`` (the
        words, the arguments and one record per frame).  -> the directory."""
        directory = os.fspath(directory)
        os.makedirs(directory, exist_ok=True)
        arrays = {k: getattr(self, k) for k in self.COLUMNS + ("clip_rotation", "n_frames")}
        arrays.update(payload=self.payload.cpu().numpy(), pair_valid=self.plan.valid, pair_reason=np.asarray(self.plan.reason, dtype=str),
                      rows=np.arange(len(self.plan)) if self.rows is None else np.asarray(self.rows))
        np.savez(os.path.join(directory, "frames.npz"), **arrays)
        rows = arrays["rows"]
        out = []
        for k in range(len(self)):
            i = int(self.clip[k])
            cls = None if self.cls is None else int(self.cls[i])
            rec = {c: getattr(self, c)[k].item() for c in self.COLUMNS}
            rec.update(row=int(rows[i]), name=None if cls is None or not self.names else self.names.get(cls))
            rec["class"] = cls
            out.append(rec)
        with open(os.path.join(directory, "frames.json"), "w") as f:
            json.dump({"words": [w.tolist() for w in self.plan.words], "payload": self.plan.payload, "threshold": self.plan.threshold,
                       "max_errors": self.plan.max_errors, "tile": self.plan.TILE, "file": "frames.npz", "frames": out}, f, indent=1)
        return directory


def _packed_symbols(d, plan):
    """The packed buffer the views ``d.symbols`` look into (``sy11_demod_decide``'s r); a copy only where they are not one buffer's slices."""
    total = int(np.asarray(d.raw["sym0"])[-1])
    live = [i for i in range(len(plan)) if d.symbols[i].numel()]
    base = d.symbols[live[0]]
    base = base if base._base is None else base._base
    if base.dim() == 1 and base.dtype == torch.complex64 and base.is_contiguous() and base.shape[0] == total and \
            all(d.symbols[i].data_ptr() == base.data_ptr() + 8 * int(plan.sym_off[i]) and d.symbols[i].is_contiguous() for i in live):
        return base
    out = torch.zeros(total, dtype=torch.complex64, device=base.device)
    for i in live:
        out[int(plan.sym_off[i]):int(plan.sym_off[i]) + d.symbols[i].shape[0]] = d.symbols[i]
    return out


def find_frames(demodulation, words, *, payload=0, threshold=0.8, max_errors=None, t0=None):
    """Search every clip of ``demodulation`` (``sy11.data.demodulate.Demodulation``) for every word of ``words`` -> ``Frames``: three launches over all
    clips and one ``torch.nonzero`` between the second and the third; one copy of the hit list and one of the rows to the host.  ``payload``: the
    symbols to read after each word; ``threshold``: the smallest normalised correlation of a frame; ``max_errors``: drop frames whose word has
    more symbol errors (on the host, after launch 3); ``t0``: per clip, seconds added to ``time`` (``extraction.t0``).  Without a valid pair, or
    without a hit, the later launches are skipped and the result is empty."""
    from .. import ops
    d = demodulation
    plan = plan_frames(d, words, payload, threshold, max_errors=max_errors, t0=t0)
    meta = dict(rows=d.rows, cls=d.cls, conf=d.conf, names=d.names)
    raw = {"rho2": None, "q": None, "hit": None, "pos0": plan.pos0}
    dev = d.symbols[0].device if len(d.symbols) else torch.device("cpu")

    def result(cols, bits):
        return Frames(plan, cols, bits, raw, **meta)

    def empty():
        cols = {k: np.zeros(0, dtype=np.float64 if k in ("rho", "sample", "time") else np.int64) for k in Frames.COLUMNS}
        return result(cols, torch.zeros((0, 0), dtype=torch.uint8, device=dev))
    if plan.total_positions == 0:
        return empty()
    sym = _packed_symbols(d, plan)
    items, _ = plan.items()
    wbuf = torch.from_numpy(plan.word_buf).to(dev)
    n_pos = plan.total_positions
    rho2 = torch.zeros(n_pos, dtype=torch.float64, device=dev)
    q = torch.zeros(n_pos, dtype=torch.uint8, device=dev)
    hit = torch.zeros(n_pos, dtype=torch.uint8, device=dev)
    ops.sync_correlate(sym, items, wbuf, rho2, q)
    ops.sync_peaks(rho2, items, plan.threshold * plan.threshold, hit, sym.shape[0], wbuf.shape[0])
    raw.update(rho2=rho2, q=q, hit=hit)
    idx = torch.nonzero(hit).squeeze(1)                                     # in position order: (clip, word, position)
    if idx.shape[0] == 0:
        return empty()
    hits = torch.stack((idx.to(torch.float64), q[idx].to(torch.float64), rho2[idx]), 1).cpu().numpy()      # positions below 2^31: exact
    at = hits[:, 0].astype(np.int64)
    W = len(plan.words)
    pair = np.searchsorted(plan.pos0, at, side="right") - 1
    clip, word, pos = pair // W, pair % W, at - plan.pos0[pair]
    n = at.shape[0]
    fr = np.zeros(n, dtype=FRAME)
    fr["sym_off"], fr["n_sym"], fr["word_off"], fr["p"] = plan.sym_off[clip], plan.n_symbols[clip], plan.word_off.reshape(-1)[pair], pos
    fr["L"], fr["order"], fr["q"], fr["payload"], fr["row"] = plan.L.reshape(-1)[pair], plan.order[clip], hits[:, 1].astype(np.int64), plan.payload, np.arange(n)
    stride = int((plan.payload * (int(plan.order[clip].max()) // 2) + 7) // 8)
    rows = torch.zeros((n, 3), dtype=torch.int32, device=dev)
    bits = torch.zeros((n, stride), dtype=torch.uint8, device=dev)
    ops.sync_frames(sym, fr, wbuf, rows, bits)
    rh = rows.cpu().numpy().astype(np.int64)
    sample = np.array([(d.raw["T0"][c] + (d.raw["i_first"][c] + int(p)) * d.raw["STEP"][c]) / 2.0 ** 32 for c, p in zip(clip, pos)], dtype=np.float64)
    time = sample / np.asarray(d.sample_rate, dtype=np.float64)[clip]
    if plan.t0 is not None:
        time = time + plan.t0[clip]
    cols = {"clip": clip, "word": word, "position": pos, "rotation": hits[:, 1].astype(np.int64), "rho": np.sqrt(hits[:, 2]), "errors": rh[:, 0],
            "bit_errors": rh[:, 1], "n_payload": rh[:, 2], "sample": sample, "time": time}
    if plan.max_errors is not None:
        keep = rh[:, 0] <= plan.max_errors
        cols = {k: v[keep] for k, v in cols.items()}
        bits = bits[torch.from_numpy(keep).to(dev)]
    return result(cols, bits)
