"""Decode the frames the frame search found on the GPU: the host plan of ``csrc/fec.hip`` (the soft bits of every frame's payload symbols,
depunctured, in ONE launch; the Viterbi decoder of the rate 1/2, K = 7 convolutional code in a second; the re-encoded channel error count, the
de-whitened information bits and their CRC in a third), ``decode_frames`` and the ``Decoded`` result.

Definition.  Frame ``k`` lies in clip ``i`` at position ``p`` with rotation ``q`` and word length ``L``; the clip has order ``o``, ``w = log2(o)`` bits per
symbol; its received stream starts at symbol ``sym_off[i] + p + L`` of the demodulation's packed ``r``.

    code      rate 1/2, K = 7, generators (g0, g1), 7-bit with bits 6 and 0 set;  R = (u_t << 6) | s,  c[2t + j] = parity(R & g_j),  s' = R >> 1,  s_0 = 0;
              tail: six zero bits follow the n_info information bits, T = n_info + 6 steps, end state 0;  no tail: T = n_info, end state free;  T <= 8192
    puncture  a 0/1 pattern over c[0], c[1], ..., even period <= 64, 1 = sent;  n_coded = its ones over [0, 2T),  n_need = ceil(n_coded / w) symbols
    launch 1  received bit m = component m % w of symbol m // w turned back by q steps;  y = clamp(rintf(x * scale_k), -127, 127), NaN -> 0,
              scale_k = float32(soft_scale / a_i),  a_i = gain[i] (order 2), gain[i] / sqrt(2) (order 4);  mother position j gets the next y or 0
    launch 2  PM(0) = 0, PM(s != 0) = -2^30;  R_b = (s' << 1) | b,  m_b = PM(R_b & 63) + sum_j (1 - 2 parity(R_b & g_j)) y[2t + j],  d_t(s') = m_1 > m_0,
              PM'(s') = max(m_0, m_1);  end state 0 (tail) or the largest metric, the lowest state on a tie;  u_t = s >> 5,  s = ((s << 1) | d_t(s)) & 63
    launch 3  c^ = the decided bits encoded again;  n_channel = #{y != 0},  channel_errors = #{y != 0 and (y < 0) != c^};  v_t = u_t ^ whiten_t, t < n_info;
              crc_recv = the last `width` bits of v, MSB first;  crc_calc over the n_info - width bits before them (Rocksoft model)
"""
from __future__ import annotations

import math

import numpy as np
import torch

from ._frame_table import BitTable, frame_columns, unpack_check

# laid out as sy11_fec_frame (include/sy11.h)
FECFRAME = np.dtype([("sym_off", "<i8"), ("T", "<i4"), ("order", "<i4"), ("q", "<i4"), ("tail", "<i4"), ("row", "<i4"), ("scale", "<f4")])

K = 7
REASONS = ("short", "gain")                                    # fewer payload symbols than the code needs; the clip's gain is not a positive number

# the Rocksoft model of the checks by name
CRCS = {
    "crc8": dict(width=8, poly=0x07, init=0x00, refin=False, refout=False, xorout=0x00),
    "crc16-ccitt-false": dict(width=16, poly=0x1021, init=0xFFFF, refin=False, refout=False, xorout=0x0000),
    "crc16-x25": dict(width=16, poly=0x1021, init=0xFFFF, refin=True, refout=True, xorout=0xFFFF),
    "crc32": dict(width=32, poly=0x04C11DB7, init=0xFFFFFFFF, refin=True, refout=True, xorout=0xFFFFFFFF),
}


def t_max():
    """T_MAX: the trellis steps of a frame at the most, a constant of the library's build (``sy11_fec_tmax``)."""
    from .. import _lib
    return int(_lib.load().sy11_fec_tmax())


def lfsr_bits(taps, state, n):
    """``n`` bits of a Fibonacci shift register, uint8: ``state[i - 1]`` is stage ``i``; per bit the output is the XOR of the stages ``taps`` (1-based), and is
    shifted in at stage 1.  ``lfsr_bits((4, 7), [1] * 7, 127)`` is the 802.11 scrambler's sequence."""
    s = [int(b) for b in state]
    taps = [int(t) for t in taps]
    if not s or any(b not in (0, 1) for b in s) or not taps or any(not 1 <= t <= len(s) for t in taps):
        raise ValueError(f"lfsr_bits: `state` must be a non-empty 0/1 sequence and `taps` stages in [1, {len(s)}], got {state!r} / {taps!r}")
    out = np.zeros(int(n), dtype=np.uint8)
    for k in range(int(n)):
        b = 0
        for t in taps:
            b ^= s[t - 1]
        out[k] = b
        s = [b] + s[:-1]
    return out


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _bit_array(what, name, v):
    try:
        a = np.asarray(v)
    except (TypeError, ValueError):
        a = np.zeros(0, dtype=object)
    if isinstance(v, (str, bytes)) or a.ndim != 1 or a.shape[0] == 0 or a.dtype == bool or not np.issubdtype(a.dtype, np.integer) or not ((a == 0) | (a == 1)).all():
        raise ValueError(f"{what}: `{name}` must be a non-empty 1-D sequence of the integers 0 and 1")
    return a.astype(np.uint8)


def _crc_spec(what, crc, n_info):
    if crc is None:
        return None
    if isinstance(crc, str):
        if crc not in CRCS:
            raise ValueError(f"{what}: crc {crc!r} is not one of {sorted(CRCS)}")
        spec = dict(CRCS[crc], name=crc)
    elif isinstance(crc, dict):
        if set(crc) - {"name"} != {"width", "poly", "init", "refin", "refout", "xorout"}:
            raise ValueError(f"{what}: a crc dict holds width, poly, init, refin, refout and xorout, got {sorted(crc)}")
        spec = dict(crc)
        spec.setdefault("name", None)
    else:
        raise ValueError(f"{what}: crc must be None, a name of CRCS or a dict, got {crc!r}")
    W = spec["width"]
    if not _is_int(W) or not 8 <= W <= 32:
        raise ValueError(f"{what}: the crc's width must be an integer in [8, 32], got {W!r}")
    for k in ("poly", "init", "xorout"):
        if not _is_int(spec[k]) or not 0 <= spec[k] < 2 ** W:
            raise ValueError(f"{what}: the crc's {k} must be an integer of {W} bits, got {spec[k]!r}")
    for k in ("refin", "refout"):
        if not isinstance(spec[k], (bool, np.bool_)) and spec[k] not in (0, 1):
            raise ValueError(f"{what}: the crc's {k} must be a bool, got {spec[k]!r}")
        spec[k] = bool(spec[k])
    if n_info <= W:
        raise ValueError(f"{what}: n_info = {n_info} must exceed the crc's {W} bits")
    if spec["refin"] and (n_info - W) % 8:
        raise ValueError(f"{what}: a crc with refin takes whole bytes, but n_info - width = {n_info - W} bits")
    return spec


class DecodePlan:
    """The arguments, checked: ``n_info``, ``polys``, ``tail``, ``T`` (trellis steps), ``pattern`` (uint8, None when nothing is punctured), ``period`` and ``mask`` (bit i =
    position i; 2 and 3 without a pattern), ``n_coded`` (received bits of a frame), ``whiten`` (uint8 of n_info bits, or None), ``crc`` (the Rocksoft dict
    with its ``name``, or None), ``soft_scale``; per frame of the ``Frames``: ``valid``, ``reason`` ("" when valid), ``n_need`` (payload symbols), ``scale`` (float32) and
    ``sym_off`` (the first payload symbol in the packed symbol buffer)."""

    def __init__(self, n_info, polys, tail, T, pattern, whiten, crc, soft_scale, order, gain, sym_off, n_payload):
        self.n_info, self.polys, self.tail, self.T, self.pattern, self.whiten, self.crc, self.soft_scale = n_info, polys, tail, T, pattern, whiten, crc, soft_scale
        pat = np.array([1, 1], dtype=np.uint8) if pattern is None else pattern
        self.period = int(pat.shape[0])
        self.mask = int(sum(int(b) << i for i, b in enumerate(pat)))
        self.n_coded = int(np.resize(pat, 2 * T).sum())
        w = np.where(order == 4, 2, 1)
        self.n_need = -(-self.n_coded // w)
        self.sym_off = sym_off
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            a = np.where(order == 4, gain / math.sqrt(2.0), gain)
            good = np.isfinite(gain) & (gain > 0)
            self.scale = np.where(good, soft_scale / np.where(good, a, 1.0), 0.0).astype(np.float32)    # float64 on the host, rounded once
        good &= np.isfinite(self.scale) & (self.scale > 0)
        self.reason = np.full(order.shape[0], "", dtype=object)
        self.reason[~good] = "gain"
        self.reason[n_payload < self.n_need] = "short"
        self.valid = self.reason == ""

    def __len__(self):
        return self.valid.shape[0]

    def __repr__(self):
        return f"DecodePlan({len(self)} frames, {int(self.valid.sum())} valid, n_info={self.n_info}, T={self.T}, {self.n_coded} received bits)"

    def table(self, rotation, order):
        """The ``FECFRAME`` records of the valid frames, each writing the row of its index -> (records, the indices)."""
        at = np.flatnonzero(self.valid)
        fr = np.zeros(at.shape[0], dtype=FECFRAME)
        fr["sym_off"], fr["T"], fr["order"], fr["q"], fr["tail"], fr["row"], fr["scale"] = self.sym_off[at], self.T, order[at], rotation[at], int(self.tail), at, self.scale[at]
        return fr, at


def _plan_frames(what, frames, demodulation, n_info, whiten, crc, soft_scale, make):
    """What the plan of a decoder checks and derives whatever its code: ``frames`` and ``demodulation`` belong together; ``whiten`` (cut to the ``n_info`` information bits),
    ``crc`` and ``soft_scale``; every frame's order, gain, first payload symbol and payload symbols, from which ``make(whiten, crc, soft_scale, order, gain, sym_off,
    n_payload)`` builds the plan; a payload that no frame's code fits is refused.  -> the plan."""
    f, d = frames, demodulation
    if not all(hasattr(f, k) for k in ("plan", "clip", "word", "position", "rotation", "n_payload")) or not all(hasattr(d, k) for k in ("gain", "n_symbols", "order")):
        raise ValueError(f"{what}: give the Frames of find_frames and the Demodulation they were found in")
    fp = f.plan
    if np.asarray(d.n_symbols).shape != fp.n_symbols.shape or np.asarray(d.gain).shape != fp.n_symbols.shape \
            or not np.array_equal(np.asarray(d.n_symbols, dtype=np.int64), fp.n_symbols) or not np.array_equal(np.asarray(d.order, dtype=np.int64), fp.order):
        raise ValueError(f"{what}: the frames were not found in this demodulation (the clips' count, n_symbols or order differ)")
    if whiten is not None:
        whiten = _bit_array(what, "whiten", whiten)
        if whiten.shape[0] < n_info:
            raise ValueError(f"{what}: `whiten` holds {whiten.shape[0]} bits, fewer than n_info = {n_info}")
        whiten = whiten[:n_info].copy()
    spec = _crc_spec(what, crc, n_info)
    if isinstance(soft_scale, (bool, np.bool_)) or not isinstance(soft_scale, (int, float, np.integer, np.floating)) or not math.isfinite(float(soft_scale)) \
            or not 0.0 < float(soft_scale) <= 127.0:
        raise ValueError(f"{what}: soft_scale must be finite and in (0, 127], got {soft_scale!r}")
    clip, word = np.asarray(f.clip, dtype=np.int64), np.asarray(f.word, dtype=np.int64)
    order = fp.order[clip]
    gain = np.asarray(d.gain, dtype=np.float64)[clip]
    sym_off = fp.sym_off[clip] + np.asarray(f.position, dtype=np.int64) + fp.L[clip, word]
    plan = make(whiten, spec, float(soft_scale), order, gain, sym_off, np.asarray(f.n_payload, dtype=np.int64))
    n_least = -(-plan.n_coded // 2)
    if fp.payload < n_least:
        raise ValueError(f"{what}: the frames were read with payload = {fp.payload} symbols, but the code needs {n_least} at order 4 ({plan.n_coded} at order 2): "
                         f"no frame could be decoded")
    if order.size and fp.payload < int(plan.n_need.min()):
        raise ValueError(f"{what}: the frames were read with payload = {fp.payload} symbols, but the code needs {int(plan.n_need.min())}: no frame could be decoded")
    return plan


def plan_decode(frames, demodulation, *, n_info, polys=(0o171, 0o133), puncture=None, tail=True, whiten=None, crc=None, soft_scale=32.0):
    """The ``DecodePlan`` of ``frames`` (a ``Frames``) on ``demodulation`` (the ``Demodulation`` it was found in).  Every argument error is a ``ValueError`` raised
    here, before anything touches the device; a frame that cannot be decoded is an entry with ``valid`` False and a ``reason``."""
    what = "plan_decode"
    if not isinstance(tail, (bool, np.bool_)):
        raise ValueError(f"{what}: tail must be a bool, got {tail!r}")
    tail = bool(tail)
    T_MAX = t_max()
    if not _is_int(n_info) or n_info < 1 or n_info + (K - 1) * tail > T_MAX:
        raise ValueError(f"{what}: n_info must be an integer with 1 <= n_info and T = n_info{' + 6' if tail else ''} <= {T_MAX}, got {n_info!r}")
    n_info = int(n_info)
    T = n_info + (K - 1) * tail
    try:
        polys = tuple(polys)
    except TypeError:
        polys = ()
    if len(polys) != 2 or not all(_is_int(g) and 0 <= g < 128 and (g & 0x41) == 0x41 for g in polys):
        raise ValueError(f"{what}: polys must be two 7-bit integers with bits 6 and 0 set, got {polys!r}")
    polys = (int(polys[0]), int(polys[1]))
    pattern = None
    if puncture is not None:
        pattern = _bit_array(what, "puncture", puncture)
        if pattern.shape[0] % 2 or pattern.shape[0] > 64 or not pattern.any():
            raise ValueError(f"{what}: the puncture pattern's period must be even and at most 64, and it must hold a 1; got {pattern.tolist()}")
    return _plan_frames(what, frames, demodulation, n_info, whiten, crc, soft_scale, lambda *per_frame: DecodePlan(n_info, polys, tail, T, pattern, *per_frame))


class Decoded(BitTable):
    """One row per frame of the ``Frames``, in its order, each a numpy array over the frames: ``valid`` and ``reason`` ("short": fewer payload symbols than the
    code needs; "gain": the clip's gain is not a positive number), ``clip``, ``word``, ``position``, ``metric`` (the final path metric), ``end_state``,
    ``channel_errors`` and ``n_channel`` (received bits that differ from the re-encoded decision, of those that are not erasures), ``ber`` (their ratio, NaN at
    0), ``crc_ok`` (bool; all True without a ``crc``), ``crc_calc`` and ``crc_recv`` (uint32); an invalid frame's row is zeros (``ber`` NaN, ``crc_ok`` False).
    ``data``: (frames, bytes) uint8 on the DEVICE, the de-whitened information bits packed MSB first; ``bits(k)`` unpacks a row on the host, ``message(k)`` is
    what precedes the check field; ``soft(k)`` the frame's 2T soft bits, a device view.  ``rows`` / ``cls`` / ``conf`` / ``names`` come from the frames.  ``raw`` keeps the
    device buffers ``soft``, ``decided`` (the packed decisions of launch 2), ``out`` and ``rows`` (None when nothing was launched).  ``save(directory)`` writes ``decode.npz``
    and ``decode.json``; the table itself is ``_frame_table.BitTable``."""

    COLUMNS = ("valid", "clip", "word", "position", "metric", "end_state", "channel_errors", "n_channel", "ber", "crc_ok", "crc_calc", "crc_recv")
    STEM = "decode"

    def _header(self):
        p = self.plan
        return {"n_info": p.n_info, "polys": list(p.polys), "tail": p.tail, "puncture": None if p.pattern is None else p.pattern.tolist(),
                "whiten": None if p.whiten is None else p.whiten.tolist(), "crc": p.crc, "soft_scale": p.soft_scale}


def decode_frames(frames, demodulation, *, n_info, polys=(0o171, 0o133), puncture=None, tail=True, whiten=None, crc=None, soft_scale=32.0):
    """Decode every frame of ``frames`` (``sy11.data.frames.Frames``, found in ``demodulation``) -> ``Decoded``: three launches over all frames and one copy of
    the result rows to the host.  ``n_info``: the information bits of a frame, the check field included; ``polys``: the generators; ``puncture``: the 0/1
    pattern over the mother stream, 1 = sent; ``tail``: six zero bits end the frame; ``whiten``: the 0/1 sequence XORed onto the information bits
    (``lfsr_bits``); ``crc``: a name of ``CRCS`` or a Rocksoft dict; ``soft_scale``: the soft value of a clean component.  ``frames`` must have been read with
    ``payload`` of at least ``n_need`` symbols.  Without a valid frame nothing is launched."""
    from .. import ops
    from .frames import _packed_symbols
    f, d = frames, demodulation
    plan = plan_decode(f, d, n_info=n_info, polys=polys, puncture=puncture, tail=tail, whiten=whiten, crc=crc, soft_scale=soft_scale)
    n = len(plan)
    meta = dict(rows=f.rows, cls=f.cls, conf=f.conf, names=f.names)
    dev = f.payload.device
    n_data = (plan.n_info + 7) // 8
    cols = frame_columns(plan.valid, f, ("metric", "end_state"), channel=True)
    raw = {"soft": None, "decided": None, "out": None, "rows": None}
    fr, at = plan.table(np.asarray(f.rotation, dtype=np.int64), f.plan.order[cols["clip"]])
    if at.shape[0] == 0:
        return Decoded(plan, cols, plan.reason, torch.zeros((n, n_data), dtype=torch.uint8, device=dev), raw, **meta)
    sym = _packed_symbols(d, f.plan)
    soft = torch.zeros((n, 2 * plan.T), dtype=torch.int8, device=dev)
    decided = torch.zeros((n, (plan.T + 7) // 8), dtype=torch.uint8, device=dev)
    out = torch.zeros((n, 2), dtype=torch.int32, device=dev)
    rows = torch.zeros((n, 5), dtype=torch.int32, device=dev)
    data = torch.zeros((n, n_data), dtype=torch.uint8, device=dev)
    whiten = None if plan.whiten is None else torch.from_numpy(plan.whiten).to(dev)
    ops.fec_soft(sym, fr, soft, plan.period, plan.mask)
    ops.fec_viterbi(soft, fr, plan.polys, decided, out)
    ops.fec_check(soft, decided, fr, plan.polys, plan.n_info, data, rows, whiten=whiten, crc=plan.crc)
    raw.update(soft=soft, decided=decided, out=out, rows=rows)
    h = torch.cat((out, rows), 1).cpu().numpy()                             # one copy: metric, end state, crc_calc, crc_recv, crc_ok, errors, n_channel
    v = plan.valid
    cols["metric"][v], cols["end_state"][v] = h[v, 0], h[v, 1]
    unpack_check(cols, v, h, 2, channel=True)
    return Decoded(plan, cols, plan.reason, data, raw, **meta)
