"""Correct the decoded frames on the GPU: the host plan of ``csrc/rs.hip`` (the Reed-Solomon codewords of every frame de-interleaved and corrected in ONE
launch; the sums of a frame and the CRC of its information bytes in a second), ``correct_decoded`` and the ``Corrected`` result; ``gf_tables``,
``rs_generator`` and ``rs_encode`` are the host side of the code, as ``lfsr_bits`` is of the whitening.

Definition.

    field     GF(2^8) modulo ``poly``, 9 bits with bit 8 set, primitive (x has order 255);  alpha = 0x02
    code      n bytes of which k carry information, 1 <= k < n <= 255, nroots = n - k in [1, 64], t = nroots // 2;  fcr in [0, 254];  prim in [1, 254],
              gcd(prim, 255) = 1;  c[0] is the coefficient of x^(n-1), the first k bytes are the information, the last nroots the parity;
              c is a codeword iff S_j = sum_i c[i] alpha^(prim (fcr + j) (n - 1 - i)) = 0, j in [0, nroots);  n < 255: the missing leading bytes are zero
    layout    a frame's row of ``Decoded.data`` holds n_info bits packed MSB first;  byte offset + m, m in [0, I n), is byte m // I of codeword m % I,
              I = interleave in [1, 8];  8 (offset + I n) <= n_info
    launch 1  per (frame, codeword), received word r: the codeword c with d(c, r) <= t if there is one (it is unique): errors = d(c, r), bit_errors =
              popcount(c ^ r);  else errors = -1, bit_errors = 0 and the bytes pass through.  info[f, w k .. (w + 1) k) = the information bytes of codeword w
    launch 2  per frame: n_failed, the sums of errors and bit_errors over the corrected codewords;  crc_recv = the last width / 8 bytes of info[f], MSB first,
              crc_calc over the bytes before them (the Rocksoft model of ``decode``, whole bytes)

The CCSDS presets use the CONVENTIONAL basis: a byte is the field element its bits spell.  The dual basis of the CCSDS recommendation (a fixed 8 x 8 bit
matrix applied to every byte before and after the code) is out of scope; so are erasures, other fields and convolutional interleavers.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from ._frame_table import FrameTable, frame_columns, unpack_check
from .decode import _crc_spec, _is_int

# n, k, the field polynomial, the first consecutive root and the primitive element's power
CODES = {
    "dvb-204-188": dict(n=204, k=188, poly=0x11D, fcr=0, prim=1),
    "rs-255-239": dict(n=255, k=239, poly=0x11D, fcr=0, prim=1),
    "ccsds-255-223": dict(n=255, k=223, poly=0x187, fcr=112, prim=11),
    "ccsds-255-239": dict(n=255, k=239, poly=0x187, fcr=120, prim=11),
}
NROOTS_MAX, I_MAX = 64, 8
REASONS = ("undecoded",)                                       # the frame was not decoded (``Decoded.valid`` False)


def gf_tables(poly, what="gf_tables"):
    """The field modulo ``poly`` -> (exp (512,) uint8 with exp[e] = exp[e + 255] = alpha^e for e < 255, log (256,) uint8 with log[alpha^e] = e, log[0] = 0).  A
    ``poly`` that does not have 9 bits, or under which x does not have order 255, is a ``ValueError``."""
    if not _is_int(poly) or not 0x100 <= poly <= 0x1FF:
        raise ValueError(f"{what}: the field polynomial must be an integer of 9 bits (bit 8 set), got {poly!r}")
    exp, log = np.zeros(512, dtype=np.uint8), np.zeros(256, dtype=np.uint8)
    v = 1
    for e in range(255):
        if e and v == 1:
            raise ValueError(f"{what}: the field polynomial 0x{int(poly):X} is not primitive (x has order {e})")
        exp[e] = exp[e + 255] = v
        log[v] = e
        v <<= 1
        if v & 0x100:
            v ^= int(poly)
    if v != 1:
        raise ValueError(f"{what}: the field polynomial 0x{int(poly):X} is not primitive (x does not have order 255)")
    return exp, log


def _code_spec(what, code):
    """A preset's name or a dict n, k, poly, fcr, prim -> the checked dict, with its ``name`` (None for a dict)."""
    if isinstance(code, str):
        if code not in CODES:
            raise ValueError(f"{what}: code {code!r} is not one of {sorted(CODES)}")
        spec = dict(CODES[code], name=code)
    elif isinstance(code, dict):
        if set(code) - {"name"} != {"n", "k", "poly", "fcr", "prim"}:
            raise ValueError(f"{what}: a code dict holds n, k, poly, fcr and prim, got {sorted(code)}")
        spec = dict(code)
        spec.setdefault("name", None)
    else:
        raise ValueError(f"{what}: code must be a name of CODES or a dict, got {code!r}")
    for key in ("n", "k", "poly", "fcr", "prim"):
        if not _is_int(spec[key]):
            raise ValueError(f"{what}: the code's {key} must be an integer, got {spec[key]!r}")
        spec[key] = int(spec[key])
    n, k = spec["n"], spec["k"]
    if not 1 <= k < n <= 255:
        raise ValueError(f"{what}: the code's n and k must satisfy 1 <= k < n <= 255, got n = {n}, k = {k}")
    if n - k > NROOTS_MAX:
        raise ValueError(f"{what}: the code's nroots = n - k = {n - k} exceeds {NROOTS_MAX}")
    if not 0 <= spec["fcr"] <= 254:
        raise ValueError(f"{what}: the code's fcr must be in [0, 254], got {spec['fcr']}")
    if not 1 <= spec["prim"] <= 254 or math.gcd(spec["prim"], 255) != 1:
        raise ValueError(f"{what}: the code's prim must be in [1, 254] and coprime to 255, got {spec['prim']}")
    gf_tables(spec["poly"], what)
    return spec


def rs_generator(code):
    """The generator polynomial prod_j (x - alpha^(prim (fcr + j))), j in [0, nroots), of ``code`` (a name of ``CODES`` or a dict) -> uint8 (nroots + 1,), the
    highest coefficient (1) first."""
    c = _code_spec("rs_generator", code)
    exp, log = gf_tables(c["poly"])
    g = [1]
    for j in range(c["n"] - c["k"]):
        r = (c["prim"] * (c["fcr"] + j)) % 255                               # log of the root
        g = [a ^ (int(exp[int(log[b]) + r]) if b else 0) for a, b in zip(g + [0], [0] + g)]
    return np.array(g, dtype=np.uint8)


def rs_encode(message_bytes, code, interleave=1):
    """What a transmitter sends for ``message_bytes`` (``interleave * k`` bytes, the information of codeword 0 first: the layout of ``Corrected.data``): every k bytes
    get their nroots parity bytes, and the codewords are interleaved byte by byte -> uint8 (interleave * n,)."""
    what = "rs_encode"
    c = _code_spec(what, code)
    if not _is_int(interleave) or not 1 <= interleave <= I_MAX:
        raise ValueError(f"{what}: interleave must be an integer in [1, {I_MAX}], got {interleave!r}")
    n, k, I = c["n"], c["k"], int(interleave)
    m = np.frombuffer(bytes(message_bytes), dtype=np.uint8) if isinstance(message_bytes, (bytes, bytearray)) else np.asarray(message_bytes)
    if m.ndim != 1 or m.shape[0] != I * k or not (np.issubdtype(m.dtype, np.integer) and ((m >= 0) & (m <= 255)).all()):
        raise ValueError(f"{what}: the message must be {I} x {k} = {I * k} bytes, got an array of shape {m.shape}")
    exp, log = gf_tables(c["poly"])
    g = rs_generator(c)[1:]
    lg, gz = log[g].astype(np.int64), g == 0                                # a coefficient may be zero
    out = np.zeros((I, n), dtype=np.uint8)
    for w in range(I):
        msg = m[w * k:(w + 1) * k].astype(np.uint8)
        rem = np.zeros(n - k, dtype=np.uint8)
        for b in msg:
            fb = int(b) ^ int(rem[0])
            rem = np.concatenate((rem[1:], [0])).astype(np.uint8)
            if fb:
                rem ^= np.where(gz, 0, exp[lg + int(log[fb])]).astype(np.uint8)
        out[w, :k], out[w, k:] = msg, rem
    return np.ascontiguousarray(out.T).reshape(-1)


class CorrectPlan:
    """The arguments, checked: ``code`` (the dict with its ``name``), ``n``, ``k``, ``nroots``, ``t``, ``interleave``, ``offset``, ``n_bytes`` (= interleave k, the information bytes
    of a frame), ``crc`` (the Rocksoft dict with its ``name``, or None); per frame of the ``Decoded``: ``valid`` and ``reason`` ("" when valid, "undecoded" for a frame
    the decoder left out)."""

    def __init__(self, code, interleave, offset, crc, valid):
        self.code, self.interleave, self.offset, self.crc = code, interleave, offset, crc
        self.n, self.k = code["n"], code["k"]
        self.nroots = self.n - self.k
        self.t = self.nroots // 2
        self.n_bytes = interleave * self.k
        self.valid = np.asarray(valid, dtype=bool).copy()
        self.reason = np.where(self.valid, "", "undecoded").astype(object)

    def __len__(self):
        return self.valid.shape[0]

    def __repr__(self):
        return f"CorrectPlan({len(self)} frames, {int(self.valid.sum())} valid, {self.interleave} x RS({self.n}, {self.k}) at byte {self.offset})"


def plan_correct(decoded, *, code="dvb-204-188", interleave=1, offset=0, crc=None):
    """The ``CorrectPlan`` of ``decoded`` (a ``Decoded``).  Every argument error is a ``ValueError`` raised here, before anything touches the device; a frame that was
    not decoded is an entry with ``valid`` False and the reason "undecoded"."""
    what = "plan_correct"
    d = decoded
    if not all(hasattr(d, key) for key in ("plan", "valid", "data", "clip", "word", "position")) or not hasattr(d.plan, "n_info"):
        raise ValueError(f"{what}: give the Decoded of decode")
    spec = _code_spec(what, code)
    if not _is_int(interleave) or not 1 <= interleave <= I_MAX:
        raise ValueError(f"{what}: interleave must be an integer in [1, {I_MAX}], got {interleave!r}")
    if not _is_int(offset) or offset < 0:
        raise ValueError(f"{what}: offset must be an integer of at least 0 bytes, got {offset!r}")
    I, offset = int(interleave), int(offset)
    n_info = int(d.plan.n_info)
    if 8 * (offset + I * spec["n"]) > n_info:
        raise ValueError(f"{what}: the block of {I} x {spec['n']} bytes at byte {offset} ends beyond the frames' n_info = {n_info} bits")
    check = _crc_spec(what, crc, 1 << 40)
    if check is not None:
        if check["width"] % 8:
            raise ValueError(f"{what}: the crc's width must be whole bytes, got {check['width']} bits")
        if 8 * I * spec["k"] <= check["width"]:
            raise ValueError(f"{what}: the crc's {check['width']} bits are not shorter than the {8 * I * spec['k']} information bits")
    return CorrectPlan(spec, I, offset, check, d.valid)


class Corrected(FrameTable):
    """One row per frame of the ``Decoded``, in its order, each a numpy array over the frames: ``valid`` and ``reason`` ("undecoded": the decoder left the frame
    out), ``clip``, ``word``, ``position``, ``n_failed`` (codewords that could not be corrected), ``byte_errors`` and ``bit_errors`` (corrected, summed over the other
    codewords), ``ok`` (valid and n_failed == 0), ``crc_ok`` (bool; all True without a ``crc``), ``crc_calc`` and ``crc_recv`` (uint32); an invalid frame's row is zeros
    (``ok`` and ``crc_ok`` False).  ``errors``: (frames, interleave) int64, the byte errors corrected in every codeword, -1 for one that could not be corrected (its
    bytes pass through), 0 for an invalid frame.  ``data``: (frames, interleave k) uint8 on the DEVICE, the information bytes codeword after codeword;
    ``message(k)`` is what precedes the check field.  ``rows`` / ``cls`` / ``conf`` / ``names`` come from the frames.  ``raw`` keeps the device buffers ``cw`` and ``rows`` (None
    when nothing was launched).  ``save(directory)`` writes ``correct.npz`` and ``correct.json``; the table itself is ``_frame_table.FrameTable``."""

    COLUMNS = ("valid", "clip", "word", "position", "n_failed", "byte_errors", "bit_errors", "ok", "crc_ok", "crc_calc", "crc_recv")
    EXTRA, STEM = ("errors",), "correct"

    def __init__(self, plan, cols, reason, errors, data, raw, rows=None, cls=None, conf=None, names=None):
        super().__init__(plan, cols, reason, data, raw, rows=rows, cls=cls, conf=conf, names=names)
        self.errors = errors

    def _header(self):
        p = self.plan
        return {"code": p.code, "interleave": p.interleave, "offset": p.offset, "crc": p.crc}

    def _message(self, row):
        return row[:self.plan.n_bytes - (self.plan.crc["width"] // 8 if self.plan.crc else 0)].tobytes()


def correct_decoded(decoded, *, code="dvb-204-188", interleave=1, offset=0, crc=None):
    """Correct every valid frame of ``decoded`` (``sy11.data.decode.Decoded``) -> ``Corrected``: two launches over all frames and one copy of the result rows to the
    host.  ``code``: a name of ``CODES`` or a dict n, k, poly, fcr, prim (the CCSDS presets in the conventional basis; the dual basis is out of scope);
    ``interleave``: the codewords of a frame, interleaved byte by byte from byte ``offset`` of the frame's de-whitened bytes; ``crc``: a name of
    ``sy11.data.decode.CRCS`` or a Rocksoft dict of whole bytes, checked over the information bytes, the check field last.  Without a valid frame nothing is
    launched."""
    from .. import ops
    d = decoded
    plan = plan_correct(d, code=code, interleave=interleave, offset=offset, crc=crc)
    n, I = len(plan), plan.interleave
    meta = dict(rows=d.rows, cls=d.cls, conf=d.conf, names=d.names)
    dev = d.data.device
    cols = frame_columns(plan.valid, d, ("n_failed", "byte_errors", "bit_errors"), bools=("ok",))
    errors = np.zeros((n, I), dtype=np.int64)
    raw = {"cw": None, "rows": None}
    at = np.flatnonzero(plan.valid)
    info = torch.zeros((n, plan.n_bytes), dtype=torch.uint8, device=dev)
    if at.shape[0] == 0:
        return Corrected(plan, cols, plan.reason, errors, info, raw, **meta)
    code_args = {key: plan.code[key] for key in ("n", "k", "poly", "fcr", "prim")}
    cw = torch.zeros((n, I, 2), dtype=torch.int32, device=dev)
    rows = torch.zeros((n, 6), dtype=torch.int32, device=dev)
    ops.rs_decode(d.data.contiguous(), at, code_args, info, cw, interleave=I, offset=plan.offset)
    ops.rs_check(info, cw, at, code_args, rows, interleave=I, crc=plan.crc)
    raw.update(cw=cw, rows=rows)
    h = torch.cat((rows, cw.reshape(n, 2 * I)), 1).cpu().numpy()             # one copy: the six of launch 2, then (errors, bit_errors) per codeword
    v = plan.valid
    cols["n_failed"][v], cols["byte_errors"][v], cols["bit_errors"][v] = h[v, 0], h[v, 1], h[v, 2]
    unpack_check(cols, v, h, 3)
    cols["ok"] = v & (cols["n_failed"] == 0)
    errors[v] = h[v, 6::2]
    return Corrected(plan, cols, plan.reason, errors, info, raw, **meta)
