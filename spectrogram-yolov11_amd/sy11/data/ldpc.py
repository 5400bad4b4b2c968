"""Decode the frames of a quasi-cyclic LDPC code on the GPU: the host plan of ``csrc/ldpc.hip`` (the soft bits of every frame's payload symbols in ONE launch, the
launch 1 of ``decode`` unchanged; the layered normalised min-sum decoder in a second; the channel error count, the de-whitened information bits and their CRC in
a third), ``decode_ldpc_frames`` and the ``LdpcDecoded`` result; ``ldpc_code``, ``ldpc_staircase`` and ``ldpc_encode`` are the host side of the code.

Definition.  A code is ``{"Z": int, "base": mb x nb integers}``: entry -1 is the Z x Z zero block, entry s in [0, Z) the identity shifted by s, row r
of block (i, j) has its one in column (r + s) mod Z.  N = nb Z, M = mb Z, K = N - M; the first K bits of a codeword are the information.  Codeword bit m is
received bit m: component m % w of payload symbol m // w.

    limits    1 <= mb <= 64, mb < nb <= 128, 1 <= Z <= 512;  N even and <= 16384 (``n_max()``);  every row weight in [2, 32], every column weight >= 1;
              2 N + 8 M + 4 entries within the 160 KiB of LDS of a compute unit
    launch 1  y[n] = clamp(rintf(x * scale_k), -127, 127), NaN -> 0, as ``decode`` (``sy11_fec_soft`` with T = N / 2, no tail, nothing punctured);  y > 0 = bit 0
    launch 2  Q[n] = y[n], R[c, j] = 0;  iteration it = 1 .. iterations, layer i = 0 .. mb - 1, every check c = i Z + r of the layer with its variables n_j in rising j:
              T_j = Q[n_j] - R[c, j],  s_j = T_j < 0,  a_j = |T_j|;  m1 = min a_j at j1,  m2 = min over j != j1,  S = XOR s_j;
              R[c, j] = (S ^ s_j ? -1 : +1) min((scale (j == j1 ? m2 : m1)) >> 4, 127);  Q[n_j] = T_j + R[c, j]
              after the mb layers x[n] = Q[n] < 0,  unsat = #{c : XOR_j x[n_j] = 1};  stop when unsat = 0
    launch 3  n_channel = #{y != 0},  channel_errors = #{y != 0 and (y < 0) != x};  v_t = x_t ^ whiten_t, t < K;  crc_recv = the last `width` bits of v, MSB first;
              crc_calc over the K - width bits before them (Rocksoft model)

Out of scope: named presets of any standard (type the base matrix in), shortening and puncturing, circulants of weight above 1, N above 16384, non-binary
codes, offset min-sum and sum-product, an outer BCH code, soft output to a later stage beyond ``posterior``.
"""
from __future__ import annotations

import numpy as np
import torch

from ._frame_table import BitTable, frame_columns, unpack_check
from .decode import DecodePlan, _is_int, _plan_frames

# laid out as sy11_ldpc_entry (include/sy11.h)
LDPCENTRY = np.dtype([("column", "<i4"), ("shift", "<i4")])

MB_MAX, NB_MAX, Z_MAX, WEIGHT_MIN, WEIGHT_MAX, ITER_MAX, SCALE_MAX = 64, 128, 512, 2, 32, 100, 16
LDS_MAX = 160 * 1024
REASONS = ("short", "gain")                                    # fewer payload symbols than the code needs; the clip's gain is not a positive number


def n_max():
    """N_MAX: the bits of a codeword at the most, a constant of the library's build (``sy11_ldpc_nmax``)."""
    from .. import _lib
    return int(_lib.load().sy11_ldpc_nmax())


class LdpcCode:
    """A checked code: ``Z``, ``base`` (mb x nb int64), ``mb``, ``nb``, ``N``, ``M``, ``K``; ``layer`` (int32, mb + 1: layer i holds the entries layer[i] .. layer[i + 1]) and
    ``entry`` (``LDPCENTRY`` records, a layer's in rising column): the tables ``sy11_ldpc_decode`` takes.  The encoder's elimination is cached here."""

    def __init__(self, base, Z):
        self.base, self.Z = base, Z
        self.mb, self.nb = base.shape
        self.N, self.M = self.nb * Z, self.mb * Z
        self.K = self.N - self.M
        i, j = np.nonzero(base >= 0)                                             # row-major: rising column within a row
        self.entry = np.zeros(i.shape[0], dtype=LDPCENTRY)
        self.entry["column"], self.entry["shift"] = j, base[i, j]
        self.layer = np.concatenate(([0], np.cumsum((base >= 0).sum(axis=1)))).astype(np.int32)
        self._inverse = None

    def __repr__(self):
        return f"LdpcCode({self.mb} x {self.nb}, Z={self.Z}: N={self.N}, K={self.K}, {self.entry.shape[0]} entries)"

    def spec(self):
        return {"Z": self.Z, "base": self.base.tolist()}


def ldpc_code(base, Z, what="ldpc_code"):
    """The checked ``LdpcCode`` of the base matrix ``base`` (mb x nb integers, -1 = no block, else the shift) with circulants of size ``Z``.  A broken limit is a
    ``ValueError`` that names the offending row, column or entry."""
    if not _is_int(Z) or not 1 <= Z <= Z_MAX:
        raise ValueError(f"{what}: Z must be an integer in [1, {Z_MAX}], got {Z!r}")
    Z = int(Z)
    try:
        b = np.asarray(base)
    except (TypeError, ValueError):
        b = np.zeros(0, dtype=object)
    if isinstance(base, (str, bytes)) or b.ndim != 2 or b.dtype == bool or not np.issubdtype(b.dtype, np.integer):
        raise ValueError(f"{what}: `base` must be a 2-D array of integers (-1 or a shift), got an array of shape {b.shape} and dtype {b.dtype}")
    b = b.astype(np.int64)
    mb, nb = b.shape
    if not 1 <= mb <= MB_MAX or not mb < nb <= NB_MAX:
        raise ValueError(f"{what}: `base` must have 1 <= mb <= {MB_MAX} rows and mb < nb <= {NB_MAX} columns, got {mb} x {nb}")
    N = nb * Z
    if N % 2 or N > n_max():
        raise ValueError(f"{what}: N = nb Z = {nb} x {Z} = {N} must be even and at most {n_max()}")
    bad = (b < -1) | (b >= Z)
    if bad.any():
        i, j = (int(v[0]) for v in np.nonzero(bad))
        raise ValueError(f"{what}: entry ({i}, {j}) of `base` is {int(b[i, j])}, not -1 or a shift in [0, {Z})")
    weight = (b >= 0).sum(axis=1)
    bad = (weight < WEIGHT_MIN) | (weight > WEIGHT_MAX)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise ValueError(f"{what}: row {i} of `base` has weight {int(weight[i])}, not in [{WEIGHT_MIN}, {WEIGHT_MAX}]")
    empty = (b >= 0).sum(axis=0) == 0
    if empty.any():
        raise ValueError(f"{what}: column {int(np.flatnonzero(empty)[0])} of `base` has no entry")
    from .. import _lib
    lds = int(_lib.load().sy11_ldpc_lds_bytes(Z, mb, nb, int(weight.sum())))
    if lds > LDS_MAX:
        raise ValueError(f"{what}: the code ({mb} x {nb}, Z = {Z}) takes {lds} bytes of LDS (2 N + 8 M + 4 entries), more than the {LDS_MAX} of a compute unit")
    return LdpcCode(b, Z)


def _code_of(what, code):
    """An ``LdpcCode`` or a dict Z, base -> the checked ``LdpcCode``."""
    if isinstance(code, LdpcCode):
        return code
    if not isinstance(code, dict) or set(code) != {"Z", "base"}:
        raise ValueError(f"{what}: code must be an LdpcCode or a dict of Z and base, got {code!r}")
    return ldpc_code(code["base"], code["Z"], what)


def ldpc_staircase(kb, mb, Z, seed, row_weight=6):
    """A seeded IRA-style test code -> ``LdpcCode``: ``kb`` information and ``mb`` parity block columns; every row has ``row_weight`` information entries with random
    shifts and every information column is used; the parity part is block dual-diagonal with shift 0, so the code is always encodable."""
    what = "ldpc_staircase"
    for name, v in (("kb", kb), ("mb", mb), ("Z", Z), ("seed", seed), ("row_weight", row_weight)):
        if not _is_int(v) or v < (0 if name == "seed" else 1):
            raise ValueError(f"{what}: {name} must be an integer of at least {0 if name == 'seed' else 1}, got {v!r}")
    kb, mb, Z, row_weight = int(kb), int(mb), int(Z), int(row_weight)
    if row_weight > kb or kb > mb * row_weight:
        raise ValueError(f"{what}: row_weight = {row_weight} must be at most kb = {kb}, and mb row_weight = {mb * row_weight} at least kb, so that every column is used")
    g = np.random.default_rng(int(seed))
    base = np.full((mb, kb + mb), -1, dtype=np.int64)
    for t, j in enumerate(g.permutation(kb)):
        base[t % mb, j] = g.integers(0, Z)
    for i in range(mb):
        free = np.flatnonzero(base[i, :kb] < 0)
        for j in g.choice(free, row_weight - (kb - free.shape[0]), replace=False):
            base[i, j] = g.integers(0, Z)
        base[i, kb + i] = 0
        if i:
            base[i, kb + i - 1] = 0
    return ldpc_code(base, Z, what)


def _roll_rows(u, s):
    """Row r of a block shifted by s reads bit (r + s) mod Z: the bits ``u`` (..., Z) as the block's rows see them."""
    return np.roll(u, -int(s), axis=-1)


def _parity_inverse(code):
    """The inverse over GF(2) of the parity part H[:, K:], by Gaussian elimination on packed rows -> uint8 (M, M); a singular part is a ``ValueError``."""
    if code._inverse is not None:
        return code._inverse
    M, Z, kb = code.M, code.Z, code.nb - code.mb
    P = np.zeros((M, M), dtype=np.uint8)
    r = np.arange(Z)
    for i in range(code.mb):
        for j in range(kb, code.nb):
            if code.base[i, j] >= 0:
                P[i * Z + r, (j - kb) * Z + (r + code.base[i, j]) % Z] = 1
    A = np.packbits(np.concatenate((P, np.eye(M, dtype=np.uint8)), axis=1), axis=1)
    for c in range(M):
        byte, bit = c >> 3, 0x80 >> (c & 7)
        at = np.flatnonzero(A[c:, byte] & bit)
        if at.shape[0] == 0:
            raise ValueError("ldpc_encode: the parity part of the code is singular over GF(2): not encodable")
        p = c + int(at[0])
        if p != c:
            A[[c, p]] = A[[p, c]]
        rows = np.flatnonzero(A[:, byte] & bit)
        rows = rows[rows != c]
        A[rows] ^= A[c]
    code._inverse = np.unpackbits(A, axis=1)[:, M:2 * M]
    return code._inverse


def ldpc_encode(bits, code):
    """What a transmitter sends for the information bits ``bits`` ((K,) or (frames, K) of 0 / 1) under ``code`` (an ``LdpcCode`` or a dict Z, base): the codeword whose
    first K bits they are -> uint8 of the same leading shape and N bits.  The parity part is solved over GF(2) on the host: block by block when it is block
    lower-triangular with one circulant on the diagonal, else by an elimination that is cached on the code.  A singular parity part raises
    ``ValueError("... not encodable")``."""
    what = "ldpc_encode"
    cd = _code_of(what, code)
    try:
        u = np.asarray(bits)
    except (TypeError, ValueError):
        u = np.zeros(0, dtype=object)
    if u.ndim not in (1, 2) or u.shape[-1] != cd.K or u.dtype == bool or not np.issubdtype(u.dtype, np.integer) or not ((u == 0) | (u == 1)).all():
        raise ValueError(f"{what}: `bits` must be (K,) or (frames, K) integers 0 and 1 with K = {cd.K}, got an array of shape {u.shape}")
    u2 = np.atleast_2d(u).astype(np.uint8)
    F, Z, mb, kb = u2.shape[0], cd.Z, cd.mb, cd.nb - cd.mb
    ub = u2.reshape(F, kb, Z)
    s = np.zeros((F, mb, Z), dtype=np.uint8)                                    # the information part's sum of every check
    for i in range(mb):
        for j in np.flatnonzero(cd.base[i, :kb] >= 0):
            s[:, i] ^= _roll_rows(ub[:, j], cd.base[i, j])
    par = cd.base[:, kb:]
    tri = all(par[i, i] >= 0 and (par[i, i + 1:] < 0).all() for i in range(mb))
    if tri:
        p = np.zeros((F, mb, Z), dtype=np.uint8)
        for i in range(mb):
            rhs = s[:, i].copy()
            for j in np.flatnonzero(par[i, :i] >= 0):
                rhs ^= _roll_rows(p[:, j], par[i, j])
            p[:, i] = np.roll(rhs, int(par[i, i]), axis=-1)
    else:
        inv = _parity_inverse(cd)
        p = ((s.reshape(F, -1).astype(np.int64) @ inv.T.astype(np.int64)) & 1).astype(np.uint8)
    c = np.concatenate((u2, p.reshape(F, -1)), axis=1)
    return c[0] if u.ndim == 1 else c


class LdpcPlan(DecodePlan):
    """The arguments, checked: ``code`` (the ``LdpcCode``), ``N``, ``M``, ``n_info`` (= K), ``iterations``, ``scale`` (sixteenths), ``whiten`` (uint8 of K bits, or None), ``crc`` (the
    Rocksoft dict with its ``name``, or None), ``soft_scale``; per frame of the ``Frames``: ``valid``, ``reason`` ("" when valid), ``n_need`` (= ceil(N / w) payload symbols),
    ``scale`` (the quantiser's float32 scale, computed by ``DecodePlan`` as ``decode`` computes it; the min-sum normalisation is ``scale16``) and ``sym_off``."""

    def __init__(self, code, iterations, scale, whiten, crc, soft_scale, order, gain, sym_off, n_payload):
        super().__init__(code.K, None, False, code.N // 2, None, whiten, crc, soft_scale, order, gain, sym_off, n_payload)
        self.code, self.N, self.M, self.iterations, self.scale16 = code, code.N, code.M, iterations, scale

    def __repr__(self):
        return f"LdpcPlan({len(self)} frames, {int(self.valid.sum())} valid, {self.code!r}, {self.iterations} iterations, scale {self.scale16}/16)"


def plan_ldpc(frames, demodulation, *, code, iterations=20, scale=12, whiten=None, crc=None, soft_scale=16.0):
    """The ``LdpcPlan`` of ``frames`` (a ``Frames``) on ``demodulation`` (the ``Demodulation`` it was found in).  Every argument error is a ``ValueError`` raised here,
    before anything touches the device; a frame that cannot be decoded is an entry with ``valid`` False and a ``reason``."""
    what = "plan_ldpc"
    cd = _code_of(what, code)
    if not _is_int(iterations) or not 1 <= iterations <= ITER_MAX:
        raise ValueError(f"{what}: iterations must be an integer in [1, {ITER_MAX}], got {iterations!r}")
    if not _is_int(scale) or not 1 <= scale <= SCALE_MAX:
        raise ValueError(f"{what}: scale must be an integer in [1, {SCALE_MAX}] (sixteenths), got {scale!r}")
    return _plan_frames(what, frames, demodulation, cd.K, whiten, crc, soft_scale, lambda *per_frame: LdpcPlan(cd, int(iterations), int(scale), *per_frame))


class LdpcDecoded(BitTable):
    """One row per frame of the ``Frames``, in its order, each a numpy array over the frames: ``valid`` and ``reason`` ("short": fewer payload symbols than the code
    needs; "gain": the clip's gain is not a positive number), ``clip``, ``word``, ``position``, ``iterations`` (run), ``unsatisfied`` (checks the decision leaves open),
    ``converged`` (valid and none open), ``channel_errors`` and ``n_channel`` (received bits that differ from the decision, of those that are not erasures), ``ber`` (their
    ratio, NaN at 0), ``crc_ok`` (bool; all True without a ``crc``), ``crc_calc`` and ``crc_recv`` (uint32); an invalid frame's row is zeros (``ber`` NaN, ``crc_ok`` and
    ``converged`` False).  ``data``: (frames, ceil(K / 8)) uint8 on the DEVICE, the de-whitened information bits packed MSB first; ``bits(k)`` unpacks a row on the host,
    ``message(k)`` is what precedes the check field; ``soft(k)`` the frame's N soft bits and ``posterior(k)`` its N final Q (int16), device views.  ``rows`` / ``cls`` /
    ``conf`` / ``names`` come from the frames.  ``raw`` keeps the device buffers ``soft``, ``decided`` (the packed decisions of launch 2), ``out``, ``post`` and ``rows`` (None when
    nothing was launched).  It carries what ``plan_correct`` reads of a ``Decoded``, so ``correct`` takes it as it is.  ``save(directory)`` writes ``ldpc.npz`` and ``ldpc.json``;
    the table itself is ``_frame_table.BitTable``."""

    COLUMNS = ("valid", "clip", "word", "position", "iterations", "unsatisfied", "converged", "channel_errors", "n_channel", "ber", "crc_ok", "crc_calc", "crc_recv")
    STEM = "ldpc"

    def _header(self):
        p = self.plan
        return {"code": p.code.spec(), "N": p.N, "K": p.n_info, "iterations": p.iterations, "scale": p.scale16, "whiten": None if p.whiten is None else p.whiten.tolist(),
                "crc": p.crc, "soft_scale": p.soft_scale}

    def posterior(self, k):
        """The N final values Q of frame ``k``, int16 (negative = bit 1), a view of the device buffer (zeros for an invalid frame)."""
        k = range(len(self))[k]
        if self.raw["post"] is None:
            return torch.zeros(self.plan.N, dtype=torch.int16, device=self.data.device)
        return self.raw["post"][k, :self.plan.N]


def decode_ldpc_frames(frames, demodulation, *, code, iterations=20, scale=12, whiten=None, crc=None, soft_scale=16.0):
    """Decode every frame of ``frames`` (``sy11.data.frames.Frames``, found in ``demodulation``) -> ``LdpcDecoded``: three launches over all frames and one copy of the
    result rows to the host.  ``code``: an ``LdpcCode`` (``ldpc_code``, ``ldpc_staircase``) or a dict Z, base; ``iterations``: the sweeps at the most, a frame stops at the
    first that satisfies every check; ``scale``: the min-sum normalisation in sixteenths (12 = 0.75); ``whiten``: the 0/1 sequence XORed onto the K information
    bits (``sy11.data.decode.lfsr_bits``); ``crc``: a name of ``sy11.data.decode.CRCS`` or a Rocksoft dict, the check field the last bits of the K; ``soft_scale``: the soft
    value of a clean component.  ``frames`` must have been read with ``payload`` of at least ``n_need`` = ceil(N / w) symbols.  Without a valid frame nothing is
    launched."""
    from .. import ops
    from .frames import _packed_symbols
    f, d = frames, demodulation
    plan = plan_ldpc(f, d, code=code, iterations=iterations, scale=scale, whiten=whiten, crc=crc, soft_scale=soft_scale)
    n, N, K = len(plan), plan.N, plan.n_info
    meta = dict(rows=f.rows, cls=f.cls, conf=f.conf, names=f.names)
    dev = f.payload.device
    n_data = (K + 7) // 8
    cols = frame_columns(plan.valid, f, ("iterations", "unsatisfied"), bools=("converged",), channel=True)
    raw = {"soft": None, "decided": None, "out": None, "post": None, "rows": None}
    fr, at = plan.table(np.asarray(f.rotation, dtype=np.int64), f.plan.order[cols["clip"]])
    if at.shape[0] == 0:
        return LdpcDecoded(plan, cols, plan.reason, torch.zeros((n, n_data), dtype=torch.uint8, device=dev), raw, **meta)
    sym = _packed_symbols(d, f.plan)
    soft = torch.zeros((n, N), dtype=torch.int8, device=dev)
    decided = torch.zeros((n, (N + 7) // 8), dtype=torch.uint8, device=dev)
    out = torch.zeros((n, 2), dtype=torch.int32, device=dev)
    post = torch.zeros((n, N), dtype=torch.int16, device=dev)
    rows = torch.zeros((n, 5), dtype=torch.int32, device=dev)
    data = torch.zeros((n, n_data), dtype=torch.uint8, device=dev)
    whiten = None if plan.whiten is None else torch.from_numpy(plan.whiten).to(dev)
    ops.fec_soft(sym, fr, soft, 2, 3)
    ops.ldpc_decode(soft, at, plan.code, decided, out, post=post, iterations=plan.iterations, scale=plan.scale16)
    ops.ldpc_check(soft, decided, at, N, K, data, rows, whiten=whiten, crc=plan.crc)
    raw.update(soft=soft, decided=decided, out=out, post=post, rows=rows)
    h = torch.cat((out, rows), 1).cpu().numpy()                             # one copy: iterations, unsat, crc_calc, crc_recv, crc_ok, errors, n_channel
    v = plan.valid
    cols["iterations"][v], cols["unsatisfied"][v] = h[v, 0], h[v, 1]
    cols["converged"] = v & (cols["unsatisfied"] == 0)
    unpack_check(cols, v, h, 2, channel=True)
    return LdpcDecoded(plan, cols, plan.reason, data, raw, **meta)
