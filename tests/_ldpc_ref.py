"""Numpy reference of the LDPC frame decoder ("LDPC frame decoding"), written from the definition and independently of the package: ``dense_h`` (the
parity-check matrix of a base matrix, dense), ``neighbours`` (the variables of every check, read off the dense matrix), ``decode`` (launch 2: the layered
normalised min-sum decoder, a batch of frames at once, each stopping on its own), ``check`` (launch 3) and the helpers the tests share: ``staircase_base`` (a
seeded base matrix with a dual-diagonal parity part, built here and not by the package), ``encode_staircase`` and ``awgn_soft`` (BPSK over AWGN, quantised as
launch 1 quantises)."""
import numpy as np

from tests import _fec_ref as FEC

N_MAX = 16384


def dense_h(base, Z):
    """Entry -1 is the Z x Z zero block, entry s the identity shifted by s: row r of the block has its one in column (r + s) mod Z -> uint8 (mb Z, nb Z)."""
    base = np.asarray(base, dtype=np.int64)
    mb, nb = base.shape
    H = np.zeros((mb * Z, nb * Z), dtype=np.uint8)
    r = np.arange(Z)
    for i in range(mb):
        for j in range(nb):
            if base[i, j] >= 0:
                H[i * Z + r, j * Z + (r + base[i, j]) % Z] = 1
    return H


def neighbours(H, mb, Z):
    """-> list over the layers of (Z, weight) int64: the variables of each check of the layer in rising order (= rising block column)."""
    out = []
    for i in range(mb):
        rows = [np.flatnonzero(H[i * Z + r]) for r in range(Z)]
        assert len({len(v) for v in rows}) == 1
        out.append(np.stack(rows).astype(np.int64))
    return out


def decode(y, base, Z, iterations=20, scale=12):
    """Launch 2 on the soft bits ``y`` (frames, N) int8 (or (N,)) -> dict: x (frames, N) uint8, iterations, unsat (frames,), post (frames, N) int16, t_max (the
    largest |T| met, over all frames), n_clip (how often a scaled minimum exceeded 127 and was clipped).  Every frame stops after the first iteration that leaves no check unsatisfied."""
    y2 = np.atleast_2d(np.asarray(y)).astype(np.int64)
    base = np.asarray(base, dtype=np.int64)
    mb = base.shape[0]
    H = dense_h(base, Z)
    nbr = neighbours(H, mb, Z)
    F, N = y2.shape
    assert N == H.shape[1]
    Q = y2.copy()
    R = [np.zeros((F,) + v.shape, dtype=np.int64) for v in nbr]
    its, unsat = np.zeros(F, dtype=np.int64), np.zeros(F, dtype=np.int64)
    live = np.ones(F, dtype=bool)
    t_max = n_clip = 0
    for it in range(1, iterations + 1):
        f = np.flatnonzero(live)
        if f.shape[0] == 0:
            break
        for i, idx in enumerate(nbr):
            T = Q[f][:, idx] - R[i][f]                                          # (frames, Z, weight)
            t_max = max(t_max, int(np.abs(T).max()))
            s, a = T < 0, np.abs(T)
            j1 = np.argmin(a, axis=2)
            m1 = np.take_along_axis(a, j1[:, :, None], axis=2)[:, :, 0]
            rest = a.copy()
            np.put_along_axis(rest, j1[:, :, None], 1 << 40, axis=2)
            m2 = rest.min(axis=2)
            S = np.bitwise_xor.reduce(s, axis=2)
            at_j1 = np.arange(idx.shape[1])[None, None, :] == j1[:, :, None]
            mag = (scale * np.where(at_j1, m2[:, :, None], m1[:, :, None])) >> 4
            n_clip += int((mag > 127).sum())
            mag = np.minimum(mag, 127)
            Rn = np.where(S[:, :, None] ^ s, -mag, mag)
            R[i][f] = Rn
            Qf = Q[f]
            Qf[:, idx] = T + Rn                                                 # the checks of a layer share no variable
            Q[f] = Qf
        x = (Q[f] < 0).astype(np.int64)
        u = sum(((x[:, idx].sum(axis=2)) & 1).sum(axis=1) for idx in nbr)         # the rows of H one by one: x H^T without the product
        its[f], unsat[f] = it, u
        live[f[u == 0]] = False
    assert np.abs(Q).max() <= 127 * 65
    return {"x": (Q < 0).astype(np.uint8), "iterations": its, "unsat": unsat, "post": Q.astype(np.int16), "t_max": t_max, "n_clip": n_clip}


def check(y, x, K, whiten=None, crc_spec=None):
    """Launch 3 for one frame -> dict: n_channel, channel_errors, v (the de-whitened information bits), data (packed), crc_calc, crc_recv, crc_ok."""
    y, x = np.asarray(y).astype(np.int64), np.asarray(x).astype(np.uint8)
    live = y != 0
    v = x[:K] ^ (np.asarray(whiten, dtype=np.uint8)[:K] if whiten is not None else 0)
    out = {"n_channel": int(live.sum()), "channel_errors": int((live & ((y < 0) != x.astype(bool))).sum()), "v": v.astype(np.uint8), "data": np.packbits(v), "crc_calc": 0,
           "crc_recv": 0, "crc_ok": -1}
    if crc_spec is not None:
        W = crc_spec["width"]
        out["crc_calc"] = FEC.crc(v[:K - W], crc_spec)
        out["crc_recv"] = int("".join(str(int(b)) for b in v[K - W:]), 2)
        out["crc_ok"] = int(out["crc_calc"] == out["crc_recv"])
    return out


# ------------------------------------------------------------------------------------------------------- helpers the tests share
def staircase_base(kb, mb, Z, seed, weight):
    """A seeded mb x (kb + mb) base matrix: ``weight`` information entries a row with random shifts, every information column used, and a parity part with shift
    0 on the diagonal and on the one below it."""
    g = np.random.default_rng(seed)
    base = np.full((mb, kb + mb), -1, dtype=np.int64)
    assert weight <= kb <= mb * weight
    order = g.permutation(kb)
    for t, j in enumerate(order):
        base[t % mb, j] = g.integers(0, Z)
    for i in range(mb):
        free = np.flatnonzero(base[i, :kb] < 0)
        more = weight - (kb - free.shape[0])
        for j in g.choice(free, more, replace=False):
            base[i, j] = g.integers(0, Z)
        base[i, kb + i] = 0
        if i:
            base[i, kb + i - 1] = 0
    return base


def encode_staircase(u, base, Z):
    """The codeword of the information bits ``u`` (K,) under a base matrix of ``staircase_base``: parity block i = the information part's sum of layer i + parity block
    i - 1 -> uint8 (N,)."""
    base = np.asarray(base, dtype=np.int64)
    mb, nb = base.shape
    kb = nb - mb
    H = dense_h(base, Z)
    s = (H[:, :kb * Z].astype(np.int64) @ np.asarray(u, dtype=np.int64)) & 1
    p = np.zeros((mb, Z), dtype=np.int64)
    for i in range(mb):
        p[i] = s[i * Z:(i + 1) * Z] ^ (p[i - 1] if i else 0)
    c = np.concatenate((np.asarray(u, dtype=np.int64), p.reshape(-1))).astype(np.uint8)
    assert not ((H.astype(np.int64) @ c) & 1).any()
    return c


def awgn_soft(c, ebn0_db, rate, g, soft_scale=16.0):
    """BPSK (bit 0 -> +1) over AWGN at Eb/N0, quantised like launch 1: clamp(rint(x soft_scale), -127, 127) -> int8."""
    sigma = np.sqrt(1.0 / (2.0 * rate * 10.0 ** (ebn0_db / 10.0)))
    x = (1.0 - 2.0 * np.asarray(c, dtype=np.float64)) + sigma * g.standard_normal(np.shape(c))
    return FEC.quantize(x.astype(np.float32), soft_scale)
