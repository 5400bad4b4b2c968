"""Numpy / Python reference of the Reed-Solomon outer decoder ("Frame correction"), written from the definition and independently of
the package (it imports nothing of ``sy11``).  The field product is shift-and-reduce (``mul`` on ints, ``gf_mul`` on arrays), the encoder a polynomial
division, and the decoder takes another route than the kernel: the Euclidean (Sugiyama) algorithm for the key equation, then the roots by trying
all 255 positions.  Whatever it finds is checked against the definition before it is accepted: the corrected word has zero syndromes under the
slow product and lies within t bytes of the received one; everything else is a failure and passes through.

    code      dict n, k, poly, fcr, prim;  c[0] is the coefficient of x^(n-1), the first k bytes are the information
    layout    byte offset + m of a frame's row is byte m // I of codeword m % I
"""
import functools

import numpy as np

CODES = {
    "dvb-204-188": dict(n=204, k=188, poly=0x11D, fcr=0, prim=1),
    "rs-255-239": dict(n=255, k=239, poly=0x11D, fcr=0, prim=1),
    "ccsds-255-223": dict(n=255, k=223, poly=0x187, fcr=112, prim=11),
    "ccsds-255-239": dict(n=255, k=239, poly=0x187, fcr=120, prim=11),
}


def code(n, k, poly=0x11D, fcr=0, prim=1):
    return dict(n=n, k=k, poly=poly, fcr=fcr, prim=prim)


# ------------------------------------------------------------------------------------------------------------- the field
def mul(a, b, poly):
    """The product of two field elements (ints) by shift-and-reduce."""
    p = 0
    for _ in range(8):
        if b & 1:
            p ^= a
        b >>= 1
        a <<= 1
        if a & 0x100:
            a ^= poly
    return p


def gf_mul(a, b, poly):
    """The same product over integer arrays, broadcast."""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64))
    a, b = a.copy(), b.copy()
    p = np.zeros(a.shape, dtype=np.int64)
    for _ in range(8):
        p ^= np.where(b & 1, a, 0)
        b >>= 1
        a <<= 1
        a ^= np.where(a & 0x100, poly, 0)
    return p


def power(a, e, poly):
    """a^e for a != 0, any integer e (the exponent is taken modulo 255)."""
    e %= 255
    v = 1
    while e:
        if e & 1:
            v = mul(v, a, poly)
        a = mul(a, a, poly)
        e >>= 1
    return v


def inv(a, poly):
    assert a != 0
    return power(a, 254, poly)


def order_of_x(poly):
    v, n = 2, 1
    while v != 1 and n < 256:
        v, n = mul(v, 2, poly), n + 1
    return n


def roots_of(cd):
    """The nroots consecutive roots alpha^(prim (fcr + j)) of the generator."""
    return [power(2, cd["prim"] * (cd["fcr"] + j), cd["poly"]) for j in range(cd["n"] - cd["k"])]


# ------------------------------------------------------------------------------------------------------------- the code
def generator(cd):
    """prod_j (x - root_j), the highest coefficient (1) first."""
    g = [1]
    for r in roots_of(cd):
        g = [a ^ mul(b, r, cd["poly"]) for a, b in zip(g + [0], [0] + g)]
    return g


def encode(msg, cd):
    """The k information bytes ``msg`` ((k,) or (words, k)) -> the codewords (n,) / (words, n): the remainder of msg(x) x^nroots by the generator follows them."""
    m = np.atleast_2d(np.asarray(msg)).astype(np.int64)
    n, k = cd["n"], cd["k"]
    assert m.shape[1] == k
    g = np.array(generator(cd)[1:], dtype=np.int64)
    rem = np.zeros((m.shape[0], n - k), dtype=np.int64)
    for i in range(k):
        fb = m[:, i] ^ rem[:, 0]
        rem = np.concatenate((rem[:, 1:], np.zeros((m.shape[0], 1), dtype=np.int64)), axis=1) ^ gf_mul(fb[:, None], g[None, :], cd["poly"])
    out = np.concatenate((m, rem), axis=1).astype(np.uint8)
    return out[0] if np.asarray(msg).ndim == 1 else out


def syndromes(words, cd):
    """S_j = sum_i c[i] root_j^(n - 1 - i) of every word ((words, n)) -> (words, nroots), by Horner with the slow product."""
    w = np.atleast_2d(np.asarray(words)).astype(np.int64)
    x = np.array(roots_of(cd), dtype=np.int64)[None, :]
    S = np.zeros((w.shape[0], x.shape[1]), dtype=np.int64)
    for i in range(cd["n"]):
        S = gf_mul(S, x, cd["poly"]) ^ w[:, i, None]
    return S


def interleave(cws):
    """(I, n) codewords -> the I n bytes of a frame, byte m = byte m // I of codeword m % I."""
    return np.ascontiguousarray(np.asarray(cws, dtype=np.uint8).T).reshape(-1)


def deinterleave(block, I):
    return np.ascontiguousarray(np.asarray(block, dtype=np.uint8).reshape(-1, I).T)


# ------------------------------------------------------------------------------------------------------------- the decoder
def _deg(p):
    d = len(p) - 1
    while d >= 0 and p[d] == 0:
        d -= 1
    return d


def _euclid(S, nroots, poly):
    """Extended Euclid on (x^nroots, S(x)), lowest coefficient first, until 2 deg(remainder) < nroots -> (the cofactor of S, the remainder)."""
    r0, r1 = [0] * nroots + [1], list(S)
    t0, t1 = [0], [1]
    while 2 * _deg(r1) >= nroots:
        d1 = _deg(r1)
        lead = inv(r1[d1], poly)
        q, r = [0] * len(r0), list(r0)
        while _deg(r) >= d1:
            d = _deg(r)
            c, sh = mul(r[d], lead, poly), d - d1
            q[sh] ^= c
            for i in range(d1 + 1):
                r[i + sh] ^= mul(c, r1[i], poly)
        t = list(t0) + [0] * (len(q) + len(t1))
        for i, qi in enumerate(q):
            if qi:
                for j, tj in enumerate(t1):
                    if tj:
                        t[i + j] ^= mul(qi, tj, poly)
        r0, r1, t0, t1 = r1, r, t1, t
    return t1, r1


@functools.lru_cache(maxsize=None)
def _position_roots(poly, prim):
    """beta^(-p) for the 255 positions p, beta = alpha^prim: where the locator of an error at the coefficient of x^p vanishes."""
    beta = power(2, prim, poly)
    return np.array([power(beta, -p, poly) for p in range(255)], dtype=np.int64)


def _candidate(r, S, cd):
    """The word the key equation points to for the received ``r`` with syndromes ``S`` (not all zero), or None."""
    n, k, poly, fcr, prim = cd["n"], cd["k"], cd["poly"], cd["fcr"], cd["prim"]
    nroots = n - k
    t = nroots // 2
    lam, omega = _euclid([int(v) for v in S], nroots, poly)
    L = _deg(lam)
    if L < 1 or L > t or lam[0] == 0:
        return None
    norm = inv(lam[0], poly)
    lam = [mul(v, norm, poly) for v in lam[:L + 1]]
    omega = [mul(v, norm, poly) for v in omega[:max(_deg(omega), 0) + 1]]
    beta = power(2, prim, poly)
    xinv = _position_roots(poly, prim)                             # the root that stands for the coefficient of x^p
    val = np.zeros(255, dtype=np.int64)
    for cf in reversed(lam):
        val = gf_mul(val, xinv, poly) ^ cf
    at = np.flatnonzero(val == 0)
    if at.shape[0] != L or at.max() >= n:                          # fewer roots than the degree, or one among the bytes that are not transmitted
        return None
    out = np.array(r, dtype=np.uint8)
    for p in at.tolist():
        xi, X = int(xinv[p]), power(beta, p, poly)
        num = 0
        for cf in reversed(omega):
            num = mul(num, xi, poly) ^ cf
        den = 0
        for i in range(1, L + 1, 2):                               # the derivative: the odd terms, one power lower
            den ^= mul(lam[i], power(xi, i - 1, poly), poly)
        if den == 0:
            return None
        out[n - 1 - p] ^= mul(power(X, 1 - fcr, poly), mul(num, inv(den, poly), poly), poly)
    return out


def decode(words, cd):
    """Launch 1 for received words ((words, n) uint8) -> (info (words, k) uint8, cw (words, 2) int32: errors or -1, bit_errors).  Every accepted word is
    checked again: zero syndromes and at most t bytes from the received one."""
    r = np.atleast_2d(np.asarray(words, dtype=np.uint8))
    n, k = cd["n"], cd["k"]
    t = (n - k) // 2
    assert r.shape[1] == n
    S = syndromes(r, cd)
    cand = r.copy()
    tried = np.flatnonzero(S.any(axis=1))
    for w in tried.tolist():
        c = _candidate(r[w], S[w], cd)
        if c is not None:
            cand[w] = c
    dist = (cand != r).sum(axis=1)
    good = ~syndromes(cand, cd).any(axis=1) & (dist <= t)           # the definition, whatever the route was
    assert good[dist == 0].sum() == (~S.any(axis=1)).sum()
    out = np.where(good[:, None], cand, r)
    cw = np.zeros((r.shape[0], 2), dtype=np.int32)
    cw[:, 0] = np.where(good, dist, -1)
    cw[:, 1] = np.where(good, np.unpackbits(cand ^ r, axis=1).sum(axis=1), 0)
    return out[:, :k].copy(), cw


def correct_rows(data, rows, cd, I, offset):
    """Launch 1 over the frames ``rows`` of the table ``data`` ((n_rows, stride) uint8) -> (info (frames, I k) uint8, cw (frames, I, 2) int32)."""
    n, k = cd["n"], cd["k"]
    words = np.concatenate([deinterleave(data[r, offset:offset + I * n], I) for r in rows], axis=0)
    info, cw = decode(words, cd)
    return info.reshape(len(rows), I * k), cw.reshape(len(rows), I, 2)


def check(info_row, cw, crc_fn=None, spec=None):
    """Launch 2 for one frame: ``info_row`` its I k information bytes, ``cw`` (I, 2) -> [n_failed, byte_errors, bit_errors, crc_calc, crc_recv, crc_ok];
    ``crc_fn``: the Rocksoft model over a bit sequence (``tests/_fec_ref.crc``)."""
    cw = np.asarray(cw)
    ok = cw[:, 0] >= 0
    out = [int((~ok).sum()), int(cw[ok, 0].sum()), int(cw[ok, 1].sum()), 0, 0, -1]
    if spec is not None:
        nb = spec["width"] // 8
        bits = np.unpackbits(np.asarray(info_row, dtype=np.uint8))
        out[3] = int(crc_fn(bits[:bits.shape[0] - 8 * nb], spec))
        out[4] = int.from_bytes(bytes(np.asarray(info_row, dtype=np.uint8)[-nb:].tolist()), "big")
        out[5] = int(out[3] == out[4])
    return out
