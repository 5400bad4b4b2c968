"""Float64 numpy reference of the frame search ("Frame search"), written from the definition and independently of the package:
``decisions`` / ``points`` (a word's bits -> decisions -> un-normalised points), ``correlate`` (rho2 and q at every position), ``peaks`` (the hits),
``turn`` / ``decide`` / ``frames`` (launch 3 for one hit: errors, bit errors, n_payload and the packed payload bytes), ``find`` (the chain for one clip
and one word); ``clip`` (a seeded generator that embeds given decision words at given symbol indices of a BPSK / four-phase stream, and
returns what was sent), ``stream_index`` (which symbol sent the demodulator's first symbol is) and ``CASES`` / ``case_clips`` / ``case_reference`` (the
four clips the CPU and the GPU tests share, and the reference demodulation and search of each, computed once)."""
import functools
import math

import numpy as np

from tests._demod_ref import demodulate, point, rrc

TILE = 256                                                     # positions per work item (sy11_sync_tile)
L_MIN, L_MAX = 8, 256


def decisions(bits, order):
    """A word's bits, first bit first -> its decisions as ``Demodulation.bits`` maps them, or None when the bit count does not divide."""
    bits = [int(b) for b in bits]
    if order == 2:
        return np.array(bits, dtype=np.uint8)
    if len(bits) % 2:
        return None
    return np.array([2 * bits[i] + bits[i + 1] for i in range(0, len(bits), 2)], dtype=np.uint8)


def points(w, order):
    """The un-normalised points of decisions: +-1 at order 2, +-1 +- i at order 4."""
    w = np.asarray(w).astype(np.int64)
    if order == 2:
        return (1.0 - 2.0 * (w & 1)).astype(np.complex128)
    return (1.0 - 2.0 * ((w >> 1) & 1)) + 1j * (1.0 - 2.0 * (w & 1))


def pair_reason(n_symbols, order, n_bits, clip_valid=True):
    """"" when the pair (clip, word) is valid, else why it is skipped."""
    if not clip_valid or order not in (2, 4) or n_symbols < 1:
        return "clip not valid"
    bps = order // 2
    if n_bits % bps:
        return "bit count not divisible by log2(order)"
    L = n_bits // bps
    if not L_MIN <= L <= L_MAX:
        return "word outside [8, 256] symbols"
    if L > n_symbols:
        return "clip shorter than the word"
    return ""


def correlate(r, w, order):
    """-> (rho2 (P,) float64, q (P,) uint8): float64 from the float32 symbols, k ascending, every product and sum rounded on its own."""
    r = np.asarray(r).astype(np.complex64)
    re, im = r.real.astype(np.float64), r.imag.astype(np.float64)
    c = points(w, order)
    L, P = len(w), r.shape[0] - len(w) + 1
    assert P >= 1
    Cr, Ci, E = np.zeros(P), np.zeros(P), np.zeros(P)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for k in range(L):
            a, b, cr, ci = re[k:k + P], im[k:k + P], c[k].real, c[k].imag
            Cr = Cr + (a * cr + b * ci)
            Ci = Ci + (b * cr - a * ci)
            E = E + (a * a + b * b)
        rho2 = np.where(E == 0.0, 0.0, (Cr * Cr + Ci * Ci) / (float((order // 2) * L) * E))
        if order == 2:
            q = (Cr < 0.0).astype(np.uint8)
        else:
            cand = (Cr, Ci, -Cr, -Ci)
            q, top = np.zeros(P, dtype=np.uint8), Cr.copy()
            for j in (1, 2, 3):
                more = cand[j] > top                                         # strictly: the lowest index wins a tie, a NaN never wins
                q[more], top[more] = j, cand[j][more]
    return rho2, q


def peaks(rho2, L, thr2):
    """-> hit (P,) uint8: at least thr2, no earlier position within L - 1 at least as large, no later one within L - 1 larger."""
    P = rho2.shape[0]
    hit = np.zeros(P, dtype=np.uint8)
    for p in range(P):
        v = rho2[p]
        if not v >= thr2:
            continue
        before, after = rho2[max(p - L + 1, 0):p], rho2[p + 1:min(p + L - 1, P - 1) + 1]
        with np.errstate(invalid="ignore"):
            hit[p] = not ((before >= v).any() or (after > v).any())
    return hit


def turn(r, q, order):
    """r turned back by q steps of 2 pi / order, exactly (complex64 in, complex64 out)."""
    r = np.asarray(r).astype(np.complex64)
    re, im = r.real, r.imag
    re, im = ((re, im), (-re, -im))[q] if order == 2 else ((re, im), (im, -re), (-re, -im), (-im, re))[q]
    out = np.empty(r.shape, dtype=np.complex64)                             # the planes one by one: a complex product would spread a NaN
    out.real, out.imag = re, im
    return out


def decide(v, order):
    v = np.asarray(v)
    return (v.real < 0).astype(np.uint8) if order == 2 else (2 * (v.real < 0) + (v.imag < 0)).astype(np.uint8)


def bits_of(d, order):
    d = np.asarray(d).astype(np.uint8)
    return (d & 1) if order == 2 else np.stack(((d >> 1) & 1, d & 1), axis=1).reshape(-1)


def frames(r, w, order, p, q, payload, stride):
    """Launch 3 for one hit -> (errors, bit_errors, n_payload, the row's ``stride`` payload bytes)."""
    L, N = len(w), len(r)
    n_pay = min(payload, N - p - L)
    d = decide(turn(r[p:p + L + n_pay], q, order), order)
    mask = 1 if order == 2 else 3
    diff = d[:L] ^ (np.asarray(w, dtype=np.uint8) & mask)
    packed = np.packbits(bits_of(d[L:], order))
    row = np.zeros(stride, dtype=np.uint8)
    row[:packed.shape[0]] = packed
    return int((diff != 0).sum()), int(sum(bin(int(v)).count("1") for v in diff)), n_pay, row


def find(r, bits, order, threshold=0.8, payload=0):
    """The chain for one clip and one word -> dict: rho2, q, hit, and per hit position, rotation, rho, errors, bit_errors, n_payload, payload (bits)."""
    w = decisions(bits, order)
    rho2, q = correlate(r, w, order)
    hit = peaks(rho2, len(w), threshold * threshold)
    stride = (payload * (order // 2) + 7) // 8
    out = {"rho2": rho2, "q": q, "hit": hit, "position": np.flatnonzero(hit), "rotation": [], "rho": [], "errors": [], "bit_errors": [], "n_payload": [], "payload": []}
    for p in out["position"]:
        e, be, n_pay, row = frames(r, w, order, int(p), int(q[p]), payload, stride)
        out["rotation"].append(int(q[p])), out["rho"].append(math.sqrt(rho2[p])), out["errors"].append(e), out["bit_errors"].append(be)
        out["n_payload"].append(n_pay), out["payload"].append(np.unpackbits(row)[:n_pay * (order // 2)])
    return out


# ---------------------------------------------------------------------------------------------------------------- generator
def clip(order, M, seed, sps, offset, snr_db, embed, beta=0.35, span=8):
    """A seeded clip of ``M`` complex64 samples shaped as ``tests/_demod_ref.clip`` shapes them, whose symbol stream is random decisions with the
    decision words of ``embed`` ({index in the stream: decisions}) written over them -> (x, d, u0): ``d`` the decisions sent (uint8) and ``u0`` the
    timing phase: sample ``n`` is taken at ``u = n / sps + u0`` symbol periods, where the symbol ``d[m + span]`` peaks at ``u = m``."""
    g = np.random.default_rng(seed)
    t = np.arange(M, dtype=np.float64)
    n_sym = int(M / sps) + 2 * span + 2
    d = g.integers(0, order, n_sym).astype(np.uint8)
    for j, w in embed.items():
        assert 0 <= j and j + len(w) <= n_sym
        d[j:j + len(w)] = w
    a = point(d, order)
    u0 = g.uniform(0.0, 1.0)
    u = t / sps + u0
    n = np.floor(u).astype(np.int64)[:, None] + np.arange(-span + 1, span + 1)[None, :]
    s = (a[n + span] * rrc(u[:, None] - n, beta)).sum(1)
    s = s / math.sqrt(np.mean(np.abs(s) ** 2))
    s = s * np.exp(2j * np.pi * (offset * t + g.uniform(0.0, 1.0)))
    sigma = math.sqrt(0.5 * 10.0 ** (-snr_db / 10.0))
    return (s + sigma * (g.standard_normal(M) + 1j * g.standard_normal(M))).astype(np.complex64), d, u0


def stream_index(T0, STEP, i_first, sps_true, u0, span=8):
    """The index in the sent stream ``d`` of the demodulator's first symbol: it is taken at ``(T0 + i_first STEP) 2^-32`` samples."""
    return int(round((T0 + i_first * STEP) / 2.0 ** 32 / sps_true + u0)) + span


# ------------------------------------------------------------------------------------------------------- the shared clips
FS = 1.0e6
SPAN = 8
BIN = 1.0 / 1024
PAYLOAD = 40
BARKER13 = (0, 0, 0, 0, 0, 1, 1, 0, 0, 1, 0, 1, 0)
# label, order, M, D, sps, offset (cycles / sample), snr_db, rate error (bins), offset error (bins), word bits, stream indices of the frames, seed.
# The rates are handed over 1/4 bin off and the offsets 1/16 bin off, as the demodulation's cases are.  The data around the frames is
# random: at 13 symbols a random BPSK window reaches rho 0.8 once in about 300 positions, so the seed of that clip is one whose 550
# positions hold none ACCORDING TO THE REFERENCE (tests/test_frames_cpu.py asserts it); the longer words have no such chance.
# The seed of the third clip is one at which the demodulator lands a quarter turn off, so that the sense of ``rotation`` is tested.
CASES = (
    ("bpsk 3.3", 2, 3000, 1, 3.3, 5.3 / 64, 20.0, 0.25, 1.0 / 16, tuple(int(b) for b in np.random.default_rng(101).integers(0, 2, 32)), (60, 350, 700), 61),
    ("qpsk 2.5", 4, 3000, 1, 2.5, 0.02, 12.0, -0.25, 1.0 / 16, tuple(int(b) for b in np.random.default_rng(102).integers(0, 2, 48)), (80, 500, 1000), 62),
    ("qpsk 7.3", 4, 8400, 2, 7.3, -0.03, 20.0, -0.25, -1.0 / 16, tuple(int(b) for b in np.random.default_rng(103).integers(0, 2, 32)), (100, 800), 68),
    ("bpsk 16", 2, 9000, 1, 16.0, 0.004, 20.0, 0.25, -1.0 / 16, BARKER13, (40, 250, 470), 64),
)


@functools.lru_cache(maxsize=None)
def case_clips():
    """-> tuple of dicts per entry of ``CASES``: x, d, u0, fs, D, sps (true), rate / offset (Hz, as handed over), order, bits, at, label."""
    out = []
    for label, order, M, D, sps, off, snr, dr, do, bits, at, seed in CASES:
        fs = FS / D
        w = decisions(bits, order)
        x, d, u0 = clip(order, M, seed, sps, off, snr, {j: w for j in at}, span=SPAN)
        out.append({"label": label, "x": x, "d": d, "u0": u0, "fs": fs, "D": D, "sps": sps, "rate": (1.0 / sps + dr * BIN) * fs, "offset": (off + do * BIN) * fs,
                    "order": order, "bits": bits, "at": at})
    return tuple(out)


@functools.lru_cache(maxsize=None)
def case_reference():
    """-> tuple per clip of (the reference demodulation, the reference search of its float32-rounded r at threshold 0.8 with 40 payload
    symbols, the index in the sent stream of its first symbol).  Computed once; leave it unchanged."""
    out = []
    for c in case_clips():
        ref = demodulate(c["x"], c["fs"], c["rate"], c["offset"], c["order"], span=SPAN)
        found = find(ref["r"].astype(np.complex64), c["bits"], c["order"], 0.8, PAYLOAD)
        out.append((ref, found, stream_index(ref["T0"], ref["STEP"], ref["i_first"], c["sps"], c["u0"], SPAN)))
    return tuple(out)
