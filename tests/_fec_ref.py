"""Numpy reference of the frame decoder ("Frame decoding"), written from the definition and independently of the package: ``encode``
(the rate 1/2, K = 7 code), ``puncture`` / ``depuncture``, ``quantize`` (one float32 product, ``np.rint``), ``received`` / ``soft`` (launch 1 for one frame),
``viterbi`` (launch 2, one frame or a batch of equal length), ``crc`` (the Rocksoft model, bit by bit), ``lfsr_bits``, ``check`` (launch 3) and ``decode`` (the chain for
one frame); ``CASES`` / ``case_clips`` / ``case_reference``: the three end-to-end clips the CPU and the GPU tests share, with the reference demodulation, frame
search and decoding of each, computed once."""
import functools
import math

import numpy as np

from tests import _frames_ref as F
from tests._demod_ref import demodulate

T_MAX = 8192
POLYS = (0o171, 0o133)
CRCS = {
    "crc8": dict(width=8, poly=0x07, init=0x00, refin=False, refout=False, xorout=0x00),
    "crc16-ccitt-false": dict(width=16, poly=0x1021, init=0xFFFF, refin=False, refout=False, xorout=0x0000),
    "crc16-x25": dict(width=16, poly=0x1021, init=0xFFFF, refin=True, refout=True, xorout=0xFFFF),
    "crc32": dict(width=32, poly=0x04C11DB7, init=0xFFFFFFFF, refin=True, refout=True, xorout=0xFFFFFFFF),
}


def parity(v):
    v = np.asarray(v).astype(np.int64)
    p = np.zeros(v.shape, dtype=np.int64)
    for i in range(8):
        p ^= (v >> i) & 1
    return p


def encode(u, polys=POLYS, tail=True):
    """The information bits ``u`` (and six zero bits with ``tail``) -> the 2T mother bits, uint8."""
    u = [int(b) for b in u] + [0] * (6 if tail else 0)
    s, c = 0, []
    for b in u:
        R = (b << 6) | s
        c += [bin(R & polys[0]).count("1") & 1, bin(R & polys[1]).count("1") & 1]
        s = R >> 1
    return np.array(c, dtype=np.uint8)


def sent_mask(pattern, n):
    """Which of the first ``n`` mother positions are sent -> bool (n,)."""
    pat = np.array([1, 1] if pattern is None else pattern, dtype=np.int64)
    return np.resize(pat, n).astype(bool)


def puncture(c, pattern):
    c = np.asarray(c)
    return c[sent_mask(pattern, c.shape[0])]


def depuncture(y, pattern, T):
    """The received soft values ``y`` -> the 2T values of the mother stream, 0 where the bit was not sent."""
    m = sent_mask(pattern, 2 * T)
    out = np.zeros(2 * T, dtype=np.int8)
    out[m] = np.asarray(y)[:int(m.sum())]
    return out


def quantize(x, scale):
    """clamp(rint(x * scale), -127, 127) as int8: one float32 product; a NaN product gives 0."""
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.asarray(x, dtype=np.float32) * np.float32(scale)
        assert p.dtype == np.float32
        r = np.rint(p)
        return np.where(np.isnan(p), 0.0, np.clip(r, -127.0, 127.0)).astype(np.int8)


def scale_of(soft_scale, gain, order):
    """float32(soft_scale / a), a = gain at order 2, gain / sqrt(2) at order 4, in float64, rounded once."""
    return np.float32(float(soft_scale) / (float(gain) / math.sqrt(2.0) if order == 4 else float(gain)))


def received(r, order, q):
    """The symbols ``r`` turned back by ``q`` steps -> the float32 components in received-bit order (Re; Re then Im at order 4)."""
    v = F.turn(r, q, order)
    return v.real.astype(np.float32) if order == 2 else np.stack((v.real, v.imag), axis=1).reshape(-1).astype(np.float32)


def n_need(T, pattern, order):
    n_coded = int(sent_mask(pattern, 2 * T).sum())
    return n_coded, -(-n_coded // (order // 2))


def soft(r, order, q, scale, pattern, T):
    """Launch 1 for one frame whose payload symbols are ``r`` -> the 2T int8 of the mother stream."""
    n_coded, need = n_need(T, pattern, order)
    return depuncture(quantize(received(np.asarray(r)[:need], order, q), scale)[:n_coded], pattern, T)


def viterbi(y, polys=POLYS, tail=True, start=False):
    """Launch 2 -> (the decided bits uint8 (T,), the final metric, the end state); for ``y`` of shape (frames, 2T) arrays over the frames.  ``start``: also
    the state in which the traceback lands."""
    y2 = np.atleast_2d(np.asarray(y)).astype(np.int64)
    n, T = y2.shape[0], y2.shape[1] // 2
    sp = np.arange(64, dtype=np.int64)
    R = [(sp << 1) | b for b in (0, 1)]
    pred = [r & 63 for r in R]
    sg = [[1 - 2 * parity(r & g) for g in polys] for r in R]
    pm = np.full((n, 64), -2 ** 30, dtype=np.int64)
    pm[:, 0] = 0
    dec = np.zeros((T, n, 64), dtype=bool)
    for t in range(T):
        y0, y1 = y2[:, 2 * t, None], y2[:, 2 * t + 1, None]
        m0 = pm[:, pred[0]] + (sg[0][0] * y0 + sg[0][1] * y1)
        m1 = pm[:, pred[1]] + (sg[1][0] * y0 + sg[1][1] * y1)
        d = m1 > m0                                                          # strictly: a tie keeps b = 0
        dec[t] = d
        pm = np.where(d, m1, m0)
    rows = np.arange(n)
    end = np.zeros(n, dtype=np.int64) if tail else np.argmax(pm, axis=1)     # the first of equal maxima: the lowest state
    metric = pm[rows, end]
    assert np.abs(pm).max() < 2 ** 31
    s, u = end.copy(), np.zeros((n, T), dtype=np.uint8)
    for t in range(T - 1, -1, -1):
        u[:, t] = s >> 5
        s = ((s << 1) | dec[t, rows, s]) & 63
    if np.asarray(y).ndim == 1:
        return (u[0], int(metric[0]), int(end[0])) + ((int(s[0]),) if start else ())
    return (u, metric, end) + ((s,) if start else ())


def crc(bits, spec):
    """The Rocksoft model over a bit sequence (with refin each group of 8 bits LSB first) -> int."""
    W = spec["width"]
    bits = [int(b) for b in bits]
    if spec["refin"]:
        assert len(bits) % 8 == 0
        bits = [bits[(k & ~7) | (7 - (k & 7))] for k in range(len(bits))]
    top, all_ = 1 << (W - 1), (1 << W) - 1
    reg = spec["init"]
    for b in bits:
        fb = (1 if reg & top else 0) ^ b
        reg = (reg << 1) & all_
        if fb:
            reg ^= spec["poly"]
    if spec["refout"]:
        reg = int(format(reg, f"0{W}b")[::-1], 2)
    return reg ^ spec["xorout"]


def bits_of_bytes(b):
    return np.unpackbits(np.frombuffer(bytes(b), dtype=np.uint8))


def int_bits(v, W):
    return np.array([(v >> (W - 1 - i)) & 1 for i in range(W)], dtype=np.uint8)


def lfsr_bits(taps, state, n):
    """A Fibonacci register: the output is the XOR of the tapped stages (1-based) and is shifted in at stage 1."""
    s = [int(b) for b in state]
    out = []
    for _ in range(n):
        b = 0
        for t in taps:
            b ^= s[t - 1]
        out.append(b)
        s = [b] + s[:-1]
    return np.array(out, dtype=np.uint8)


def check(y, u, n_info, polys=POLYS, whiten=None, crc_spec=None):
    """Launch 3 for one frame -> dict: n_channel, channel_errors, v (the de-whitened information bits), data (packed), crc_calc, crc_recv, crc_ok."""
    y, u = np.asarray(y).astype(np.int64), np.asarray(u).astype(np.uint8)
    c = encode(u, polys, tail=False)
    live = y != 0
    v = u[:n_info] ^ (np.asarray(whiten, dtype=np.uint8)[:n_info] if whiten is not None else 0)
    out = {"n_channel": int(live.sum()), "channel_errors": int((live & ((y < 0) != c.astype(bool))).sum()), "v": v.astype(np.uint8), "data": np.packbits(v),
           "crc_calc": 0, "crc_recv": 0, "crc_ok": -1}
    if crc_spec is not None:
        W = crc_spec["width"]
        out["crc_calc"] = crc(v[:n_info - W], crc_spec)
        out["crc_recv"] = int("".join(str(int(b)) for b in v[n_info - W:]), 2)
        out["crc_ok"] = int(out["crc_calc"] == out["crc_recv"])
    return out


def decode(y, n_info, polys=POLYS, tail=True, whiten=None, crc_spec=None):
    """Launches 2 and 3 for one frame's soft bits -> the dict of ``check`` plus u, metric, end_state."""
    u, metric, end = viterbi(y, polys, tail)
    out = check(y, u, n_info, polys, whiten, crc_spec)
    out.update(u=u, metric=metric, end_state=end)
    return out


def frame_bits(u, crc_spec, polys=POLYS, pattern=None, whiten=None, order=2):
    """What a transmitter sends for the message bits ``u``: the check field follows MSB first, whitening, tail, code, puncture, a 0 bit up to whole
    symbols -> (the channel bits, the information bits before whitening)."""
    info = np.concatenate((np.asarray(u, dtype=np.uint8), int_bits(crc(u, crc_spec), crc_spec["width"]))) if crc_spec is not None else np.asarray(u, dtype=np.uint8)
    sent = info ^ (np.asarray(whiten, dtype=np.uint8)[:info.shape[0]] if whiten is not None else 0)
    c = puncture(encode(sent, polys, True), pattern)
    if order == 4 and c.shape[0] % 2:
        c = np.concatenate((c, [0]))
    return c.astype(np.uint8), info


# ------------------------------------------------------------------------------------------------------- the shared clips
FS, SPAN, BIN, THRESHOLD, CRC = 1.0e6, 8, 1.0 / 1024, 0.6, "crc16-ccitt-false"
P64 = (1, 1, 0, 1, 1, 0)
# label, order, sps, M, offset (cycles / sample), snr_db, seed, stream indices of the frames, message bits per frame, puncture pattern
CASES = (
    ("a: qpsk 2.5, 2 dB", 4, 2.5, 3000, 0.02, 2.0, 62, (80, 500), 200, None),
    ("b: bpsk 3.3, 0 dB", 2, 3.3, 6000, 5.3 / 64, 0.0, 61, (60, 700), 200, None),
    ("c: qpsk 2.5, 4 dB, punctured", 4, 2.5, 3000, 0.02, 4.0, 62, (80, 500), 296, P64),
)


def word_bits(order):
    return tuple(int(b) for b in np.random.default_rng(101).integers(0, 2, 32 * (order // 2)))


@functools.lru_cache(maxsize=None)
def case_clips():
    """-> tuple of dicts per entry of ``CASES``: x, d, u0, fs, sps, rate / offset (Hz, as handed over: -1/4 and +1/16 bin off), order, bits (the word), at,
    u (the message bits of each frame), info (its information bits), n_info, T, pattern, n_coded, n_need, label."""
    out = []
    for label, order, sps, M, off, snr, seed, at, n_u, pattern in CASES:
        spec = CRCS[CRC]
        bits = word_bits(order)
        w = F.decisions(bits, order)
        g = np.random.default_rng(1000 + seed)
        us, infos, embed = [], [], {}
        for j in at:
            u = g.integers(0, 2, n_u).astype(np.uint8)
            c, info = frame_bits(u, spec, POLYS, pattern, None, order)
            us.append(u), infos.append(info)
            embed[j] = np.concatenate((w, F.decisions(c, order)))
        n_info = n_u + spec["width"]
        n_coded, need = n_need(n_info + 6, pattern, order)
        x, d, u0 = F.clip(order, M, seed, sps, off, snr, embed, span=SPAN)
        out.append({"label": label, "x": x, "d": d, "u0": u0, "fs": FS, "sps": sps, "rate": (1.0 / sps - 0.25 * BIN) * FS, "offset": (off + BIN / 16) * FS, "order": order,
                    "bits": bits, "at": at, "u": us, "info": infos, "n_info": n_info, "T": n_info + 6, "pattern": pattern, "n_coded": n_coded, "n_need": need})
    return tuple(out)


def decode_found(r, found, gain, order, L, c, soft_scale=32.0):
    """The reference decoder on every hit of ``found`` (``_frames_ref.find`` of the symbols ``r``) -> list of dicts (None for a hit cut short)."""
    out = []
    for p, q, n_pay in zip(found["position"], found["rotation"], found["n_payload"]):
        if n_pay < c["n_need"]:
            out.append(None)
            continue
        y = soft(r[int(p) + L:int(p) + L + c["n_need"]], order, int(q), scale_of(soft_scale, gain, order), c["pattern"], c["T"])
        dec = decode(y, c["n_info"], POLYS, True, None, CRCS[CRC])
        dec["soft"] = y
        out.append(dec)
    return out


@functools.lru_cache(maxsize=None)
def case_reference():
    """-> tuple per clip of (the reference demodulation, the reference search of its float32-rounded r at threshold 0.6 with n_need payload symbols, the
    reference decoding of every hit, the index in the sent stream of the first symbol).  Computed once; leave it unchanged."""
    out = []
    for c in case_clips():
        ref = demodulate(c["x"], c["fs"], c["rate"], c["offset"], c["order"], span=SPAN)
        r = ref["r"].astype(np.complex64)
        found = F.find(r, c["bits"], c["order"], THRESHOLD, c["n_need"])
        out.append((ref, found, decode_found(r, found, ref["gain"], c["order"], 32, c), F.stream_index(ref["T0"], ref["STEP"], ref["i_first"], c["sps"], c["u0"], SPAN)))
    return tuple(out)
