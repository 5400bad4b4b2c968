"""Float64 numpy reference of the demodulation ("Demodulation"), written from the definition and independently of the
package: ``plan`` (validity, half width, tiles, Ws / Wc of one clip), ``taps``, ``filter64`` (de-rotation and matched filter), ``timing_rows`` (the
per-tile timing partials of any filtered clip), ``fit`` (the timing line and the symbol grid), ``symbols64`` (cubic interpolation), ``z_rows``,
``phase_track``, ``decide`` (phase interpolation, de-rotation, decisions and margins), ``block_rows``, ``columns``; the float32 emulations
``filter32``, ``symbols32`` and ``decide32`` of stages 2, 5 and 7; ``demodulate`` (the whole chain for one clip, with the float32 roundings of y and
s); ``clip`` (a seeded generator that also returns the transmitted symbols and the timing phase), ``errors`` (symbol errors against the
transmitted stream up to a rotation and a shift) and ``CASES`` / ``case_clips`` (the six clips the CPU and the GPU tests share)."""
import math

import numpy as np

from tests._characterize_ref import rrc

TILE = 512                                                     # usable samples per timing tile (sy11_iq_demod_tile)
TWO64 = 1 << 64


def plan(M, fs, rate, offset, order, span=8, keyed=True):
    """One clip -> dict: valid, reason, and when valid sps, hw, n_taps, tiles, Ws, Wc (Python ints)."""
    def no(why):
        return {"valid": False, "reason": why}
    if order not in (2, 4):
        return no("order is not 2 or 4")
    if not keyed:
        return no("not keyed")
    if not (math.isfinite(rate) and math.isfinite(offset)) or rate <= 0:
        return no("rate or offset not finite")
    sps = fs / rate
    if not 2.5 <= sps <= 16.0:
        return no("samples per symbol outside [2.5, 16]")
    if not abs(offset) < fs / 2:
        return no("offset beyond fs / 2")
    hw = math.ceil(span * sps)
    if M - 2 * hw < TILE:
        return no("too short")
    return {"valid": True, "reason": "", "sps": sps, "hw": hw, "n_taps": 2 * hw + 1, "tiles": -(-(M - 2 * hw) // TILE),
            "Ws": int(math.ldexp(rate / fs, 64)), "Wc": int(math.ldexp(offset / fs, 64)) % TWO64}


def taps(sps, hw, beta=0.35):
    """-> (2 hw + 1,) float32: rrc(k / sps) in float64, unit energy, rounded once."""
    h = rrc(np.arange(-hw, hw + 1, dtype=np.float64) / sps, beta)
    return (h / np.sqrt(np.sum(h * h))).astype(np.float32)


def turns(n, W):
    """(n W mod 2^64) 2^-64 as float64 in [-0.5, 0.5) for every sample index of ``n`` (the exact integer phase, then one rounding)."""
    ph = np.asarray(n, dtype=np.uint64) * np.uint64(W)                       # wraps modulo 2^64
    return ph.astype(np.int64).astype(np.float64) * 2.0 ** -64


def filter64(x, Wc, h):
    """-> y (M,) complex128: the float32 samples de-rotated by the exact integer phase and filtered with the float32 taps, in float64."""
    x = np.asarray(x).astype(np.complex64).astype(np.complex128)
    xr = x * np.exp(-2j * np.pi * turns(np.arange(x.shape[0]), Wc))
    hw = (len(h) - 1) // 2
    xp = np.concatenate((np.zeros(hw, dtype=np.complex128), xr, np.zeros(hw, dtype=np.complex128)))
    y = np.zeros(x.shape[0], dtype=np.complex128)
    for kk, v in enumerate(np.asarray(h, dtype=np.float64)):                  # y[n] += xr[n - k] h[k], k = kk - hw
        k = kk - hw
        y += xp[hw - k:hw - k + x.shape[0]] * v
    return y


def filter32(x, Wc, h):
    """Stage 2 in float32 -> complex64: the rotator rounded to complex64, complex64 products, one sequential float32 sum over the taps."""
    x = np.asarray(x).astype(np.complex64)
    rot = np.exp(-2j * np.pi * turns(np.arange(x.shape[0]), Wc)).astype(np.complex64)
    xr = x * rot
    assert xr.dtype == np.complex64
    hw = (len(h) - 1) // 2
    xp = np.concatenate((np.zeros(hw, dtype=np.complex64), xr, np.zeros(hw, dtype=np.complex64)))
    y = np.zeros(x.shape[0], dtype=np.complex64)
    for kk, v in enumerate(np.asarray(h, dtype=np.float32)):
        k = kk - hw
        y += xp[hw - k:hw - k + x.shape[0]] * v
    assert y.dtype == np.complex64
    return y


def tile_bounds(M, hw):
    """-> [(n0, n1)] of the tiles of the usable span [hw, M - hw)."""
    return [(a, min(a + TILE, M - hw)) for a in range(hw, M - hw, TILE)]


def timing_rows(y, hw, Ws):
    """-> (tiles, 3) float64: Re, Im of sum |y[n]|^2 e^{-2 pi i (n Ws mod 2^64) 2^-64} and sum |y[n]|^2 per tile, |y|^2 from the float32 y."""
    y = np.asarray(y).astype(np.complex64)
    re, im = y.real.astype(np.float64), y.imag.astype(np.float64)
    p = re * re + im * im
    out = []
    for a, b in tile_bounds(y.shape[0], hw):
        e = np.exp(-2j * np.pi * turns(np.arange(a, b), Ws))
        T = np.sum(p[a:b] * e)
        out.append((T.real, T.imag, np.sum(p[a:b])))
    return np.array(out, dtype=np.float64)


def unwrap(a, period):
    out = [float(v) for v in a]
    for b in range(1, len(out)):
        out[b] += round((out[b - 1] - out[b]) / period) * period
    return np.array(out, dtype=np.float64)


def fit(rows, M, hw, Ws):
    """The timing fit from a clip's (tiles, 3) rows -> dict: psi, a, c, sps, timing, T0, STEP, i_first, i_last, n_symbols."""
    rows = np.asarray(rows, dtype=np.float64)
    T = rows[:, 0] + 1j * rows[:, 1]
    psi = unwrap(np.angle(T), 2.0 * np.pi)
    centre = np.array([(a + b - 1) / 2.0 for a, b in tile_bounds(M, hw)])
    w = np.abs(T)
    if len(T) >= 3 and w.sum() > 0:
        W = w.sum()
        xm, ym = (w * centre).sum() / W, (w * psi).sum() / W
        sxx = (w * (centre - xm) * (centre - xm)).sum()
        a = float((w * (centre - xm) * (psi - ym)).sum() / sxx) if sxx > 0 else 0.0
        c = float(ym - a * xm)
    else:
        a, c = 0.0, float(np.angle(T.sum()))
    sps = 1.0 / (math.ldexp(float(Ws), -64) + a / (2.0 * np.pi))
    tau = (-c / (2.0 * np.pi)) % 1.0
    STEP, T0 = int(round(sps * 2.0 ** 32)), int(round(tau * sps * 2.0 ** 32))
    idx = [i for i in range(0, int(M / sps) + 3) if hw + 1 <= ((T0 + i * STEP) >> 32) <= M - hw - 3]
    return {"psi": psi, "a": a, "c": c, "sps": sps, "timing": tau, "T0": T0, "STEP": STEP, "i_first": idx[0], "i_last": idx[-1], "n_symbols": len(idx)}


def positions(T0, STEP, i_first, n):
    """-> (k int64, mu float64 with 24 bits) of the symbols i_first .. i_first + n - 1."""
    t = [T0 + (i_first + i) * STEP for i in range(n)]
    k = np.array([v >> 32 for v in t], dtype=np.int64)
    mu = np.array([((v & 0xffffffff) >> 8) for v in t], dtype=np.float64) * 2.0 ** -24
    return k, mu


def _lagrange(mu):
    return (-mu * (mu - 1) * (mu - 2) / 6, (mu + 1) * (mu - 1) * (mu - 2) / 2, -(mu + 1) * mu * (mu - 2) / 2, (mu + 1) * mu * (mu - 1) / 6)


def symbols64(y, T0, STEP, i_first, n):
    """-> s (n,) complex128: the 4-point cubic Lagrange interpolation of the float32 y[k - 1 .. k + 2] at mu, in float64."""
    y = np.asarray(y).astype(np.complex64).astype(np.complex128)
    k, mu = positions(T0, STEP, i_first, n)
    assert k.min() >= 1 and k.max() <= y.shape[0] - 3
    c = _lagrange(mu)
    return c[0] * y[k - 1] + c[1] * y[k] + c[2] * y[k + 1] + c[3] * y[k + 2]


def symbols32(y, T0, STEP, i_first, n):
    """Stage 5 in float32 -> complex64."""
    y = np.asarray(y).astype(np.complex64)
    k, mu = positions(T0, STEP, i_first, n)
    mu = mu.astype(np.float32)
    assert (mu.astype(np.float64) == positions(T0, STEP, i_first, n)[1]).all()             # 24 bits: exact in float32
    one, two = np.float32(1), np.float32(2)
    c = (-mu * (mu - one) * (mu - two) / np.float32(6), (mu + one) * (mu - one) * (mu - two) / two, -(mu + one) * mu * (mu - two) / two,
         (mu + one) * mu * (mu - one) / np.float32(6))
    s = c[0] * y[k - 1] + c[1] * y[k] + c[2] * y[k + 1] + c[3] * y[k + 2]
    assert s.dtype == np.complex64
    return s


def blocks(n, block):
    """-> [(j0, j1)] of the blocks of ``block`` symbols, the last ragged."""
    return [(a, min(a + block, n)) for a in range(0, n, block)]


def z_rows(s, order, block):
    """-> (blocks, 3) float64: Re, Im of sum s^order (negated at order 4) and sum |s|^2, from the float32 s."""
    s = np.asarray(s).astype(np.complex64).astype(np.complex128)
    out = []
    for a, b in blocks(s.shape[0], block):
        z = np.sum(s[a:b] ** order) * (-1.0 if order == 4 else 1.0)
        out.append((z.real, z.imag, np.sum(np.abs(s[a:b]) ** 2)))
    return np.array(out, dtype=np.float64)


def phase_track(rows, order):
    """-> theta (blocks,): arg(z) / order, unwrapped sequentially modulo 2 pi / order."""
    rows = np.asarray(rows, dtype=np.float64)
    return unwrap(np.angle(rows[:, 0] + 1j * rows[:, 1]) / order, 2.0 * np.pi / order)


def centres(n, block):
    return np.array([(a + b - 1) / 2.0 for a, b in blocks(n, block)])


def point(d, order):
    """The unit constellation point a decision names."""
    d = np.asarray(d).astype(np.int64)
    if order == 2:
        return (1.0 - 2.0 * d).astype(np.complex128)
    return ((1.0 - 2.0 * (d >> 1)) + 1j * (1.0 - 2.0 * (d & 1))) / math.sqrt(2.0)


def decide(s, theta, order, block):
    """Stage 7 in float64 on the float32 s -> (r complex128, d uint8, margin): phi by np.interp over the block centres, r = s e^{-i phi}, the
    decisions, and the distance of r from the nearest decision boundary."""
    s = np.asarray(s).astype(np.complex64).astype(np.complex128)
    phi = np.interp(np.arange(s.shape[0], dtype=np.float64), centres(s.shape[0], block), theta)
    r = s * np.exp(-1j * phi)
    if order == 2:
        return r, (r.real < 0).astype(np.uint8), np.abs(r.real)
    return r, (2 * (r.real < 0) + (r.imag < 0)).astype(np.uint8), np.minimum(np.abs(r.real), np.abs(r.imag))


def decide32(s, theta, order, block):
    """Stage 7 in float32: phi in float64, w rounded to complex64, r = s conj(w) in float32 -> (r complex64, d uint8)."""
    s = np.asarray(s).astype(np.complex64)
    phi = np.interp(np.arange(s.shape[0], dtype=np.float64), centres(s.shape[0], block), theta)
    w = np.exp(1j * phi).astype(np.complex64)
    r = s * np.conj(w)
    assert r.dtype == np.complex64
    return r, ((r.real < 0).astype(np.uint8) if order == 2 else (2 * (r.real < 0) + (r.imag < 0)).astype(np.uint8))


def block_rows(r, d, order, block):
    """-> (blocks, 3) float64: sum |r|^2, sum Re(r conj(point(d))), n per block, from the float32 r."""
    r = np.asarray(r).astype(np.complex64).astype(np.complex128)
    p = point(d, order)
    return np.array([(np.sum(np.abs(r[a:b]) ** 2), np.sum((r[a:b] * np.conj(p[a:b])).real), b - a) for a, b in blocks(r.shape[0], block)], dtype=np.float64)


def columns(rows, theta, n, block, rate_fit, carrier0):
    """The host columns from the (blocks, 3) decision rows and theta."""
    rows = np.asarray(rows, dtype=np.float64)
    cnt = rows[:, 2].sum()
    A = rows[:, 1].sum() / cnt
    evm = math.sqrt(max(rows[:, 0].sum() / cnt - A * A, 0.0)) / A
    c = centres(n, block)
    slope = float(np.sum((c - c.mean()) * (theta - theta.mean())) / np.sum((c - c.mean()) ** 2)) if len(c) >= 2 else 0.0
    return {"n_symbols": int(cnt), "gain": A, "evm": evm, "mer_db": -20.0 * math.log10(evm), "carrier_fit": carrier0 + slope * rate_fit / (2.0 * np.pi)}


def demodulate(x, fs, rate, offset, order, fc=0.0, beta=0.35, span=8, block=32):
    """The whole reference for one valid clip, with the float32 roundings of y and s that the device stores -> dict."""
    p = plan(len(x), fs, rate, offset, order, span)
    assert p["valid"], p
    h = taps(p["sps"], p["hw"], beta)
    y = filter64(x, p["Wc"], h).astype(np.complex64)
    trows = timing_rows(y, p["hw"], p["Ws"])
    f = fit(trows, len(x), p["hw"], p["Ws"])
    s = symbols64(y, f["T0"], f["STEP"], f["i_first"], f["n_symbols"]).astype(np.complex64)
    zr = z_rows(s, order, block)
    theta = phase_track(zr, order)
    r, d, margin = decide(s, theta, order, block)
    out = dict(p, taps=h, y=y, timing_rows=trows, s=s, z_rows=zr, theta=theta, r=r, d=d, margin=margin)
    out.update(f)
    out.update(columns(block_rows(r, d, order, block), theta, len(s), block, fs / f["sps"], fc + offset), symbol_rate_fit=fs / f["sps"])
    return out


# ---------------------------------------------------------------------------------------------------------------- generator
def clip(kind, M, seed, sps=7.3, offset=0.0, snr_db=15.0, beta=0.35, span=8):
    """A seeded clip of ``M`` complex64 samples as ``tests/_characterize_ref.clip`` makes them -> (x, a, u0): ``a`` the transmitted unit symbols
    and ``u0`` the timing phase: sample ``n`` is taken at ``u = n / sps + u0`` symbol periods, where symbol ``m`` (``a[m + span]``) peaks at ``u = m``.
    "cw" / "noise": ``a`` and ``u0`` are None."""
    g = np.random.default_rng(seed)
    t = np.arange(M, dtype=np.float64)
    if kind == "noise":
        return ((g.standard_normal(M) + 1j * g.standard_normal(M)) * math.sqrt(0.5)).astype(np.complex64), None, None
    a, u0 = None, None
    if kind == "cw":
        s = np.ones(M, dtype=np.complex128)
    else:
        n_sym = int(M / sps) + 2 * span + 2
        a = (2.0 * g.integers(0, 2, n_sym) - 1.0).astype(np.complex128) if kind == "bpsk" else \
            ((2.0 * g.integers(0, 2, n_sym) - 1.0) + 1j * (2.0 * g.integers(0, 2, n_sym) - 1.0)) * math.sqrt(0.5)
        u0 = g.uniform(0.0, 1.0)
        u = t / sps + u0
        n = np.floor(u).astype(np.int64)[:, None] + np.arange(-span + 1, span + 1)[None, :]
        s = (a[n + span] * rrc(u[:, None] - n, beta)).sum(1)
        s = s / math.sqrt(np.mean(np.abs(s) ** 2))
    s = s * np.exp(2j * np.pi * (offset * t + g.uniform(0.0, 1.0)))
    sigma = math.sqrt(0.5 * 10.0 ** (-snr_db / 10.0))
    return (s + sigma * (g.standard_normal(M) + 1j * g.standard_normal(M))).astype(np.complex64), a, u0


def errors(r, order, k0, sps_true, a, u0, span=8):
    """Symbol errors of the corrected symbols ``r`` (the first taken at ``k0`` samples) against the transmitted ``a``: the smallest count over
    the ``order`` rotations by 2 pi / order and shifts of -1 / 0 / +1 symbols -> (errors, rotation, shift)."""
    r = np.asarray(r).astype(np.complex128)
    m0 = int(round(k0 / sps_true + u0))
    best = None
    for shift in (-1, 0, 1):
        ref = a[m0 + shift + span:m0 + shift + span + r.shape[0]]
        assert ref.shape[0] == r.shape[0]
        for q in range(order):
            v = r * np.exp(2j * np.pi * q / order)
            bad = int(np.sum(np.sign(v.real) != np.sign(ref.real))) if order == 2 else \
                int(np.sum((np.sign(v.real) != np.sign(ref.real)) | (np.sign(v.imag) != np.sign(ref.imag))))
            if best is None or bad < best[0]:
                best = (bad, q, shift)
    return best


# ------------------------------------------------------------------------------------------------------- the shared clips
FS = 1.0e6
SPAN = 16                                                      # the shared call's span: 2 * 16 * 16 + 1 = 513 taps at 16 samples per symbol
BIN = 1.0 / 1024                                               # cycles per sample of one bin of a 1024-point transform
# label, kind, M, D, sps, offset (cycles / sample), snr_db, order handed over, rate error (bins), offset error (bins).  The rates are handed
# over 1/4 bin off and the offsets 1/16 bin off, the characterisation's stated accuracy; the signs keep fs / rate inside [2.5, 16].
CASES = (
    ("order 0", "noise", 777, 1, 4.0, 0.0, 0.0, 0, 0.0, 0.0),                   # an odd length first: every other clip starts at an odd sample
    ("bpsk 3.3", "bpsk", 1500, 1, 3.3, 5.3 / 64, 20.0, 2, 0.25, 1.0 / 16),
    ("qpsk 7.3", "qpsk", 8400, 2, 7.3, -0.03, 20.0, 4, -0.25, -1.0 / 16),
    ("qpsk 2.5", "qpsk", 3000, 1, 2.5, 0.02, 12.0, 4, -0.25, 1.0 / 16),          # a ragged last tile and a ragged last block
    ("bpsk 16", "bpsk", 9000, 1, 16.0, 0.004, 20.0, 2, 0.25, -1.0 / 16),         # 513 taps
    ("too short", "bpsk", 2 * math.ceil(SPAN * 1024 / (1024 / 3.3 + 0.25)) + 300, 1, 3.3, 0.01, 20.0, 2, 0.25, 0.0),
)


def case_clips():
    """-> list of dicts per entry of ``CASES``: x, a, u0, fs, sps (true), rate / offset (Hz, as handed over), order, D, label."""
    out = []
    for i, (label, kind, M, D, sps, off, snr, order, dr, do) in enumerate(CASES):
        fs = FS / D
        x, a, u0 = clip(kind, M, 40 + i, sps, off, snr)
        out.append({"label": label, "x": x, "a": a, "u0": u0, "fs": fs, "D": D, "sps": sps, "rate": (1.0 / sps + dr * BIN) * fs, "offset": (off + do * BIN) * fs,
                    "order": order, "true_rate": fs / sps, "true_offset": off * fs})
    return out
