"""Float64 numpy reference of the frequency-keyed demodulation ("FSK demodulation"), written from the definition and independently of
the package: ``plan`` (validity, half width, tiles, Ws / Wc of one clip), ``taps``, ``discriminator``, ``filter64``, ``timing_rows`` (the eight sums per tile of
any filtered clip), ``mean_and_line``, ``fit`` (the timing line and the symbol grid), ``symbols64`` (cubic interpolation), ``level_rows``, ``levels``, ``decide``,
``block_rows``, ``columns``; the float32 emulations ``filter32`` and ``symbols32`` of the y and s sums; ``demodulate`` (the whole chain for one clip, with the
float32 roundings of y, s and r); ``synth`` (a seeded CPFSK / GFSK generator that also returns the bits sent and the timing phase), ``bit_errors`` (against
the bits sent, up to polarity and a shift of one symbol) and ``CASES`` / ``case_clips`` (the clips the CPU and the GPU tests share)."""
import functools
import math

import numpy as np

from tests._demod_ref import blocks, positions, turns, unwrap

TILE = 512                                                     # usable samples per tile (sy11_iq_demod_tile)
TWO64 = 1 << 64
SPS_MIN, SPS_MAX = 2.5, 16.0


def half_width(sps, pulse, span):
    return math.ceil(span * sps) if pulse == "gauss" else math.ceil(sps / 2)


def plan(M, fs, rate, offset, pulse="gauss", bt=0.5, span=2):
    """One clip -> dict: valid, reason, and when valid sps, hw, n_taps, tiles, usable, Ws, Wc (Python ints)."""
    def no(why):
        return {"valid": False, "reason": why}
    if not (math.isfinite(rate) and math.isfinite(offset)) or rate <= 0:
        return no("rate or offset not finite")
    sps = fs / rate
    if not SPS_MIN <= sps <= SPS_MAX:
        return no("samples per symbol outside [2.5, 16]")
    if not abs(offset) < fs / 2:
        return no("offset beyond fs / 2")
    hw = half_width(sps, pulse, span)
    if M < 2 * hw + 1 + TILE:
        return no("too short")
    usable = M - 2 * hw - 1
    return {"valid": True, "reason": "", "sps": sps, "hw": hw, "n_taps": 2 * hw + 1, "usable": usable, "tiles": -(-usable // TILE),
            "Ws": int(math.ldexp(rate / fs, 64)), "Wc": int(math.ldexp(offset / fs, 64)) % TWO64}


def taps(sps, hw, pulse="gauss", bt=0.5):
    """-> (2 hw + 1,) float32: the closed form tap by tap in float64, unit sum, rounded once."""
    h = []
    for k in range(-hw, hw + 1):
        if pulse == "gauss":
            h.append(math.exp(-2.0 * math.pi ** 2 * bt ** 2 * (k / sps) ** 2 / math.log(2.0)))
        else:
            h.append(max(0.0, min(k + 0.5, sps / 2) - max(k - 0.5, -sps / 2)))
    h = np.array(h, dtype=np.float64)
    return (h / h.sum()).astype(np.float32)


def discriminator(x, Wc):
    """-> f (M,) float64, cycles per sample: f[n] = arg(x[n] conj(x[n - 1]) e^{-2 pi i Wc 2^-64}) / 2 pi for n >= 1; f[0] = 0 (never used)."""
    x = np.asarray(x).astype(np.complex64).astype(np.complex128)
    rot = np.exp(-2j * np.pi * turns(np.array([1]), Wc))[0]
    f = np.zeros(x.shape[0], dtype=np.float64)
    f[1:] = np.angle(x[1:] * np.conj(x[:-1]) * rot) / (2.0 * np.pi)
    return f


def tile_bounds(M, hw):
    """-> [(n0, n1)] of the tiles of the usable span [hw + 1, M - hw)."""
    return [(a, min(a + TILE, M - hw)) for a in range(hw + 1, M - hw, TILE)]


def _fir(f, h, dtype):
    """y[n] = sum_k f[n - k] h[k] on hw + 1 <= n < M - hw, zero elsewhere; one sequential sum over the taps in ``dtype``."""
    M, hw = f.shape[0], (len(h) - 1) // 2
    f, h = f.astype(dtype), np.asarray(h).astype(dtype)
    y = np.zeros(M, dtype=dtype)
    lo, hi = hw + 1, M - hw
    for kk in range(2 * hw + 1):
        k = kk - hw
        y[lo:hi] += f[lo - k:hi - k] * h[kk]
    assert y.dtype == dtype
    return y


def filter64(x, Wc, h):
    """-> y (M,) float64."""
    return _fir(discriminator(x, Wc), h, np.float64)


def filter32(x, Wc, h):
    """The y sums in float32: f rounded to float32, float32 products, one sequential float32 sum over the taps -> float32."""
    return _fir(discriminator(x, Wc), h, np.float32)


def timing_rows(y, hw, Ws):
    """-> (tiles, 8) float64 per tile: Re, Im of sum y^2 w; Re, Im of sum y w; Re, Im of sum w; sum y; sum y^2, from the float32 y."""
    y = np.asarray(y).astype(np.float32).astype(np.float64)
    out = []
    for a, b in tile_bounds(y.shape[0], hw):
        w = np.exp(-2j * np.pi * turns(np.arange(a, b), Ws))
        v = y[a:b]
        A, B, Cw = np.sum(v * v * w), np.sum(v * w), np.sum(w)
        out.append((A.real, A.imag, B.real, B.imag, Cw.real, Cw.imag, np.sum(v), np.sum(v * v)))
    return np.array(out, dtype=np.float64)


def row_scales(y, hw):
    """-> (tiles, 8): what an entry of ``timing_rows`` is small or large against: sum y^2, sum |y| and the count of the tile."""
    y = np.asarray(y).astype(np.float64)
    out = []
    for a, b in tile_bounds(y.shape[0], hw):
        p, q, c = np.sum(y[a:b] ** 2), np.sum(np.abs(y[a:b])), float(b - a)
        out.append((p, p, q, q, c, c, q, p))
    return np.array(out, dtype=np.float64)


def mean_and_line(rows, usable):
    rows = np.asarray(rows, dtype=np.float64)
    m = float(rows[:, 6].sum() / usable)
    T = (rows[:, 0] + 1j * rows[:, 1]) - 2.0 * m * (rows[:, 2] + 1j * rows[:, 3]) + m * m * (rows[:, 4] + 1j * rows[:, 5])
    return m, T


def fit(T, M, hw, Ws):
    """The timing fit from a clip's line ``T`` (tiles,) complex -> dict: psi, a, c, sps, timing, T0, STEP, i_first, i_last, n_symbols; the symbols are those
    with hw + 2 <= t_i >> 32 <= M - hw - 4."""
    T = np.asarray(T, dtype=np.complex128)
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
    idx = [i for i in range(0, int(M / sps) + 3) if hw + 2 <= ((T0 + i * STEP) >> 32) <= M - hw - 4]
    return {"psi": psi, "a": a, "c": c, "sps": sps, "timing": tau, "T0": T0, "STEP": STEP, "i_first": idx[0], "i_last": idx[-1], "n_symbols": len(idx)}


def _lagrange(mu):
    return (-mu * (mu - 1) * (mu - 2) / 6, (mu + 1) * (mu - 1) * (mu - 2) / 2, -(mu + 1) * mu * (mu - 2) / 2, (mu + 1) * mu * (mu - 1) / 6)


def symbols64(y, T0, STEP, i_first, n):
    """-> s (n,) float64: the 4-point cubic Lagrange interpolation of the float32 y[k - 1 .. k + 2] at mu."""
    y = np.asarray(y).astype(np.float32).astype(np.float64)
    k, mu = positions(T0, STEP, i_first, n)
    assert k.min() >= 1 and k.max() <= y.shape[0] - 3
    c = _lagrange(mu)
    return c[0] * y[k - 1] + c[1] * y[k] + c[2] * y[k + 1] + c[3] * y[k + 2]


def symbols32(y, T0, STEP, i_first, n):
    """The s sums in float32 -> float32."""
    y = np.asarray(y).astype(np.float32)
    k, mu = positions(T0, STEP, i_first, n)
    mu = mu.astype(np.float32)
    one, two = np.float32(1), np.float32(2)
    c = (-mu * (mu - one) * (mu - two) / np.float32(6), (mu + one) * (mu - one) * (mu - two) / two, -(mu + one) * mu * (mu - two) / two,
         (mu + one) * mu * (mu - one) / np.float32(6))
    s = c[0] * y[k - 1] + c[1] * y[k] + c[2] * y[k + 1] + c[3] * y[k + 2]
    assert s.dtype == np.float32
    return s


def level_rows(s, m, block):
    """-> (blocks, 4) float64: #(s >= m), sum s over s >= m, sum s over s < m, sum s^2, from the float32 s."""
    s = np.asarray(s).astype(np.float32).astype(np.float64)
    out = []
    for a, b in blocks(s.shape[0], block):
        v = s[a:b]
        hi = v >= m
        out.append((float(hi.sum()), v[hi].sum(), v[~hi].sum(), np.sum(v * v)))
    return np.array(out, dtype=np.float64)


def levels(rows, n):
    """-> dict: n_hi, n_lo, one_tone, and c_hi, c_lo, f0, dev unless one tone."""
    rows = np.asarray(rows, dtype=np.float64)
    n_hi = int(round(rows[:, 0].sum()))
    n_lo = n - n_hi
    if n_hi == 0 or n_lo == 0:
        return {"n_hi": n_hi, "n_lo": n_lo, "one_tone": True}
    c_hi, c_lo = rows[:, 1].sum() / n_hi, rows[:, 2].sum() / n_lo
    return {"n_hi": n_hi, "n_lo": n_lo, "one_tone": False, "c_hi": c_hi, "c_lo": c_lo, "f0": (c_hi + c_lo) / 2.0, "dev": (c_hi - c_lo) / 2.0}


def decide(s, f0, dev):
    """-> (r float64, d uint8) from the float32 s: r = (s - f0) / dev, d = (f32(r) < 0)."""
    r = (np.asarray(s).astype(np.float32).astype(np.float64) - f0) / dev
    return r, (r.astype(np.float32) < 0).astype(np.uint8)


def block_rows(r, block):
    """-> (blocks, 3) float64: sum r^2, sum |r|, n per block, from the float32 r."""
    r = np.asarray(r).astype(np.float32).astype(np.float64)
    return np.array([(np.sum(r[a:b] ** 2), np.sum(np.abs(r[a:b])), b - a) for a, b in blocks(r.shape[0], block)], dtype=np.float64)


def columns(rows, f0, dev, fs, fc, offset, rate_fit):
    rows = np.asarray(rows, dtype=np.float64)
    cnt = rows[:, 2].sum()
    A = rows[:, 1].sum() / cnt
    evm = math.sqrt(max(rows[:, 0].sum() / cnt - A * A, 0.0)) / A
    return {"n_symbols": int(cnt), "gain": A, "evm": evm, "mer_db": -20.0 * math.log10(evm) if evm > 0 else math.inf, "carrier_fit": fc + offset + f0 * fs,
            "deviation": dev * fs, "mod_index": 2.0 * dev * fs / rate_fit}


def demodulate(x, fs, rate, offset, pulse="gauss", bt=0.5, span=2, block=32, fc=0.0):
    """The whole reference for one clip the plan accepts, with the float32 roundings of y, s and r that the device stores -> dict (``valid`` False with
    the reason "one tone" where the levels say so)."""
    p = plan(len(x), fs, rate, offset, pulse, bt, span)
    assert p["valid"], p
    h = taps(p["sps"], p["hw"], pulse, bt)
    f = discriminator(x, p["Wc"])
    y = filter64(x, p["Wc"], h).astype(np.float32)
    trows = timing_rows(y, p["hw"], p["Ws"])
    m, T = mean_and_line(trows, p["usable"])
    ft = fit(T, len(x), p["hw"], p["Ws"])
    s = symbols64(y, ft["T0"], ft["STEP"], ft["i_first"], ft["n_symbols"]).astype(np.float32)
    lrows = level_rows(s, m, block)
    lv = levels(lrows, len(s))
    out = dict(p, taps=h, f=f, y=y, timing_rows=trows, m=m, s=s, level_rows=lrows)
    out.update(ft)
    out.update(lv)
    if lv["one_tone"]:
        out.update(valid=False, reason="one tone")
        return out
    r, d = decide(s, lv["f0"], lv["dev"])
    r32 = r.astype(np.float32)
    out.update(r=r32, d=d, symbol_rate_fit=fs / ft["sps"])
    out.update(columns(block_rows(r32, block), lv["f0"], lv["dev"], fs, fc, offset, fs / ft["sps"]))
    return out


# ---------------------------------------------------------------------------------------------------------------- generator
def lead_symbols(sps):
    """The symbols that ``modulate`` keys before sample 0, so that the shaping filter sees data there too."""
    return math.ceil((math.ceil(4 * sps) + 2) / sps) + 2


def modulate(bits, M, sps, h=0.5, pulse="gauss", bt=0.5, u0=0.0, offset=0.0, phase=0.0):
    """CPFSK / GFSK: bit b is the NRZ level 1 - 2 b (a 1 is the LOWER tone) held for one symbol; sample ``n`` is taken at ``u = n / sps + u0`` symbol
    periods, symbol ``j`` spans ``[j, j + 1)``.  The frequency of sample ``n`` (between n - 1/2 and n + 1/2) is ``h / 2`` cycles per symbol times the mean level
    there, shaped at ``pulse`` "gauss" by the Gaussian of ``bt`` (4 symbols each side, unit sum); the phase is 2 pi times its running sum, plus
    ``offset`` cycles per sample.  -> complex128 (M,), unit envelope."""
    a = 1.0 - 2.0 * np.asarray(bits, dtype=np.float64)
    pad = math.ceil(4 * sps) + 2
    n = np.arange(-pad, M + pad, dtype=np.float64)
    cum = np.concatenate(([0.0], np.cumsum(a)))

    def integral(u):                                                       # of the level from symbol time 0 to u
        u = np.clip(u, 0.0, len(a) - 1e-9)
        j = np.floor(u).astype(np.int64)
        return cum[j] + a[j] * (u - j)
    lead = lead_symbols(sps)
    fr = 0.5 * h * (integral((n + 0.5) / sps + u0 + lead) - integral((n - 0.5) / sps + u0 + lead))
    if pulse == "gauss":
        hw = math.ceil(4 * sps)
        g = taps(sps, hw, "gauss", bt).astype(np.float64)
        fr = np.convolve(fr, g / g.sum(), mode="same")
    fr = fr[pad:pad + M] + offset
    return np.exp(2j * np.pi * (np.cumsum(fr) + phase)), lead


def synth(M, seed, sps, h=0.5, pulse="gauss", bt=0.5, snr_db=None, offset=0.0, p_one=0.5, bits=None, u0=None):
    """A seeded clip of ``M`` complex64 samples (``bits``, when given, replace the random ones from symbol time 0 on) -> (x, bits, u0, lead): bit ``lead + j`` spans the symbol times ``[j, j + 1)`` of ``u = n / sps + u0``.  ``snr_db`` None:
    no noise."""
    g = np.random.default_rng(seed)
    u0 = g.uniform(0.0, 1.0) if u0 is None else u0
    n_sym = int(M / sps) + 2 * (math.ceil(4 + 4 / sps) + 6)
    b = (g.uniform(size=n_sym) < p_one).astype(np.uint8)
    if bits is not None:                                                   # the first of them starts at symbol time 0
        b[lead_symbols(sps):lead_symbols(sps) + len(bits)] = bits
    x, lead = modulate(b, M, sps, h, pulse, bt, u0, offset, g.uniform(0.0, 1.0))
    if snr_db is not None:
        sigma = math.sqrt(0.5 * 10.0 ** (-snr_db / 10.0))
        x = x + sigma * (g.standard_normal(M) + 1j * g.standard_normal(M))
    return x.astype(np.complex64), b, u0, lead


def bit_errors(d, k0, sps_true, bits, u0, lead):
    """Bit errors of the decisions ``d`` (the first taken at ``k0`` samples) against the bits sent: the smallest count over both polarities and shifts of
    -1 / 0 / +1 symbols -> (errors, inverted, shift).  The discriminator looks half a sample back, a symbol is decided at its centre."""
    d = np.asarray(d).astype(np.int64)
    j0 = int(round((k0 - 0.5) / sps_true + u0 - 0.5)) + lead
    best = None
    for shift in (-1, 0, 1):
        ref = np.asarray(bits[j0 + shift:j0 + shift + d.shape[0]]).astype(np.int64)
        assert ref.shape[0] == d.shape[0]
        for inv in (0, 1):
            bad = int(np.sum((d ^ inv) != ref))
            if best is None or bad < best[0]:
                best = (bad, inv, shift)
    return best


# ------------------------------------------------------------------------------------------------------- the shared clips
FS = 1.0e6
BLOCK = 32
# label, M, sps (true), h, pulse, bt, span, snr_db, offset (cycles / sample, true), offset handed over (cycles / sample), rate error handed over (ppm), p_one,
# kind ("fsk", "tone": a constant tone at fs / 4, "short" / "sps": refused by the plan)
CASES = (
    ("too short", 2 * 8 + 1 + TILE - 2, 4.0, 0.5, "gauss", 0.5, 2, None, 0.0, 0.0, 0.0, 0.5, "short"),       # an odd length first: the next clip starts odd
    ("rect 4, one tile", 2 * 2 + 1 + TILE, 4.0, 1.0, "rect", 0.5, 2, None, 0.0, 0.0, 0.0, 0.5, "fsk"),
    ("rect 4, a tile of one", 2 * 2 + 1 + TILE + 1, 4.0, 1.0, "rect", 0.5, 2, None, 0.0, 0.0, 0.0, 0.5, "fsk"),
    ("gmsk 8.37", 2300, 8.37, 0.5, "gauss", 0.3, 2, None, 0.02, 0.0195, 200.0, 0.5, "fsk"),
    ("gauss 16, 513 taps", 513 + 2 * TILE + 100, 16.0, 0.7, "gauss", 0.5, 16, None, 0.0, 0.0, 0.0, 0.5, "fsk"),
    ("rect 2.5", 1500, 2.5, 1.0, "rect", 0.5, 2, None, -0.01, 0.0, 0.0, 0.5, "fsk"),
    ("unbalanced", 3000, 5.0, 1.0, "rect", 0.5, 2, None, 0.01, 0.0, 0.0, 0.8, "fsk"),             # a full-response pulse: both levels are reached, see the CPU test
    ("noisy", 2500, 6.2, 0.7, "gauss", 0.5, 2, 18.0, -0.005, 0.0, 0.0, 0.5, "fsk"),
    ("constant tone", 1200, 4.0, 0.5, "gauss", 0.5, 2, None, 0.25, 0.0, 0.0, 0.5, "tone"),
    ("sps 20", 2000, 20.0, 0.5, "gauss", 0.5, 2, None, 0.0, 0.0, 0.0, 0.5, "sps"),
)


@functools.lru_cache(maxsize=None)
def case_clips():
    """-> tuple of dicts per entry of ``CASES``: x, bits, u0, lead, fs, sps (true), rate / offset (Hz, as handed over), pulse, bt, span, h, true_offset (Hz),
    label, kind.  Computed once; leave it unchanged."""
    out = []
    for i, (label, M, sps, h, pulse, bt, span, snr, off, off_arg, ppm, p_one, kind) in enumerate(CASES):
        if kind == "tone":
            x, bits, u0, lead = (1j ** (np.arange(M) % 4)).astype(np.complex64), None, None, None
        else:
            x, bits, u0, lead = synth(M, 70 + i, sps, h, pulse, bt, snr, off, p_one)
        out.append({"label": label, "x": x, "bits": bits, "u0": u0, "lead": lead, "fs": FS, "sps": sps, "rate": FS / sps * (1.0 + ppm * 1e-6), "offset": off_arg * FS,
                    "pulse": pulse, "bt": bt, "span": span, "h": h, "true_offset": off * FS, "kind": kind})
    return tuple(out)


@functools.lru_cache(maxsize=None)
def case_reference():
    """-> tuple per clip: the reference demodulation of a clip the plan accepts, else None.  Computed once; leave it unchanged."""
    return tuple(demodulate(c["x"], c["fs"], c["rate"], c["offset"], c["pulse"], c["bt"], c["span"], BLOCK, fc=2.4e9) if c["kind"] in ("fsk", "tone") else None
                 for c in case_clips())
