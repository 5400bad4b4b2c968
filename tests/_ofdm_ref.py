"""The float64 numpy reference of the OFDM demodulation ("OFDM demodulation spec"), built on ``np.fft`` and independent of ``sy11.data.demodulate_ofdm``, with the
synthesiser and the clips the CPU and the GPU tests share.  A clip is a dict; ``case_clips()`` builds the cases of the issue once."""
import functools
import math

import numpy as np

FS = 1.0e6                                                                    # every clip's rate; the carrier spacing of a clip is FS / N
CHANNEL = np.array([1.0, 0.0, 0.3j, 0.0, -0.1])


def layout(N, G, half, pilot_k, pilot_c=None):
    """Used carriers +-1 .. +-half; the pilots at ``pilot_k`` with values ``pilot_c`` (default: 1, 1, 1, -1 repeating); the rest is data."""
    pk = np.array(sorted(pilot_k), dtype=np.int64)
    pc = np.array(([1, 1, 1, -1] * len(pk))[:len(pk)] if pilot_c is None else pilot_c, dtype=np.int64)
    used = np.array([k for k in range(-half, half + 1) if k != 0], dtype=np.int64)
    assert np.isin(pk, used).all() and len(set(np.diff(pk))) == 1
    return {"N": N, "G": G, "S": N + G, "a": G // 4, "data": used[~np.isin(used, pk)], "pk": pk, "pc": pc, "d": int(pk[1] - pk[0]), "used": used}


LAYOUT_A = layout(64, 16, 26, (-21, -7, 7, 21))                               # 802.11a


def points(dec, order):
    """Decisions (uint8, as ``Demodulation.decisions`` holds them) -> unit constellation points."""
    dec = np.asarray(dec).astype(np.int64)
    if order == 2:
        return (1.0 - 2.0 * (dec & 1)).astype(np.complex128)
    return ((1.0 - 2.0 * ((dec >> 1) & 1)) + 1j * (1.0 - 2.0 * (dec & 1))) / math.sqrt(2.0)


def synth(lay, order, n_ofdm, lead, tail, eps, snr_db, seed, channel=None, dec=None, over=1, phase=1.1):
    """``n_ofdm`` OFDM symbols of unit power per sample after ``lead`` and before ``tail`` samples without signal, turned by ``eps`` carrier spacings, in complex noise ``snr_db``
    below the signal.  ``dec``: the decisions to send (n_ofdm, n_data), random when None.  ``over``: the oversampling (an ``over * N``-point IFFT and an ``over * G`` prefix;
    lead, tail and the noise are then at that rate too, and the noise is ``snr_db`` below the signal in the band of the clip's rate).  -> (x complex128, dec)."""
    g = np.random.default_rng(seed)
    N, G, nd = lay["N"] * over, lay["G"] * over, lay["data"].shape[0]
    if dec is None:
        dec = g.integers(0, order, (n_ofdm, nd)).astype(np.uint8)
    pts = points(dec, order)
    parts = []
    for m in range(n_ofdm):
        X = np.zeros(N, dtype=np.complex128)
        X[lay["data"] % N], X[lay["pk"] % N] = pts[m], lay["pc"]
        t = np.fft.ifft(X) * N / math.sqrt(lay["used"].shape[0])
        parts.append(np.concatenate((t[-G:], t)))
    s = np.concatenate(parts)
    if channel is not None:
        s = np.convolve(s, channel)[:s.shape[0]]
    x = np.concatenate((np.zeros(lead, dtype=np.complex128), s, np.zeros(tail, dtype=np.complex128)))
    x = x * np.exp(2j * np.pi * eps * np.arange(x.shape[0]) / N + 1j * phase)
    sigma = math.sqrt(over * 10.0 ** (-snr_db / 10.0) / 2.0)
    return x + sigma * (g.standard_normal(x.shape[0]) + 1j * g.standard_normal(x.shape[0])), dec


# ----------------------------------------------------------------------------------------------------------------- the definition
def fold(x, N, G):
    """-> (F (S,) complex128, E (S,), the scales of F and of E: per residue the sum of the terms' magnitudes)."""
    x = np.asarray(x).astype(np.complex128)
    S = N + G
    L = (x.shape[0] - N) // S
    a, b = x[:L * S].reshape(L, S), x[N:N + L * S].reshape(L, S)
    e = 0.5 * (np.abs(a) ** 2 + np.abs(b) ** 2)
    return (b * np.conj(a)).sum(0), e.sum(0), (np.abs(b) * np.abs(a)).sum(0), e.sum(0)


def fit1(F, E, N, G):
    S = F.shape[0]
    idx = (np.arange(S)[:, None] + np.arange(G)[None, :]) % S
    gam, phi = F[idx].sum(1), E[idx].sum(1)
    theta = int(np.argmax(np.abs(gam)))
    return {"theta": theta, "eps": float(np.angle(gam[theta]) / (2.0 * np.pi)), "cp_corr": float(np.abs(gam[theta]) / phi[theta]) if phi[theta] > 0 else 0.0}


def starts(theta, M, lay):
    """The first sample of every FFT window: theta + G - a + m S for every integer m that keeps the window inside the clip."""
    base = theta + lay["G"] - lay["a"]
    return np.array([base + m * lay["S"] for m in range(-2, M // lay["S"] + 2) if base + m * lay["S"] >= 0 and base + m * lay["S"] + lay["N"] <= M], dtype=np.int64)


def word(offset_cycles, eps, N):
    return int(round(math.ldexp(offset_cycles + eps / N, 64))) % (1 << 64)


def spectra(x, st, W, lay):
    """-> (Y (n_ofdm, n_used + n_pil sorted: the data and pilot carriers ascending) complex128, u (n_ofdm, P), power (n_ofdm,), the carriers).  The turn of sample n is the
    exact ``(n W mod 2^64) 2^-64`` of a cycle."""
    x = np.asarray(x).astype(np.complex128)
    N, a = lay["N"], lay["a"]
    turn = np.array([((n * W) % (1 << 64)) / 2.0 ** 64 for n in range(x.shape[0])], dtype=np.float64)
    v = x * np.exp(-2j * np.pi * turn)
    k = np.sort(np.concatenate((lay["data"], lay["pk"])))
    Y = np.array([np.fft.fft(v[s:s + N])[k % N] for s in st]).reshape(len(st), k.shape[0]) * np.exp(2j * np.pi * ((k * a) % N) / N)[None, :]
    u = Y[:, np.searchsorted(k, lay["pk"])] * lay["pc"][None, :]
    return Y, u, (np.abs(Y) ** 2).sum(1), k


def fit2(u, lay):
    c = (u[:, 1:] * np.conj(u[:, :-1])).sum()
    beta = float(np.angle(c)) / lay["d"]
    z = (u * np.exp(-1j * beta * lay["pk"])[None, :]).sum(1)
    mag = np.abs(z)
    active = mag >= 0.5 * mag.max()
    A = float(np.abs(u[active]).mean())
    rho = np.exp(-1j * np.angle(z)) / A if A > 0 else np.zeros(z.shape[0], dtype=np.complex128)
    return {"beta": beta, "z": z, "phi": np.angle(z), "active": active, "A": A, "rho": rho, "tau": np.exp(-1j * beta * lay["data"])}


def decide(Yc, rho, tau, lay, order, k):
    """``Yc`` (n_ofdm, n_used) as stored (complex64) -> (r complex128 before its rounding, r as stored complex64, decisions uint8), each (n_ofdm, n_data)."""
    y = np.asarray(Yc).astype(np.complex128)[:, np.searchsorted(k, lay["data"])]
    r = y * rho[:, None] * tau[None, :]
    r32 = r.astype(np.complex64)
    nr, ni = (r32.real < 0).astype(np.uint8), (r32.imag < 0).astype(np.uint8)
    return r, r32, nr if order == 2 else (2 * nr + ni).astype(np.uint8)


def rows_of(r32, dec, order):
    """(n_ofdm, n_data) stored symbols and decisions -> (n_ofdm, 3) float64: sum |r|^2, sum Re(r conj(point(d))), n_data."""
    r = np.asarray(r32).astype(np.complex128)
    return np.stack(((np.abs(r) ** 2).sum(1), (r * np.conj(points(dec, order))).real.sum(1), np.full(r.shape[0], r.shape[1], dtype=np.float64)), axis=1)


def columns(rows, active):
    rows = rows[active]
    n = rows[:, 2].sum()
    A = rows[:, 1].sum() / n
    with np.errstate(divide="ignore", invalid="ignore"):
        evm = float(np.sqrt(max(rows[:, 0].sum() / n - A * A, 0.0)) / np.float64(A))
        return {"gain": float(A), "evm": evm, "mer_db": float(-20.0 * np.log10(np.float64(evm)))}


def demodulate(x, lay, order, offset_cycles=0.0):
    """The whole definition on one clip (``x`` as stored, complex64) -> dict."""
    N, G = lay["N"], lay["G"]
    F, E, sF, sE = fold(x, N, G)
    f1 = fit1(F, E, N, G)
    st = starts(f1["theta"], len(x), lay)
    W = word(offset_cycles, f1["eps"], N)
    Y, u, power, k = spectra(x, st, W, lay)
    f2 = fit2(u, lay)
    r, r32, dec = decide(Y.astype(np.complex64), f2["rho"], f2["tau"], lay, order, k)
    rows = rows_of(r32, dec, order)
    out = {"F": F, "E": E, "starts": st, "W": W, "Y": Y, "u": u, "power": power, "k": k, "r": r, "r32": r32, "dec": dec, "rows": rows}
    out.update(f1)
    out.update(f2)
    out.update(columns(rows, f2["active"]))
    return out


def sent_symbols(st, c):
    """Which transmitted OFDM symbol every FFT window of ``st`` reads: (index (n_ofdm,), -1 where none; the largest distance in samples of a window from where it was meant to
    sit)."""
    lay = c["lay"]
    j = np.round((st - c["lead"] - lay["G"] + lay["a"]) / lay["S"]).astype(np.int64)
    ok = (j >= 0) & (j < c["n_ofdm"])
    miss = np.abs(st - (c["lead"] + lay["G"] - lay["a"] + j * lay["S"]))[ok].max()
    return np.where(ok, j, -1), int(miss)


def symbol_errors(dec, active, st, c):
    """-> (symbol errors on the active OFDM symbols, whether the active ones are exactly the transmitted ones, |theta - true| in samples)."""
    j, miss = sent_symbols(st, c)
    exact = bool(np.array_equal(active, j >= 0)) and int((j >= 0).sum()) == c["n_ofdm"]
    bad = sum(int((dec[m] != c["dec"][j[m]]).sum()) for m in np.flatnonzero(active & (j >= 0)))
    return bad, exact, miss


# ----------------------------------------------------------------------------------------------------------------- the shared clips
# label, layout, order, OFDM symbols, lead, tail, eps, snr_db, channel, seed
def _cases():
    p128 = tuple(-42 + 12 * i for i in range(8))
    p256 = tuple(-88 + 25 * i for i in range(8))
    p512 = tuple(-180 + 40 * i for i in range(10))
    p1024 = tuple(-275 + 50 * i for i in range(12))
    return (("1: 802.11a qpsk", LAYOUT_A, 4, 12, 37, 150, 0.31, 20.0, None, 11),
            ("2: 802.11a bpsk", LAYOUT_A, 2, 8, 5, 400, -0.42, 12.0, None, 12),
            ("3: 802.11a 37 symbols", LAYOUT_A, 4, 37, 100, 100, 0.1, 20.0, None, 13),
            ("4: N 128", layout(128, 32, 50, p128), 4, 10, 300, 100, 0.2, 20.0, None, 14),
            ("5: N 256, G 18", layout(256, 18, 100, p256), 4, 6, 77, 700, -0.1, 15.0, None, 15),
            ("6: N 512 bpsk", layout(512, 128, 200, p512), 2, 3, 11, 900, 0.25, 20.0, None, 16),
            ("7: N 1024", layout(1024, 72, 300, p1024), 4, 4, 500, 2300, 0.45, 20.0, None, 17),
            ("8: 802.11a multipath", LAYOUT_A, 4, 40, 37, 150, 0.31, 20.0, CHANNEL, 18))


@functools.lru_cache(maxsize=None)
def case_clips():
    """-> tuple of dicts: the eight parity cases (kind "ofdm"), then "short" (one period too few), "rate" (its ``spacing`` is 0.1 % off), "order" (3) and "zero" (20 periods of
    zeros).  Per clip: x (complex64), lay, order, spacing (Hz), kind, label, and for "ofdm": dec (as sent), n_ofdm, lead, eps, snr_db.  Leave them unchanged."""
    out = []
    for label, lay, order, n_ofdm, lead, tail, eps, snr, ch, seed in _cases():
        x, dec = synth(lay, order, n_ofdm, lead, tail, eps, snr, seed, channel=ch)
        out.append({"label": label, "kind": "ofdm", "x": x.astype(np.complex64), "lay": lay, "order": order, "spacing": FS / lay["N"], "dec": dec, "n_ofdm": n_ofdm, "lead": lead,
                    "eps": eps, "snr_db": snr})
    g = np.random.default_rng(19)
    noise = lambda n: ((g.standard_normal(n) + 1j * g.standard_normal(n)) * 0.1).astype(np.complex64)      # noqa: E731
    A = LAYOUT_A
    for kind, n, order, spacing in (("short", 64 + 2 * 80 - 1, 4, FS / 64), ("rate", 1000, 4, FS / 64 * 1.001), ("order", 1000, 3, FS / 64)):
        out.append({"label": kind, "kind": kind, "x": noise(n), "lay": A, "order": order, "spacing": spacing})
    out.append({"label": "zero", "kind": "zero", "x": np.zeros(64 + 20 * 80, dtype=np.complex64), "lay": A, "order": 4, "spacing": FS / 64})
    return tuple(out)


@functools.lru_cache(maxsize=None)
def case_reference():
    """The reference demodulation of every clip of ``case_clips()`` that has one (None elsewhere).  Computed once; leave it unchanged."""
    return tuple(demodulate(c["x"], c["lay"], c["order"]) if c["kind"] in ("ofdm", "zero") else None for c in case_clips())
