"""Float64 numpy reference of the characterisation ("Characterisation"), written from the definition and independently of
the package: ``plan`` (frames, groups and the searched bins of a clip), ``spectra`` (the three averaged spectra), ``moments``, ``partials64`` (the
definition's per-group sums), ``emulate32`` (stage 1 with float32 products, a complex64 FFT and float32 sums), ``reduce`` (stage 2 in the
device's sequential orders, from any table of per-group partial sums), ``derive`` (the host's columns), ``characterize`` (all of it for one
clip) and ``clip`` (a small seeded generator of BPSK / QPSK / CW / noise clips)."""
import math

import numpy as np

G = 16                                                         # frames per group (sy11_iq_cyclo_group)


def window(N):
    """-> (w float32 (N,), W2): periodic Hann computed in float64 and rounded once; W2 = sum w^2 in float64, exactly rounded."""
    w = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N, dtype=np.float64) / N)).astype(np.float32)
    return w, math.fsum(float(v) * float(v) for v in w)


def plan(M, fs, N, min_rate=0.0):
    """One clip of ``M`` samples at ``fs`` -> dict: valid, J (0 when invalid), L (samples the frames cover), groups, k_min."""
    H = N // 2
    valid = M >= N
    J = (M - N) // H + 1 if valid else 0
    return {"valid": valid, "J": J, "L": (J - 1) * H + N if valid else 0, "groups": -(-J // G), "k_min": max(3, math.ceil(min_rate * N / fs))}


def signed(a):
    """FFT order (bin 0 first) -> signed-bin order (bin -N/2 first), along the last axis."""
    return np.fft.fftshift(a, axes=-1)


def transforms(x):
    """-> (3, M) complex128: |x|^2, x^2, x^4 of the float32 samples, in float64."""
    x = np.asarray(x).astype(np.complex64).astype(np.complex128)
    x2 = x * x
    return np.stack(((x.real * x.real + x.imag * x.imag).astype(np.complex128), x2, x2 * x2))


def frame_powers(x, N, J):
    """float64 |FFT(w y_q,j)[k]|^2, (3, J, N) in FFT order."""
    w, H = window(N)[0].astype(np.float64), N // 2
    y = transforms(x)
    out = np.empty((3, J, N))
    for j in range(J):
        Y = np.fft.fft(y[:, j * H:j * H + N] * w, axis=-1)
        out[:, j] = Y.real ** 2 + Y.imag ** 2
    return out


def spectra(x, N):
    """-> P (3, N) in signed-bin order: the float64 definition."""
    J = plan(len(x), 1.0, N)["J"]
    return signed(frame_powers(x, N, J).sum(1)) / (J * N * window(N)[1])


def partials64(x, N):
    """-> (groups, 3, N) float64 in FFT order: the definition's sum over the frames of every group."""
    J = plan(len(x), 1.0, N)["J"]
    pw = frame_powers(x, N, J)
    return np.stack([pw[:, g * G:min(J, g * G + G)].sum(1) for g in range(-(-J // G))])


def moments(x, N):
    """-> (m20 complex, m21, m42): exactly rounded float64 sums over the samples [0, (J - 1) H + N)."""
    L = plan(len(x), 1.0, N)["L"]
    y = transforms(x)[:, :L]
    return (complex(math.fsum(y[1].real.tolist()), math.fsum(y[1].imag.tolist())), math.fsum(y[0].real.tolist()),
            math.fsum((y[0].real ** 2).tolist()))


def emulate32(x, N):
    """Stage 1 in float32 -> (groups, 3, N) float32 in FFT order: complex64 products for y_q, float32 window products, ``np.fft.fft`` on
    complex64, float32 squares, per group one sequential float32 sum over its frames."""
    w, H = window(N)[0], N // 2
    x = np.asarray(x).astype(np.complex64)
    J = plan(len(x), 1.0, N)["J"]
    x2 = x * x
    y = ((x.real * x.real + x.imag * x.imag).astype(np.complex64), x2, x2 * x2)
    part = np.zeros((-(-J // G), 3, N), dtype=np.float32)
    for j in range(J):
        for q in range(3):
            Y = np.fft.fft(y[q][j * H:j * H + N] * w)
            assert Y.dtype == np.complex64
            pw = Y.real * Y.real + Y.imag * Y.imag
            assert pw.dtype == np.float32
            part[j // G, q] += pw
    return part


def reduce(partial, N, J, k_min):
    """Stage 2 for one clip, in the device's orders: ``partial`` (groups, 3, N) in FFT order (the kernel's float32 table), groups ascending ->
    dict with P (3, N) float64 in signed-bin order and, per q, peak / left / right / median (float64), k and n_search (int)."""
    H = N // 2
    scale = 1.0 / (float(J) * float(N) * window(N)[1])
    s = np.zeros((3, N), dtype=np.float64)
    for row in np.asarray(partial).reshape(-1, 3, N):      # ascending g, one after the other
        s = s + row.astype(np.float64)
    P = signed(s * scale)
    out = {"P": P, "peak": [], "left": [], "right": [], "median": [], "k": [], "n_search": []}
    for q in range(3):
        lo, hi = (k_min if q == 0 else -H), H - 1
        k, best = lo, float(P[q, lo + H])
        for c in range(lo + 1, hi + 1):                    # the first maximum in ascending k
            if float(P[q, c + H]) > best:
                k, best = c, float(P[q, c + H])
        for key, v in zip(("peak", "left", "right", "median", "k", "n_search"),
                          (best, float(P[q, (k - 1 + H) % N]), float(P[q, (k + 1 + H) % N]), float(np.median(P[q, lo + H:hi + H + 1])), k, hi - lo + 1)):
            out[key].append(v)
    return out


def derive(r, mom, N, J, fs, fc, line_db=13.0):
    """The host's columns from ``reduce``'s dict and the moments (m20, m21, m42)."""
    f, db = [], []
    for q in range(3):
        a, b, c = r["left"][q], r["peak"][q], r["right"][q]
        delta = 0.0
        if a > 0 and c > 0 and b > 0:
            la, lb, lc = math.log(a), math.log(b), math.log(c)
            den = la - 2.0 * lb + lc
            delta = 0.5 * (la - lc) / den if den != 0 else 0.0
        f.append((r["k"][q] + delta) / N * fs)
        with np.errstate(divide="ignore", invalid="ignore"):
            db.append(float(10.0 * np.log10(np.float64(b) / np.float64(r["median"][q]))))
    L = (J - 1) * (N // 2) + N
    m20, m21, m42 = mom[0] / L, mom[1] / L, mom[2] / L
    order = 2 if db[1] >= line_db else 4 if db[2] >= line_db else 0
    return {"symbol_rate": f[0], "offset2": f[1] / 2.0, "offset4": f[2] / 4.0, "line_db": db, "power": m21,
            "c42": (m42 - (m20.real * m20.real + m20.imag * m20.imag) - 2.0 * (m21 * m21)) / (m21 * m21), "order": order,
            "carrier": fc + f[1] / 2.0 if order == 2 else fc + f[2] / 4.0 if order == 4 else float("nan"), "keyed": db[0] >= line_db}


def characterize(x, fs, fc, N, min_rate=0.0, line_db=13.0, partial=None):
    """The whole reference for one valid clip -> ``derive``'s dict plus ``reduce``'s keys.  Unless a partial table is given, it is the
    definition's: the float64 sum of every group, rounded once to float32."""
    p = plan(len(x), fs, N, min_rate)
    r = reduce(partials64(x, N).astype(np.float32) if partial is None else partial, N, p["J"], p["k_min"])
    r.update(derive(r, moments(x, N), N, p["J"], fs, fc, line_db), J=p["J"])
    return r


# ---------------------------------------------------------------------------------------------------------------- generator
def rrc(t, beta):
    """The root-raised-cosine pulse of roll-off ``beta`` at ``t`` symbol periods."""
    t = np.asarray(t, dtype=np.float64)
    h = np.empty_like(t)
    z, s = np.abs(t) < 1e-9, np.abs(np.abs(t) - 1.0 / (4.0 * beta)) < 1e-9
    o = ~(z | s)
    h[z] = 1.0 - beta + 4.0 * beta / np.pi
    h[s] = beta / np.sqrt(2.0) * ((1.0 + 2.0 / np.pi) * np.sin(np.pi / (4.0 * beta)) + (1.0 - 2.0 / np.pi) * np.cos(np.pi / (4.0 * beta)))
    u = t[o]
    h[o] = (np.sin(np.pi * u * (1.0 - beta)) + 4.0 * beta * u * np.cos(np.pi * u * (1.0 + beta))) / (np.pi * u * (1.0 - (4.0 * beta * u) ** 2))
    return h


def clip(kind, M, seed, sps=7.3, offset=0.0, snr_db=15.0, beta=0.35, span=8):
    """A seeded clip of ``M`` complex64 samples: ``kind`` "bpsk" / "qpsk" (RRC pulses of roll-off ``beta``, ``sps`` samples per symbol, which
    need not be whole), "cw" or "noise"; the signal has unit mean power, is turned by ``offset`` cycles per sample from a random phase and
    gets white Gaussian noise ``snr_db`` below it ("noise": unit-power noise alone)."""
    g = np.random.default_rng(seed)
    t = np.arange(M, dtype=np.float64)
    if kind == "noise":
        return ((g.standard_normal(M) + 1j * g.standard_normal(M)) * math.sqrt(0.5)).astype(np.complex64)
    if kind == "cw":
        s = np.ones(M, dtype=np.complex128)
    else:
        n_sym = int(M / sps) + 2 * span + 2
        a = (2.0 * g.integers(0, 2, n_sym) - 1.0).astype(np.complex128) if kind == "bpsk" else \
            ((2.0 * g.integers(0, 2, n_sym) - 1.0) + 1j * (2.0 * g.integers(0, 2, n_sym) - 1.0)) * math.sqrt(0.5)
        u = t / sps + g.uniform(0.0, 1.0)                       # time in symbols, a random timing phase
        n = np.floor(u).astype(np.int64)[:, None] + np.arange(-span + 1, span + 1)[None, :]
        s = (a[n + span] * rrc(u[:, None] - n, beta)).sum(1)
        s = s / math.sqrt(np.mean(np.abs(s) ** 2))
    s = s * np.exp(2j * np.pi * (offset * t + g.uniform(0.0, 1.0)))
    sigma = math.sqrt(0.5 * 10.0 ** (-snr_db / 10.0))
    return (s + sigma * (g.standard_normal(M) + 1j * g.standard_normal(M))).astype(np.complex64)
