"""Float64 numpy reference of the equaliser ("Equalisation"), written from the definition and independently of the package: ``target`` (a word's
decisions -> the points as received: gain, rotation), ``regressors`` (the rows u_k, zero outside the clip), ``solve`` (R and z as a matrix product, ``np.linalg.solve``;
the pivots from ``np.linalg.cholesky``), ``mse``, ``fir`` (the apply in the stated order, vectorised over the symbols), ``owners`` (the ownership rule as a plain loop
over the symbols), ``equalize`` (the chain for one clip, with the second pass) and ``channel`` (a symbol stream through complex taps, with seeded noise)."""
import math

import numpy as np

from tests import _frames_ref as F
from tests._demod_ref import point


def forward(c, q, order):
    """The points ``c`` turned FORWARD by q steps of 2 pi / order, exactly."""
    c = np.asarray(c, dtype=np.complex128)
    re, im = c.real, c.imag
    re, im = ((re, im), (-re, -im))[q] if order == 2 else ((re, im), (-im, re), (-re, -im), (im, -re))[q]
    return re + 1j * im


def target(w, order, q, A):
    """t[k] = A point(w[k]) turned forward by q steps."""
    return forward(A * point(w, order), q, order)


def regressors(r, p, Lt, N):
    """U (Lt, N): U[k, j] = r[p + k + D - j], 0 outside the clip; float64 from the float32 symbols."""
    r = np.asarray(r).astype(np.complex64).astype(np.complex128)
    D = (N - 1) // 2
    pad = np.concatenate((np.zeros(N + Lt, dtype=np.complex128), r, np.zeros(N + Lt, dtype=np.complex128)))
    k, j = np.arange(Lt)[:, None], np.arange(N)[None, :]
    return pad[p + k + D - j + N + Lt]


def solve(r, p, t, N, reg):
    """-> dict: w, R (regularised), z, mu = tr R / N before the loading, pivot_min, cond, ok.  A singular R gives the unit impulse and ok False."""
    t = np.asarray(t, dtype=np.complex128)
    U = regressors(r, p, t.shape[0], N)
    R, z = U.conj().T @ U, U.conj().T @ t
    mu = float(np.trace(R).real) / N
    R = R + reg * mu * np.eye(N)
    out = {"R": R, "z": z, "mu": mu, "ok": True}
    with np.errstate(all="ignore"):
        try:
            G = np.linalg.cholesky(R)
            out["pivot_min"] = float((G.diagonal().real ** 2).min() / mu)
            out["w"] = np.linalg.solve(R, z)
            out["cond"] = float(np.linalg.cond(R))
            out["ok"] = bool(np.isfinite(out["w"]).all() and np.isfinite(out["pivot_min"]) and out["pivot_min"] > 0)
        except np.linalg.LinAlgError:
            out["ok"] = False
    if not out["ok"]:
        out["w"] = np.zeros(N, dtype=np.complex128)
        out["w"][(N - 1) // 2] = 1.0
    return out


def fir_f64(r, w, m):
    """sum_j w[j] r[m + D - j] for the symbols ``m`` in float64, j ascending, every product and sum rounded on its own -> (re, im)."""
    r = np.asarray(r).astype(np.complex64)
    N = len(w)
    D = (N - 1) // 2
    m = np.asarray(m, dtype=np.int64)
    pad = N + 1
    a_all = np.concatenate((np.zeros(pad), r.real.astype(np.float64), np.zeros(pad)))
    b_all = np.concatenate((np.zeros(pad), r.imag.astype(np.float64), np.zeros(pad)))
    re, im = np.zeros(m.shape[0]), np.zeros(m.shape[0])
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(N):
            wr, wi = float(np.real(w[j])), float(np.imag(w[j]))
            a, b = a_all[m + D - j + pad], b_all[m + D - j + pad]
            re = re + ((wr * a) - (wi * b))
            im = im + ((wr * b) + (wi * a))
    return re, im


def fir(r, w, m):
    """e[m] = f32 of ``fir_f64``, the planes one by one -> complex64."""
    re, im = fir_f64(r, w, m)
    out = np.empty(re.shape[0], dtype=np.complex64)
    with np.errstate(invalid="ignore", over="ignore"):
        out.real, out.imag = re.astype(np.float32), im.astype(np.float32)
    return out


def mse(r, p, t, L, A, w=None):
    """sum_(k<L) |x[k] - t[k]|^2 / (L A^2), x = r[p + k] or, with taps, w^T u_k in the apply's order."""
    k = np.arange(L)
    if w is None:
        x = np.asarray(r).astype(np.complex64).astype(np.complex128)[p + k]
    else:
        re, im = fir_f64(r, w, p + k)
        x = re + 1j * im
    e = x - np.asarray(t, dtype=np.complex128)[:L]
    return float(np.sum(e.real * e.real + e.imag * e.imag) / (L * (A * A)))


def owners(N, spans):
    """The ownership rule, symbol by symbol.  ``spans``: per frame (p, length, valid) -> the owner of every symbol of a clip of N, -1 without one."""
    out = np.full(N, -1, dtype=np.int64)
    for m in range(N):
        best = None
        for f, (p, n, valid) in enumerate(spans):
            if valid and p <= m < p + n and (best is None or p > spans[best][0]):
                best = f
        out[m] = -1 if best is None else best
    return out


def segments(owner):
    """The owner array as (start, end, owner) runs."""
    out, a = [], 0
    for m in range(1, len(owner) + 1):
        if m == len(owner) or owner[m] != owner[a]:
            out.append((a, m, int(owner[a])))
            a = m
    return out


def apply(r, owner, W):
    """The apply of a clip: owned symbols through their owner's taps ``W[owner]``, the others bit for bit -> complex64."""
    r = np.asarray(r).astype(np.complex64)
    out = r.copy()
    for f in np.unique(owner[owner >= 0]):
        m = np.flatnonzero(owner == f)
        out[m] = fir(r, W[f], m)
    return out


def equalize(r, order, A, frames, N=7, reg=1e-3, refine=0):
    """The chain for one clip.  ``frames``: list of dicts p, w (the word's decisions), q, n_payload.  -> dict: e (complex64), d, owner, and per frame W, ok, n_train,
    mse_before, mse_after, pivot_min, cond."""
    r = np.asarray(r).astype(np.complex64)
    n = len(frames)
    valid = [len(f["w"]) >= 2 * N and math.isfinite(A) and A > 0 for f in frames]
    owner = owners(len(r), [(f["p"], len(f["w"]) + f["n_payload"], v) for f, v in zip(frames, valid)])
    out = {"owner": owner, "W": [None] * n, "ok": list(valid), "n_train": [0] * n, "mse_before": [math.nan] * n, "mse_after": [math.nan] * n, "pivot_min": [math.nan] * n,
           "cond": [math.nan] * n}

    def one_pass(second, d1):
        for k, f in enumerate(frames):
            if not valid[k]:
                continue
            L = len(f["w"])
            t = target(f["w"], order, f["q"], A)
            Lt = min(refine, L + f["n_payload"]) if second and refine > L else L
            if Lt > L:
                t = np.concatenate((t, A * point(d1[f["p"] + L:f["p"] + Lt], order)))
            s = solve(r, f["p"], t, N, reg)
            out["W"][k], out["ok"][k], out["n_train"][k], out["pivot_min"][k], out["cond"][k] = s["w"], s["ok"], Lt, s.get("pivot_min", math.nan), s.get("cond", math.nan)
            out["mse_before"][k], out["mse_after"][k] = mse(r, f["p"], t, L, A), mse(r, f["p"], t, L, A, s["w"])
        e = apply(r, owner, out["W"])
        return e, F.decide(e, order)
    e, d = one_pass(False, None)
    if refine and any(v and refine > len(f["w"]) and f["n_payload"] > 0 for f, v in zip(frames, valid)):
        e, d = one_pass(True, d)
    out["e"], out["d"] = e, d
    return out


def channel(s, taps, snr_db, seed):
    """The symbol stream ``s`` through the symbol-spaced complex ``taps`` (y[m] = sum_j taps[j] s[m - j]), plus seeded noise ``snr_db`` below the FIRST path's power of
    unit-modulus symbols -> complex64."""
    s = np.asarray(s, dtype=np.complex128)
    y = np.convolve(s, np.asarray(taps, dtype=np.complex128))[:s.shape[0]]
    g = np.random.default_rng(seed)
    sigma = math.sqrt(0.5 * 10.0 ** (-snr_db / 10.0))
    return (y + sigma * (g.standard_normal(s.shape[0]) + 1j * g.standard_normal(s.shape[0]))).astype(np.complex64)


def evm(x, d, order, A=1.0):
    """The rms distance of ``x`` from A point(d), relative to A."""
    e = np.asarray(x).astype(np.complex128) - A * point(d, order)
    return float(math.sqrt(np.mean(np.abs(e) ** 2)) / A)


# ------------------------------------------------------------------------------------------------------- the shared clips
# Clips "a" and "b" of tests/_fec_ref.py (four-phase at 2.5, BPSK at 3.3 samples per symbol; two coded frames each) at SNR_DB instead of 2 / 0 dB, their IQ
# through a two-path channel: the direct path plus ECHO, one symbol late rounded to whole samples (2 and 3).  At 12 dB with an echo of 0.5 e^{0.7i} the
# reference decoder already read every frame without a channel error, with and without the equaliser, so nothing could be told apart; at 9 dB with
# 0.7 e^{0.7i} the reference counts 4, 5 (a) and 2, 3 (b) channel errors without it and none with it.
SNR_DB, ECHO, TAPS, REFINE = 9.0, 0.7 * np.exp(0.7j), 7, 256
_CLIPS = {}


def case_clips():
    """-> tuple of the dicts of ``_fec_ref.case_clips()[:2]`` with ``x`` regenerated at SNR_DB and passed through the two-path channel (``delay`` samples).  Computed once."""
    from tests import _fec_ref as R
    if "clips" not in _CLIPS:
        out = []
        for c, (label, order, sps, M, off, snr, seed, at, n_u, pattern) in zip(R.case_clips()[:2], R.CASES[:2]):
            w = F.decisions(c["bits"], order)
            g = np.random.default_rng(1000 + seed)
            embed = {}
            for j in at:                                                    # the same draws as _fec_ref.case_clips: the same messages
                u = g.integers(0, 2, n_u).astype(np.uint8)
                embed[j] = np.concatenate((w, F.decisions(R.frame_bits(u, R.CRCS[R.CRC], R.POLYS, pattern, None, order)[0], order)))
            x, d, u0 = F.clip(order, M, seed, sps, off, SNR_DB, embed, span=R.SPAN)
            assert u0 == c["u0"] and np.array_equal(d, c["d"])
            delay = int(round(sps))
            y = x.astype(np.complex128)
            y[delay:] += ECHO * x.astype(np.complex128)[:-delay]
            out.append(dict(c, x=y.astype(np.complex64), delay=delay, label=f"{label.split(',')[0]}, {SNR_DB:g} dB, echo"))
        _CLIPS["clips"] = tuple(out)
    return _CLIPS["clips"]


def case_reference():
    """-> tuple per clip of (the reference demodulation, the reference search of its float32-rounded r, the reference equalisation of it, the reference decoding
    of every hit without and with the equaliser, the index in the sent stream of the first symbol).  Computed once; leave it unchanged."""
    from tests import _fec_ref as R
    from tests._demod_ref import demodulate
    if "ref" not in _CLIPS:
        out = []
        for c in case_clips():
            ref = demodulate(c["x"], c["fs"], c["rate"], c["offset"], c["order"], span=R.SPAN)
            r = ref["r"].astype(np.complex64)
            found = F.find(r, c["bits"], c["order"], R.THRESHOLD, c["n_need"])
            w = F.decisions(c["bits"], c["order"])
            frames = [dict(p=int(p), w=w, q=int(q), n_payload=int(n)) for p, q, n in zip(found["position"], found["rotation"], found["n_payload"])]
            eq = equalize(r, c["order"], ref["gain"], frames, N=TAPS, refine=REFINE)
            plain, after = R.decode_found(r, found, ref["gain"], c["order"], 32, c), R.decode_found(eq["e"], found, ref["gain"], c["order"], 32, c)
            out.append((ref, found, eq, plain, after, F.stream_index(ref["T0"], ref["STEP"], ref["i_first"], c["sps"], c["u0"], R.SPAN)))
        _CLIPS["ref"] = tuple(out)
    return _CLIPS["ref"]
