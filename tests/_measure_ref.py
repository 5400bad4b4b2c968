"""Float64 numpy reference of the measurement ("Measurement"), written from the definition and independently of the
package: ``plan`` (frames and bins of a box), ``welch`` (the averaged power spectrum and the per-frame in-box power), ``reduce`` (stage 2 in
the device's sequential orders, from any table of per-group partial sums), ``emulate32`` (stage 1 with float32 window products, a
complex64 FFT and float32 squares and sums) and ``derive`` (the host's columns)."""
import math

import numpy as np


def window(N):
    """-> (w float32 (N,), W2): periodic Hann computed in float64 and rounded once; W2 = sum w^2 in float64, exactly rounded."""
    w = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N, dtype=np.float64) / N)).astype(np.float32)
    return w, math.fsum(float(v) * float(v) for v in w)


def plan(tf, n, fs, fc, N, pad_f=0.25, noise_band=0.8):
    """Frames and bins of every box of ``tf`` (k, 4) -> dict of int64 arrays j_first, J, k_lo, k_hi, s_lo, s_hi, n_in, n_noise and L."""
    tf = np.asarray(tf, dtype=np.float64).reshape(-1, 4)
    H, out = N // 2, {k: [] for k in ("j_first", "J", "k_lo", "k_hi", "s_lo", "s_hi", "n_in", "n_noise")}
    L = math.floor(noise_band * N / 2)
    j_max = (n - N) // H
    for t0, f_lo, t1, f_hi in tf.tolist():
        j_first = math.floor(t0 * fs / H)
        j_last = max(j_first, math.ceil(t1 * fs / H) - 2)
        j_first, j_last = min(max(j_first, 0), j_max), min(max(j_last, 0), j_max)
        k_lo, k_hi = max(math.ceil((f_lo - fc) * N / fs), -H), min(math.floor((f_hi - fc) * N / fs), H - 1)
        if k_lo > k_hi:
            k_lo = k_hi = min(max(math.floor(((f_lo + f_hi) / 2 - fc) * N / fs + 0.5), -H), H - 1)
        g = math.ceil(pad_f * (k_hi - k_lo + 1))
        s_lo, s_hi = max(k_lo - g, -H), min(k_hi + g, H - 1)
        noise = [k for k in range(-L, L) if k < s_lo or k > s_hi]
        for key, v in zip(out, (j_first, j_last - j_first + 1, k_lo, k_hi, s_lo, s_hi, k_hi - k_lo + 1, len(noise))):
            out[key].append(v)
    out = {k: np.array(v, dtype=np.int64) for k, v in out.items()}
    out["L"] = L
    return out


def scale_corr(N, J):
    """The two host constants of the reduction: 1 / (J N W2) and the Wilson-Hilferty median-to-mean ratio 1 / (1 - 1 / (9 J))^3."""
    W2 = window(N)[1]
    d = 1.0 - 1.0 / (9.0 * float(J))
    return 1.0 / (float(J) * float(N) * W2), 1.0 / (d * d * d)


def signed(a):
    """FFT order (bin 0 first) -> signed-bin order (bin -N/2 first), along the last axis."""
    return np.fft.fftshift(a, axes=-1)


def frame_powers(x, N, j_first, J, n0=0):
    """float64 |X_j[k]|^2, (J, N) in FFT order; ``x`` holds the capture's samples from ``n0`` on."""
    w, H = window(N)[0].astype(np.float64), N // 2
    x = np.asarray(x).astype(np.complex128)
    out = np.empty((J, N))
    for i in range(J):
        a = (j_first + i) * H - n0
        assert 0 <= a and a + N <= x.shape[0]
        X = np.fft.fft(x[a:a + N] * w)
        out[i] = X.real ** 2 + X.imag ** 2
    return out


def welch(x, N, j_first, J, k_lo, k_hi, n0=0):
    """-> (P (N,) in signed-bin order, E (J,)): the float64 definition."""
    pw = signed(frame_powers(x, N, j_first, J, n0))
    W2 = window(N)[1]
    H = N // 2
    return pw.sum(0) / (J * N * W2), pw[:, k_lo + H:k_hi + H + 1].sum(1) / (N * W2)


def emulate32(x, N, j_first, J, k_lo, k_hi, G, n0=0):
    """Stage 1 in float32 -> (partials (groups, N) float32 in FFT order, E (J,) float32): float32 window products, ``np.fft.fft`` on
    complex64, float32 squares, per group one sequential float32 sum over its frames."""
    w, W2 = window(N)
    H = N // 2
    x = np.asarray(x).astype(np.complex64)
    groups = (j_first + J - 1) // G - j_first // G + 1
    part = np.zeros((groups, N), dtype=np.float32)
    E = np.empty(J, dtype=np.float32)
    for i in range(J):
        j = j_first + i
        a = j * H - n0
        X = np.fft.fft(x[a:a + N] * w)
        assert X.dtype == np.complex64
        pw = X.real * X.real + X.imag * X.imag
        assert pw.dtype == np.float32
        part[j // G - j_first // G] += pw
        E[i] = signed(pw)[k_lo + H:k_hi + H + 1].sum(dtype=np.float32) / np.float32(N * W2)
    return part, E


def reduce(partial, N, J, k_lo, k_hi, s_lo, s_hi, L, beta=0.99):
    """Stage 2 for one box, in the device's orders: ``partial`` (groups, N) in FFT order (the kernel's float32 table), groups ascending -> dict with P (N,)
    float64 in signed-bin order, p_in, noise_median, sum_c, sum_kc (float64) and k_dn, k_up, n_in, n_noise (int)."""
    H = N // 2
    scale, corr = scale_corr(N, J)
    s = np.zeros(N, dtype=np.float64)
    for row in np.asarray(partial).reshape(-1, N):         # ascending g, one after the other
        s = s + row.astype(np.float64)
    P = signed(s * scale)
    noise = np.array([P[k + H] for k in range(-L, L) if k < s_lo or k > s_hi], dtype=np.float64)
    med = float(np.median(noise)) if noise.size else float("nan")
    nd = med * corr
    p_in = 0.0
    for k in range(k_lo, k_hi + 1):
        p_in = p_in + float(P[k + H])
    c = P[s_lo + H:s_hi + H + 1].copy() if math.isnan(nd) else np.maximum(P[s_lo + H:s_hi + H + 1] - nd, 0.0)
    sum_c = sum_kc = 0.0
    for k, v in zip(range(s_lo, s_hi + 1), c.tolist()):
        sum_c = sum_c + v
        sum_kc = sum_kc + float(k) * v
    thr_lo, thr_hi = (1.0 - beta) / 2.0 * sum_c, (1.0 + beta) / 2.0 * sum_c
    k_dn = k_up = None
    run = 0.0
    for k, v in zip(range(s_lo, s_hi + 1), c.tolist()):
        run = run + v
        if k_dn is None and run >= thr_lo:
            k_dn = k
        if k_up is None and run >= thr_hi:
            k_up = k
    return {"P": P, "p_in": p_in, "noise_median": med, "sum_c": sum_c, "sum_kc": sum_kc, "k_dn": s_hi if k_dn is None else k_dn,
            "k_up": s_hi if k_up is None else k_up, "n_in": k_hi - k_lo + 1, "n_noise": int(noise.size)}


def derive(r, N, J, fs, fc):
    """The host's columns from ``reduce``'s dict."""
    nd = r["noise_median"] * scale_corr(N, J)[1]
    floor = r["n_in"] * nd
    with np.errstate(divide="ignore", invalid="ignore"):
        snr = float(10.0 * np.log10(np.float64(max(r["p_in"] - floor, 0.0)) / np.float64(floor))) if not math.isnan(nd) else float("nan")
        centroid = float(fc + np.float64(r["sum_kc"]) / np.float64(r["sum_c"]) * fs / N)
    return {"power": r["p_in"], "noise_density": nd * N / fs, "snr_db": snr, "bandwidth": (r["k_up"] - r["k_dn"] + 1) * fs / N,
            "centroid": centroid, "f_lo_meas": fc + (r["k_dn"] - 0.5) * fs / N, "f_hi_meas": fc + (r["k_up"] + 0.5) * fs / N}


def measure(x, tf, fs, fc, N, pad_f=0.25, beta=0.99, noise_band=0.8):
    """The whole float64 reference for every box -> list of dicts (plan entries, ``reduce``'s and ``derive``'s keys, and E).  The float64
    spectrum stands in for the partial table."""
    p = plan(tf, len(x), fs, fc, N, pad_f, noise_band)
    out = []
    for i in range(len(p["J"])):
        jf, J, k_lo, k_hi = int(p["j_first"][i]), int(p["J"][i]), int(p["k_lo"][i]), int(p["k_hi"][i])
        P, E = welch(x, N, jf, J, k_lo, k_hi)
        r = reduce64(P, N, J, k_lo, k_hi, int(p["s_lo"][i]), int(p["s_hi"][i]), p["L"], beta)
        r.update(derive(r, N, J, fs, fc), E=E, J=J)
        out.append(r)
    return out


def reduce64(P, N, J, k_lo, k_hi, s_lo, s_hi, L, beta=0.99):
    """``reduce`` from a float64 spectrum ``P`` (signed-bin order) that is already scaled: for the CPU checks of the definition."""
    scale = scale_corr(N, J)[0]
    return reduce(np.fft.ifftshift(P) / scale, N, J, k_lo, k_hi, s_lo, s_hi, L, beta)
