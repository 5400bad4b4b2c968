"""Float64 numpy restatement of the polyphase analysis filter bank (include/sy11.h, sy11_iq_channelize; definition in
sy11/data/channelize.py and DESIGN.md §4) and a float32 emulation of the kernel's arithmetic.

    y_k[m] = sum_{r < K} e^{-j 2 pi k r / K} v_m[r],     v_m[r] = sum_{i = r (mod K)} h[m D + c - i] x[i],   x = 0 outside the capture

``i`` is the absolute sample index.  No scipy here (the GPU tests import this module)."""
import numpy as np


def _fold(x, h, K, D, c, n0, m0, M, real):
    """v (M, K) in the dtype ``real``: for every (m, r) ONE sequential sum over the taps n = n_first + j K in ascending order
    (n_first = (m D + c - r) mod K), every product and every sum rounded on its own.  x = the samples [n0, n0 + len(x))."""
    cplx = np.complex128 if real == np.float64 else np.complex64
    h = np.asarray(h).astype(real)
    x = np.asarray(x).astype(cplx)
    N = h.shape[0]
    A = np.array([(m0 + t) * D + c for t in range(M)], dtype=object)               # Python ints: exact for any m0
    a_mod = np.array([int(v % K) for v in A], dtype=np.int64)[:, None]             # (M, 1)
    a_rel = np.array([int(v - n0) for v in A], dtype=np.int64)[:, None]            # index of x[A] in the array
    r = np.arange(K, dtype=np.int64)[None, :]
    n_first = (a_mod - r) % K                                                      # (M, K)
    re, im = np.zeros((M, K), dtype=real), np.zeros((M, K), dtype=real)
    for j in range((N - 1) // K + 1):
        n = n_first + j * K
        ok_n = n < N
        idx = a_rel - n
        ok = ok_n & (idx >= 0) & (idx < x.shape[0])
        v = np.where(ok, x[np.clip(idx, 0, x.shape[0] - 1)], 0).astype(cplx)
        w = np.where(ok_n, h[np.minimum(n, N - 1)], 0).astype(real)
        re = (re + (w * v.real).astype(real)).astype(real)
        im = (im + (w * v.imag).astype(real)).astype(real)
    return re, im


def pfb_ref(x, h, K, D, c, n0=0, m0=0, M=None):
    """Float64 outputs (K, M): the time steps [m0, m0 + M) of every channel of the capture whose samples [n0, n0 + len(x)) are
    ``x`` and that is zero elsewhere.  ``M`` None: every time step of a capture that is exactly ``x`` (n0 = m0 = 0)."""
    if M is None:
        M = (len(x) - 1) // D + 1
    re, im = _fold(x, h, K, D, c, n0, m0, M, np.float64)
    return np.ascontiguousarray(np.fft.fft(re + 1j * im, axis=1).T)


def twiddles(K):
    """The kernel's table: e^{-j 2 pi t / K}, t < K / 2, in float64, rounded once to complex64."""
    return np.exp(-2j * np.pi * np.arange(max(K // 2, 1), dtype=np.float64) / K).astype(np.complex64)


def pfb_f32(x, h, K, D, c, n0=0, m0=0, M=None, twiddle=None):
    """The kernel's arithmetic in numpy: float32 taps and samples, the sequential float32 fold in ascending tap order, then the
    kernel's FFT schedule in float32 with the same twiddle table — radix-2 decimation in frequency, half = K/2, K/4, .., 1; in
    every group of 2 half positions the lower one takes a + b and the upper one (a - b) w with w = twiddle[(p mod half) K /
    (2 half)]; position p then holds channel bitrev(p).  Every product and every sum is rounded on its own (no fma)."""
    if M is None:
        M = (len(x) - 1) // D + 1
    f = np.float32
    w = twiddles(K) if twiddle is None else np.asarray(twiddle, dtype=np.complex64)
    wr, wi = w.real.astype(f), w.imag.astype(f)
    re, im = _fold(np.asarray(x, dtype=np.complex64), np.asarray(h, dtype=f), K, D, c, n0, m0, M, f)
    p = np.arange(K)
    half, sh = K >> 1, 0
    while half >= 1:
        up = (p & half) != 0
        lo_i, up_i = p[~up], p[up]                                                 # pairs: lo_i[q] <-> up_i[q] = lo_i[q] + half
        ar, ai, br, bi = re[:, lo_i], im[:, lo_i], re[:, up_i], im[:, up_i]
        t = (lo_i & (half - 1)) << sh
        dr, di = (ar - br).astype(f), (ai - bi).astype(f)
        nr = ((dr * wr[t]).astype(f) - (di * wi[t]).astype(f)).astype(f)
        ni = ((dr * wi[t]).astype(f) + (di * wr[t]).astype(f)).astype(f)
        re[:, lo_i], im[:, lo_i] = (ar + br).astype(f), (ai + bi).astype(f)
        re[:, up_i], im[:, up_i] = nr, ni
        half >>= 1
        sh += 1
    bits = K.bit_length() - 1
    rev = np.array([int(format(q, f"0{bits}b")[::-1], 2) for q in range(K)])
    out = np.empty((K, M), dtype=np.complex64)
    out[rev] = (re + 1j * im).T.astype(np.complex64)
    return out


def plan_ref(x, plan, n0=0, m0=0, M=None, f32=False):
    """``pfb_ref`` / ``pfb_f32`` with everything taken from a ``ChannelPlan`` (its float32 taps and twiddles, as the kernel reads them)."""
    if f32:
        return pfb_f32(x, plan.taps, plan.K, plan.D, plan.c, n0, m0, M, plan.twiddle)
    return pfb_ref(x, plan.taps, plan.K, plan.D, plan.c, n0, m0, M)
