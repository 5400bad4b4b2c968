"""Float64 numpy restatement of the digital down-converter (include/sy11.h, sy11_iq_resample; definition in
sy11/data/resample.py and DESIGN.md §4), with exact integer phase arithmetic, and a float32 emulation of the kernel's sum order.

    y[m] = sum_k h[k] u[m Q + c - k],   u[i P] = x[i] e^{j 2 pi frac(i dphi / 2^32)},   u = 0 elsewhere and outside the capture

Only k = phi + j P, phi = (m Q + c) mod P, meets a sample: y[m] = sum_j h[phi + j P] xm[i0 - j], i0 = floor((m Q + c) / P).
No scipy here (the GPU tests import this module)."""
import numpy as np


def table_of(h, P):
    """Polyphase table (P, T) of the taps ``h`` (any float dtype, kept): entry [phi, j] = h[phi + j P], zero padded."""
    h = np.asarray(h)
    T = -(-h.shape[0] // P)
    pad = np.zeros(P * T, dtype=h.dtype)
    pad[:h.shape[0]] = h
    return np.ascontiguousarray(pad.reshape(T, P).T)


def mixed(x, n0, dphi):
    """x[i] e^{j 2 pi frac(i dphi / 2^32)} in float64 for the absolute samples i = n0 .. n0 + len(x) - 1; the phase is the exact
    integer (i dphi) mod 2^32, taken as a signed fraction of a cycle."""
    x = np.asarray(x).astype(np.complex128)
    if dphi == 0:
        return x
    i = (np.arange(x.shape[0], dtype=np.uint64) + np.uint64(n0 % (1 << 32))) & np.uint64(0xFFFFFFFF)
    ph = ((i * np.uint64(dphi)) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    ph = np.where(ph >= 1 << 31, ph - (1 << 32), ph).astype(np.float64)
    return x * np.exp(2j * np.pi * (ph / 2.0 ** 32))


def _sum(xm, table, P, Q, c, n0, m0, M, real):
    """sum_j table[phi, j] xm[i0 - j] for m = m0 .. m0 + M - 1, j ascending, in the dtype ``real`` (every product and every sum
    rounded on its own); xm = the mixed samples [n0, n0 + len(xm)), zero outside."""
    cplx = np.complex128 if real == np.float64 else np.complex64
    table = np.asarray(table).astype(real)
    T = table.shape[1]
    q = [(m0 + k) * Q + c for k in range(M)]                               # Python ints: exact for any m0
    phi = np.array([v % P for v in q], dtype=np.int64)
    rel = np.array([v // P - n0 for v in q], dtype=np.int64)               # index of xm[i0] in the array
    xm = np.asarray(xm).astype(cplx)
    re, im = np.zeros(M, dtype=real), np.zeros(M, dtype=real)
    for j in range(T):
        idx = rel - j
        ok = (idx >= 0) & (idx < xm.shape[0])
        v = np.where(ok, xm[np.clip(idx, 0, xm.shape[0] - 1)], 0).astype(cplx)
        w = table[phi, j]
        re = (re + (w * v.real).astype(real)).astype(real)
        im = (im + (w * v.imag).astype(real)).astype(real)
    return re + 1j * im


def ddc_ref(x, table, P, Q, c, dphi=0, n0=0, m0=0, M=None):
    """Float64 outputs [m0, m0 + M) of the capture whose samples [n0, n0 + len(x)) are ``x`` and that is zero elsewhere.  P == Q: the
    pure mixer y[m] = xm[m].  ``M`` None: every output of a capture that is exactly ``x`` (n0 = m0 = 0)."""
    n = len(x)
    if M is None:
        M = n if P == Q else (n - 1) * P // Q + 1
    xm = mixed(x, n0, dphi)
    if P == Q:
        return xm[m0 - n0:m0 - n0 + M]
    return _sum(xm, table, P, Q, c, n0, m0, M, np.float64)


def ddc_f32(x, table, P, Q, c, dphi=0, n0=0, m0=0, M=None):
    """The kernel's arithmetic in numpy: mixed samples (float64, exact phase) rounded to float32, float32 taps, one sequential
    float32 sum per output in ascending tap order, every product and sum rounded (no fma)."""
    n = len(x)
    if M is None:
        M = n if P == Q else (n - 1) * P // Q + 1
    xm = mixed(x, n0, dphi).astype(np.complex64)
    if P == Q:
        return xm[m0 - n0:m0 - n0 + M]
    return _sum(xm, np.asarray(table, dtype=np.float32), P, Q, c, n0, m0, M, np.float32)


def plan_ref(x, plan, n0=0, m0=0, M=None, f32=False):
    """``ddc_ref`` / ``ddc_f32`` with everything taken from a ``ResamplePlan`` (its float32 table, as the kernel reads it)."""
    return (ddc_f32 if f32 else ddc_ref)(x, plan.taps, plan.P, plan.Q, plan.c, plan.dphi, n0, m0, M)
