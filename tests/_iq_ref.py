"""Float64 numpy restatement of the IQ gather / augment kernel (include/sy11.h, sy11_iq_gather_augment) and of the label maps:
a uint32 phase accumulator, its own Philox4x32-10 in uint32 / uint64 arithmetic, Box-Muller on (x + 0.5) 2^-32.  Written from the
specification, not from the kernel; the Philox is pinned to published known answers in tests/test_iq_dataset_cpu.py so that the
kernel and this file cannot be wrong in the same way."""
import math

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: (..., 4) uint32-valued, key: (2,) -> (..., 4) uint32 (as uint64 arrays holding 32-bit values)."""
    c = [np.asarray(counter[..., i], dtype=np.uint64) & MASK for i in range(4)]
    k0, k1 = np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]                  # 32 x 32 -> 64 bits: never overflows uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK, p1 >> np.uint64(32), p1 & MASK
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return np.stack(c, -1)


def noise(seed, n):
    """Unit-variance complex normal samples 0 .. n-1 (complex128): key = seed, counter = (k, 0, 0, 0) gives samples 2k and 2k + 1."""
    k = (n + 1) // 2
    ctr = np.zeros((k, 4), dtype=np.uint64)
    ctr[:, 0] = np.arange(k, dtype=np.uint64)
    x = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)).astype(np.float64)
    u = (x + 0.5) * 2.0 ** -32
    r = np.sqrt(-np.log(u[:, 0::2]))                                          # variance 1/2 per component
    w = r * np.exp(2j * np.pi * u[:, 1::2])
    return w.reshape(-1)[:n]


def rotate(x, dphi, phi0, conj):
    """c(x[n]) * exp(2 pi i ((phi0 + n dphi) mod 2^32) / 2^32) in float64, the phase in exact integer arithmetic."""
    x = np.asarray(x, dtype=np.complex128)
    x = np.conj(x) if conj else x
    n = np.arange(x.shape[0], dtype=np.uint64)
    ph = (np.uint64(phi0) + n * np.uint64(dphi)) & MASK                       # n < 2^31, dphi < 2^32: the product fits uint64
    ph = ph.astype(np.int64)
    ph = np.where(ph > 2 ** 31, ph - 2 ** 32, ph)                             # (-pi, pi]
    return x * np.exp(1j * (ph.astype(np.float64) * (math.pi / 2 ** 31)))


def gather_augment(src, off, L, dphi=0, phi0=0, conj=False, gain=1.0, src2=None, off2=0, dphi2=0, phi02=0, conj2=False, gain2=1.0,
                   sigma=0.0, seed=0):
    out = float(np.float32(gain)) * rotate(src[off:off + L], dphi, phi0, conj)
    if src2 is not None:
        out = out + float(np.float32(gain2)) * rotate(src2[off2:off2 + L], dphi2, phi02, conj2)
    if sigma:
        out = out + float(np.float32(sigma)) * noise(seed, L)
    return out


# ---- label maps (the arithmetic of the producer's warped axis, restated)
def freq_to_row(hz, sample_rate, center_freq, n_fft, n_mel, alpha=1.25):
    b = ((hz - center_freq) / sample_rate + 0.5) * n_fft
    u = b / ((n_fft / 2) * (n_fft - 1) / n_fft) - 1.0
    m = math.copysign(math.log1p(abs(u) * alpha) / math.log1p(alpha), u)
    return (m + 1.0) * (n_mel + 1) / 2.0 - 1.0


def time_to_col(t, sample_rate, n_fft, hop):
    return (t * sample_rate - n_fft / 2) / hop
