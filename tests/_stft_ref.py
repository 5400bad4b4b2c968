"""Float64 reference of the STFT stage (csrc/stft.hip) for tests/test_stft_ref_cpu.py and tests/test_stft_kernels_gpu.py: the
per-bin power spectrum under ANY window, the gather-form filter bank with the kernels' rule, dB, min / max, the normalised
image, the windows cut from a dB strip, bank builders, test signals, and the error measure with its measured bound.
Not a test module.  Arrays are numpy; everything is frame-major like the kernels' output: (B, n_frames, bins or filters).

The error measure.  For a kernel's dB value the power it stands for is  p^ = 10^(dB / 10)  (float64); with the exact
p = P + 1e-10 the quantity bounded is

    u = |p^ - p| / (2^-24 * (p + sqrt(p * max_k p)))              max_k over the frame

The first term of the denominator pays for the log and the f32 store of the dB value (both relative to p), the second for the
rounding of an f32 FFT, whose error in the AMPLITUDE of a bin scales with the frame's peak amplitude and not with the bin's own
(|X^|^2 - |X|^2 ~ 2 |X| e, e ~ 2^-24 sqrt(max p)).  The bound is not a constant: `f32_db` is the same chain in complex64 / f32
on the CPU (torch.fft.fft, f32 bank sum, f32 log10), `u_ref` is its worst u on the very same inputs, and a kernel has to stay
within FACTOR * u_ref.  FACTOR = 4 pays for sincospif twiddles multiplied up (w2 = w1^2, w3 = w1 w2), fused multiply-adds and
the wave kernel's `__log2f`.
"""
import math

import numpy as np
import torch

LOG_EPS = 1e-10
HALF_ULP = 2.0 ** -24
FACTOR = 4.0
SPARE = 37                    # samples per batch row beyond what the frames use: a row stride is not the used length


def n_samples(n_fft, hop, n_frames):
    return n_fft + (n_frames - 1) * hop


def frames_of(iq, n_fft, hop, n_frames):
    """(B, L) -> (B, n_frames, n_fft): frame f of row b is iq[b, f * hop : f * hop + n_fft] (a copy)."""
    iq = np.asarray(iq)
    assert iq.ndim == 2 and n_samples(n_fft, hop, n_frames) <= iq.shape[1]
    idx = np.arange(n_frames)[:, None] * hop + np.arange(n_fft)[None, :]
    return iq[:, idx]


def power(iq, window, n_fft, hop, n_frames):
    """fftshift-ed |X|^2 per bin, float64 (B, n_frames, n_fft): X = FFT(frame * window) in complex128, any window."""
    x = frames_of(iq, n_fft, hop, n_frames).astype(np.complex128) * np.asarray(window, dtype=np.float64)
    X = np.fft.fftshift(np.fft.fft(x, axis=-1), axes=-1)
    return X.real ** 2 + X.imag ** 2


def bank(P, start, wts):
    """Gather-form bank with the kernels' rule: out[..., j] = sum_t wts[j, t] * P[..., start[j] + t] over the taps whose bin
    start[j] + t exists (< n_fft) and whose weight is not zero.  float64."""
    P = np.asarray(P, dtype=np.float64)
    start, wts = np.asarray(start, dtype=np.int64), np.asarray(wts, dtype=np.float64)
    n_fft = P.shape[-1]
    assert wts.ndim == 2 and start.shape == (wts.shape[0],) and (start >= 0).all() and (start < n_fft).all()
    out = np.zeros(P.shape[:-1] + (wts.shape[0],), dtype=np.float64)
    for t in range(wts.shape[1]):
        k = start + t
        use = (k < n_fft) & (wts[:, t] != 0)
        out[..., use] += wts[use, t] * P[..., k[use]]
    return out


def to_db(p):
    return 10.0 * np.log10(np.asarray(p, dtype=np.float64) + LOG_EPS)


def from_db(db):
    """The power (+ 1e-10) a dB value stands for, float64."""
    return 10.0 ** (np.asarray(db, dtype=np.float64) / 10.0)


def minmax(db):
    """(B, n_frames, n_mel) -> (B, 2): per-image [min, max]."""
    db = np.asarray(db)
    return np.stack((db.min(axis=(1, 2)), db.max(axis=(1, 2))), axis=1)


def normalise(db, mm):
    """(B, n_frames, n_mel) dB and (B, 2) [min, max] -> (B, 3, n_mel, n_frames) float64: (db - min) / max(max - min, 1e-12)."""
    db, mm = np.asarray(db, dtype=np.float64), np.asarray(mm, dtype=np.float64)
    lo, hi = mm[:, 0, None, None], mm[:, 1, None, None]
    img = (db - lo) / np.maximum(hi - lo, 1e-12)
    return np.repeat(img.transpose(0, 2, 1)[:, None], 3, axis=1)


def image(db):
    mm = minmax(db)
    return normalise(db, mm), mm


def windows(db_strip, start, n_frames):
    """Windows of n_frames frames cut from a (F, n_mel) dB strip at the frames `start` -> (img (W, 3, n_mel, n_frames) float64,
    minmax (W, 2)).  A frame outside [0, F) reads as nothing: its pixels are 0 and it enters neither min nor max; a window
    wholly outside has minmax (+inf, -inf) and a zero image."""
    strip = np.asarray(db_strip, dtype=np.float64)
    F, n_mel = strip.shape
    start = np.asarray(start, dtype=np.int64).reshape(-1)
    img = np.zeros((start.size, 3, n_mel, n_frames), dtype=np.float64)
    mm = np.empty((start.size, 2), dtype=np.float64)
    for w, s in enumerate(start):
        fr = s + np.arange(n_frames)
        inside = (fr >= 0) & (fr < F)
        if not inside.any():
            mm[w] = (np.inf, -np.inf)
            continue
        rows = strip[fr[inside]]                                   # (frames inside, n_mel)
        lo, hi = rows.min(), rows.max()
        mm[w] = (lo, hi)
        img[w, :, :, inside] = ((rows - lo) / max(hi - lo, 1e-12))[:, None, :]
    return img, mm


# ---------------------------------------------------------------------------------------------------------------- banks
def identity(n_fft, taps):
    """n_mel = n_fft, filter j is bin j alone: one unit weight at tap j % taps, start = j - j % taps (>= 0).  The unit weight
    visits every tap slot and, for tap counts that do not divide n_fft, a start reaches n_fft - 1."""
    j = np.arange(n_fft)
    start = np.maximum(j - j % taps, 0).astype(np.int32)
    wts = np.zeros((n_fft, taps), dtype=np.float32)
    wts[j, j - start] = 1.0
    return start, wts


def overhang(n_fft, taps):
    """All-ones filters: one at every start in the last taps - 1 bins (their taps past bin n_fft - 1 do not exist and must be
    dropped), and four that fit: at bin 0, across the middle (where the fftshift wraps the kernels' index), the last that fits
    whole, and bin n_fft / 2 - 1."""
    fit = [0, n_fft // 2 - taps // 2, n_fft - taps, n_fft // 2 - 1]
    start = np.array(fit + list(range(n_fft - taps + 1, n_fft)), dtype=np.int32)
    return start, np.ones((start.size, taps), dtype=np.float32)


def oracle_bank(n_mel, n_fft, rows=None):
    """oracle/stft_ref.mel_table (8 taps, zero padded).  rows: keep that many of its filters, evenly spread (a bank of fewer than
    n_fft / 14 triangles of the oracle's own would need more than 8 taps)."""
    from oracle import stft_ref as S
    start, wts = S.mel_table(n_mel, n_fft)
    if rows is not None:
        keep = np.round(np.linspace(0, n_mel - 1, rows)).astype(np.int64)
        start, wts = start[keep], wts[keep]
    return np.ascontiguousarray(start), np.ascontiguousarray(wts)


def dense(start, wts, n_fft):
    """The bank as a dense (n_mel, n_fft) float64 matrix, built entry by entry (the CPU test's cross-check of `bank`)."""
    M = np.zeros((len(start), n_fft), dtype=np.float64)
    for j in range(len(start)):
        for t in range(wts.shape[1]):
            k = int(start[j]) + t
            if k < n_fft and wts[j, t] != 0:
                M[j, k] += float(wts[j, t])
    return M


# -------------------------------------------------------------------------------------------------------------- signals
def random_window(n_fft, seed=5):
    """An asymmetric window: uniform [0.25, 1.25), f32.  (A tap paired with the wrong sample changes every bin.)"""
    return (np.random.default_rng(seed).random(n_fft) + 0.25).astype(np.float32)


def tone_in_noise(B, L, n_fft, amp=1.0, seed=11):
    """Unit-power complex white noise plus one off-bin tone 30 times above it (another bin per row), times `amp`: complex64."""
    rng = np.random.default_rng(seed)
    noise = (rng.standard_normal((B, L)) + 1j * rng.standard_normal((B, L))) / math.sqrt(2.0)
    n = np.arange(L, dtype=np.float64)
    k = (0.137 + 0.31 * np.arange(B)) * n_fft + 0.37               # bins from DC, never on a bin centre
    tone = 30.0 * np.exp(2j * math.pi * (k[:, None] / n_fft) * n[None, :])
    return (amp * (noise + tone)).astype(np.complex64)


def on_bin_tone(B, L, n_fft):
    """exp(2 pi i k n / n_fft) / n_fft: under a rectangular window every frame's spectrum is 1 at bin k and 0 elsewhere."""
    n = np.arange(L, dtype=np.float64)
    k = np.array([(5 + 3 * b) % n_fft if b % 2 == 0 else n_fft - 7 - b for b in range(B)], dtype=np.float64)
    return (np.exp(2j * math.pi * (k[:, None] * n[None, :] / n_fft)) / n_fft).astype(np.complex64), k.astype(np.int64)


def one_loud_frame(B, L, n_fft, hop, frame, seed=13):
    """Weak noise + tone (1e-5: every dB value below zero) with the samples of one frame 1e7 times stronger."""
    iq = tone_in_noise(B, L, n_fft, amp=1e-5, seed=seed)
    iq[:, frame * hop: frame * hop + n_fft] *= np.float32(1e7)
    return iq


# ----------------------------------------------------------------------------------------------------------- the measure
def u_measure(p_hat, p):
    """u per element; p_hat, p (..., frames, k) float64, the peak taken per frame."""
    p = np.asarray(p, dtype=np.float64)
    peak = p.max(axis=-1, keepdims=True)
    return np.abs(np.asarray(p_hat, dtype=np.float64) - p) / (HALF_ULP * (p + np.sqrt(p * peak)))


def f32_db(iq, window, n_fft, hop, n_frames, start, wts):
    """The chain in complex64 / f32 on the CPU: torch.fft.fft of the windowed frames, fftshift, |X|^2, the bank summed tap by
    tap in f32 with the kernels' rule, 10 * log10(. + 1e-10).  (B, n_frames, n_mel) float32 numpy."""
    x = torch.from_numpy(frames_of(np.asarray(iq, dtype=np.complex64), n_fft, hop, n_frames))
    x = x * torch.from_numpy(np.asarray(window, dtype=np.float32))
    X = torch.fft.fftshift(torch.fft.fft(x, dim=-1), dim=-1)
    P = X.real * X.real + X.imag * X.imag
    st, w = torch.from_numpy(np.asarray(start, dtype=np.int64)), torch.from_numpy(np.asarray(wts, dtype=np.float32))
    acc = torch.zeros(P.shape[:-1] + (w.shape[0],), dtype=torch.float32)
    for t in range(w.shape[1]):
        k = st + t
        use = (k < n_fft) & (w[:, t] != 0)
        acc[..., use] += w[use, t] * P[..., k[use]]
    return (10.0 * torch.log10(acc + torch.tensor(LOG_EPS, dtype=torch.float32))).numpy()


def exact_p(iq, window, n_fft, hop, n_frames, start, wts):
    return bank(power(iq, window, n_fft, hop, n_frames), start, wts) + LOG_EPS


def u_ref(iq, window, n_fft, hop, n_frames, start, wts, p=None):
    """Worst u of the f32 CPU chain on these inputs (the measured bound's base)."""
    if p is None:
        p = exact_p(iq, window, n_fft, hop, n_frames, start, wts)
    return float(u_measure(from_db(f32_db(iq, window, n_fft, hop, n_frames, start, wts)), p).max())
