"""CPU: the float64 reference of the STFT kernels (tests/_stft_ref.py) against a direct O(N^2) DFT, against the oracle
(oracle/stft_ref.py: Hann window, the product shape), its bank against a dense matrix product, the window rule on a hand case,
and the measured base u_ref of the bound that tests/test_stft_kernels_gpu.py holds the kernels to."""
import math

import numpy as np
import pytest
import torch

from tests import _stft_ref as R


def test_power_matches_direct_dft():
    """n_fft = 64, hop 16, asymmetric window, spare samples: every bin of every frame against sum_n x[n] w[n] e^{-2 pi i k n / N}."""
    n_fft, hop, n_frames, B = 64, 16, 5, 2
    L = R.n_samples(n_fft, hop, n_frames) + R.SPARE
    iq = R.tone_in_noise(B, L, n_fft)
    win = R.random_window(n_fft)
    P = R.power(iq, win, n_fft, hop, n_frames)
    assert P.shape == (B, n_frames, n_fft) and P.dtype == np.float64
    n = np.arange(n_fft)
    E = np.exp(-2j * math.pi * np.outer(n, n) / n_fft)                       # [k][n]
    for b in range(B):
        for f in range(n_frames):
            x = iq[b, f * hop: f * hop + n_fft].astype(np.complex128) * win.astype(np.float64)
            X = E @ x
            want = np.abs(X) ** 2
            want = np.concatenate((want[n_fft // 2:], want[:n_fft // 2]))    # shifted bin k <- fft bin (k + N / 2) mod N
            assert np.abs(P[b, f] - want).max() <= 1e-12 * want.max()


def test_reference_matches_oracle_on_synthetic_iq():
    """Hann window, the oracle's bank and shape: dB within the oracle's own f32 rounding (its FFT is complex64), image likewise."""
    from oracle import stft_ref as S
    iq = S.synthetic_iq(1, seed=1)
    win = torch.hann_window(S.N_FFT, periodic=True, dtype=torch.float64).numpy()
    start, wts = R.oracle_bank(S.N_MEL, S.N_FFT)
    s2, w2 = S.mel_table()
    assert np.array_equal(start, s2) and np.array_equal(wts, w2)
    db = R.to_db(R.bank(R.power(iq.numpy(), win, S.N_FFT, S.HOP, S.N_FRAMES), start, wts))      # (1, frames, mel)
    want = S.logmel_db(iq).numpy().transpose(0, 2, 1)
    # the oracle's window is f32 (relative 6e-8 per tap) and its FFT complex64: 1e-3 dB = 2.3e-4 in power covers a filter whose
    # bins lie 30 dB under the frame's peak (2^-24 * 10^1.5 * a few).  The oracle's dB values are f32 of magnitude up to 64
    # (one ulp 3.8e-6): the mean error stays within a few ulps, and the signed mean shows there is no bias
    err = np.abs(db - want)
    assert err.max() <= 1e-3 and err.mean() <= 1e-5 and abs((db - want).mean()) <= 1e-6, (err.max(), err.mean(), (db - want).mean())
    img, mm = R.image(db)
    assert img.shape == (1, 3, S.N_MEL, S.N_FRAMES)
    assert np.abs(img - S.spectrogram_image(iq).numpy()).max() <= 2e-5
    assert img.min() == 0.0 and img.max() == 1.0
    assert np.array_equal(img[:, 0], img[:, 1]) and np.array_equal(img[:, 0], img[:, 2])


@pytest.mark.parametrize("n_fft,taps", [(64, 8), (64, 3), (64, 1), (1024, 8), (1024, 11), (256, 3)])
def test_banks_match_dense_product(n_fft, taps):
    rng = np.random.default_rng(n_fft + taps)
    P = rng.random((2, 3, n_fft))
    # identity: every bin once, the unit weight in every tap slot
    start, wts = R.identity(n_fft, taps)
    assert start.dtype == np.int32 and wts.dtype == np.float32 and wts.shape == (n_fft, taps)
    assert np.array_equal(R.dense(start, wts, n_fft), np.eye(n_fft))
    assert np.array_equal(R.bank(P, start, wts), P)
    assert set((np.arange(n_fft) - start).tolist()) == set(range(taps)) and start.min() == 0
    if n_fft % taps:
        assert start.max() + taps > n_fft, "a filter whose padding taps lie past the last bin"
    # overhang: all weights one, the taps past the end dropped
    start, wts = R.overhang(n_fft, taps)
    assert (wts == 1).all() and wts.shape == (4 + taps - 1, taps)
    if taps > 1:
        assert sorted(start.tolist())[-(taps - 1):] == list(range(n_fft - taps + 1, n_fft))
    M = R.dense(start, wts, n_fft)
    assert np.array_equal(M.sum(1), np.minimum(taps, n_fft - start))
    assert np.abs(R.bank(P, start, wts) - P @ M.T).max() <= 1e-13 * taps
    # a bank with zero weights inside and a NaN behind a zero weight: zero weights are skipped, not multiplied
    start = np.array([0, n_fft - 1, 5], dtype=np.int32)
    wts = np.zeros((3, taps), dtype=np.float32)
    wts[:, 0] = (0.5, 2.0, 0.0)
    Pn = P.copy()
    Pn[..., 5] = np.nan
    got = R.bank(Pn, start, wts)
    assert np.array_equal(got[..., 0], 0.5 * P[..., 0]) and np.array_equal(got[..., 1], 2.0 * P[..., -1]) and (got[..., 2] == 0).all()


def test_oracle_bank_fits_eight_taps_at_the_sizes_the_gpu_tests_use():
    from oracle import stft_ref as S
    for n_fft, n_mel in ((64, 40), (256, 160), (1024, 640), (1024, 600), (2048, 1280)):
        start, wts = R.oracle_bank(n_mel, n_fft)
        assert wts.shape == (n_mel, 8) and np.array_equal(R.dense(start, wts, n_fft), S.mel_matrix(n_mel, n_fft).astype(np.float64))
    start, wts = R.oracle_bank(640, 1024, rows=37)
    assert wts.shape == (37, 8) and start[0] == 0 and start[-1] > 1000


def test_window_rule_hand_case():
    """F = 4 frames of 2 filters, windows of 3 frames at -1, 0, 1, 2, 4, -3."""
    strip = np.array([[1.0, 5.0], [2.0, -3.0], [0.5, 0.0], [9.0, 4.0]])
    img, mm = R.windows(strip, [-1, 0, 1, 2, 4, -3], 3)
    assert img.shape == (6, 3, 2, 3)
    assert mm[:4].tolist() == [[-3.0, 5.0], [-3.0, 5.0], [-3.0, 9.0], [0.0, 9.0]]
    assert mm[4].tolist() == [np.inf, -np.inf] and mm[5].tolist() == [np.inf, -np.inf]
    assert (img[4] == 0).all() and (img[5] == 0).all()
    # window at -1: column 0 is outside (zeros), columns 1, 2 are frames 0, 1
    assert (img[0, :, :, 0] == 0).all()
    assert np.allclose(img[0, 1, :, 1], (np.array([1.0, 5.0]) + 3) / 8) and np.allclose(img[0, 2, :, 2], (np.array([2.0, -3.0]) + 3) / 8)
    # window at 2: frames 2, 3 and one frame past the end
    assert (img[3, :, :, 2] == 0).all() and np.allclose(img[3, 0, :, 1], np.array([9.0, 4.0]) / 9)
    # window at 0 is the plain normalisation
    want, mm0 = R.image(strip[None, :3])
    assert np.array_equal(img[1], want[0]) and mm0[0].tolist() == mm[1].tolist()
    assert np.array_equal(img[:, 0], img[:, 1]) and np.array_equal(img[:, 0], img[:, 2])


def test_min_equals_max_gives_a_zero_image():
    db = np.full((2, 3, 4), -100.0)
    img, mm = R.image(db)
    assert (img == 0).all() and (mm == -100.0).all()


@pytest.mark.parametrize("amp", [1.0, 1e-3], ids=["strong", "weak"])
def test_u_ref_of_the_f32_chain(amp, lo=1.0, hi=64.0):
    """The base of the GPU bound, printed and held to a plausible band.  Storing a dB value in f32 costs up to half an ulp: at
    the frame's peak bin (denominator 2 p) that is u = ln(10) / 10 * ulp(dB) / 2 / 2^-24 / 2 = 1.8 for 16 <= dB < 32 (the weak
    tone), 7.4 for 64 <= dB < 128 (the strong one), and an f32 FFT of 1024 points adds a few units relative to sqrt(p * peak).
    Measured 11.8 / 3.2 here; the GPU tests' inputs give 5.5 - 17.8 / 2.0 - 6.3 over their cases, and the same input up to 1.5 x
    apart on two hosts (the CPU's FFT and log code differ).  Below 1 the chain would be
    better than f32 and the measure blind; above 64 (ten passes of several half-ulps each, all adding up) something is broken."""
    n_fft, hop, n_frames, B = 1024, 256, 3, 2
    L = R.n_samples(n_fft, hop, n_frames) + R.SPARE
    iq, win = R.tone_in_noise(B, L, n_fft, amp=amp), R.random_window(n_fft)
    start, wts = R.identity(n_fft, 8)
    u = R.u_ref(iq, win, n_fft, hop, n_frames, start, wts)
    print(f"[stft-u] cpu f32 chain: n_fft {n_fft} amp {amp:g} u_ref {u:.2f}")
    assert lo <= u <= hi, u
    # the measure sees one wrong twiddle-sized error: bin 100 of frame 0 off by 1e-5 of the peak amplitude
    p = R.exact_p(iq, win, n_fft, hop, n_frames, start, wts)
    bad = p.copy()
    bad[0, 0, 100] = (math.sqrt(p[0, 0, 100]) + 1e-5 * math.sqrt(p[0, 0].max())) ** 2
    assert R.u_measure(bad, p).max() > 4 * u
    assert R.u_measure(p, p).max() == 0.0
