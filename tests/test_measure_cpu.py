"""CPU: the host side of the measurement (sy11/data/measure.py) — frame and bin planning on hand cases, every argument error, the chunk
planner — and the float64 reference of tests/_measure_ref.py on constructed signals, where the answer is known from the definition."""
import math

import numpy as np
import pytest

from tests import _measure_ref as R

FS, N_CAP = 1.0e6, 40000


def _plan(tf, n=N_CAP, fs=FS, fc=0.0, **kw):
    from sy11.data.measure import plan_measure
    return plan_measure(np.asarray(tf, dtype=np.float64).reshape(-1, 4), n, fs, fc, **kw)


def _same_as_reference(p, tf, n, fs, fc, N, **kw):
    r = R.plan(tf, n, fs, fc, N, **kw)
    for key in ("j_first", "J", "k_lo", "k_hi", "s_lo", "s_hi", "n_noise"):
        assert getattr(p, key).tolist() == r[key].tolist(), key
    assert p.noise_l == r["L"]


# ------------------------------------------------------------------------------------------------------------- planning
def test_frames_and_bins_on_hand_cases():
    N, H = 256, 128                                             # bins of 3906.25 Hz, j_max = (40000 - 256) // 128 = 310
    tf = [(-0.001, 1.0e5, 0.002, 2.0e5),                        # 0 starts before sample 0: floor(-1000 / 128) = -8 -> 0; ceil(2000 / 128) - 2 = 14
          (0.030, 1.0e5, 0.040, 2.0e5),                         # 1 ends on the last sample: ceil(40000 / 128) - 2 = 311 -> 310; first = 234
          (0.010, 1.0e5, 0.01005, 2.0e5),                       # 2 shorter than a frame: first = 78, ceil(10050 / 128) - 2 = 77 -> J = 1
          (0.010, 100100.0, 0.020, 100300.0),                   # 3 narrower than a bin: ceil(25.63) = 26 > floor(25.68) = 25 -> nearest 26
          (0.010, -5.0e5, 0.020, 5.0e5)]                        # 4 the whole band: [-128, 127], no noise bins
    p = _plan(tf, n_fft=N)
    assert p.j_first.tolist() == [0, 234, 78, 78, 78] and p.J.tolist() == [15, 77, 1, 78, 78]
    assert p.k_lo.tolist() == [26, 26, 26, 26, -128] and p.k_hi.tolist() == [51, 51, 51, 26, 127]
    assert p.s_lo.tolist() == [19, 19, 19, 25, -128] and p.s_hi.tolist() == [58, 58, 58, 27, 127]          # g = ceil(0.25 * 26) = 7, ceil(0.25) = 1
    assert p.noise_l == 102 and p.n_noise.tolist() == [164, 164, 164, 201, 0]
    _same_as_reference(p, tf, N_CAP, FS, 0.0, N)
    G = p.G
    assert p.groups.tolist() == [(jf + J - 1) // G - jf // G + 1 for jf, J in zip(p.j_first.tolist(), p.J.tolist())]
    assert p.offset.tolist() == [0, 15, 92, 93, 171, 249]
    # the whole-band box has no noise bins: the reference's median is NaN, and so are noise and SNR; c falls back to P
    r = R.reduce(np.ones((1, N)), N, 78, -128, 127, -128, 127, p.noise_l)
    d = R.derive(r, N, 78, FS, 0.0)
    assert r["n_noise"] == 0 and math.isnan(r["noise_median"]) and math.isnan(d["snr_db"]) and math.isnan(d["noise_density"])
    assert r["sum_c"] > 0 and math.isfinite(d["centroid"]) and d["bandwidth"] > 0


def test_frames_three_billion_samples_into_a_capture():
    n = 3 * 10 ** 9 + 50000
    p = _plan([(3.0e9 / FS, 1.0e5, 3.0e9 / FS + 0.01, 2.0e5)], n=n, n_fft=256)
    assert p.j_first.tolist() == [3 * 10 ** 9 // 128] and p.J.tolist() == [math.ceil((3.0e9 + 10000) / 128) - 2 - 3 * 10 ** 9 // 128 + 1]
    it, _ = p.items()
    assert it["j0"].dtype == np.int64 and int(it["j0"][0]) * 128 == 3 * 10 ** 9 and int(it["nf"].sum()) == int(p.J[0])
    _same_as_reference(p, p.tf, n, FS, 0.0, 256)


def test_centre_frequency_moves_the_bins_not_the_frames():
    fc = 2.4e9
    tf = np.array([(0.001, fc - 3.0e5, 0.004, fc - 2.0e5), (0.0, fc + 4.9e5, 0.04, fc + 5.0e5)])
    for N in (64, 1024):
        p = _plan(tf, fc=fc, n_fft=N, pad_f=0.5, noise_band=0.5)
        _same_as_reference(p, tf, N_CAP, FS, fc, N, pad_f=0.5, noise_band=0.5)
        assert (p.s_hi <= N // 2 - 1).all() and (p.s_lo >= -N // 2).all() and p.k_hi[1] == N // 2 - 1


def test_every_argument_error_is_a_value_error_before_the_device():
    from sy11.data.measure import min_chunk, plan_measure_chunks
    ok = [(0.001, 1.0e5, 0.002, 2.0e5)]
    for kw in (dict(fs=0.0), dict(fs=float("nan")), dict(fc=float("inf")), dict(n=255, n_fft=256), dict(n=0), dict(n_fft=48), dict(n_fft=2048),
               dict(n_fft=True), dict(n_fft=1024.0), dict(pad_f=-0.1), dict(pad_f=float("nan")), dict(beta=0.0), dict(beta=1.1),
               dict(beta=float("nan")), dict(noise_band=0.0), dict(noise_band=1.5), dict(rows=[0.5]), dict(rows=[1]), dict(rows=[-1]),
               dict(max_frames=1)):
        with pytest.raises(ValueError, match="plan_measure"):
            _plan(ok, **kw)
    for bad in ((float("nan"), 1.0e5, 0.002, 2.0e5), (0.002, 1.0e5, 0.001, 2.0e5), (0.001, 2.0e5, 0.002, 1.0e5), (0.001, 6.0e5, 0.002, 7.0e5)):
        with pytest.raises(ValueError, match="plan_measure"):
            _plan([bad])
    p = _plan(ok, n_fft=256)
    assert min_chunk(256) == (p.G - 1) * 128 + 256
    with pytest.raises(ValueError, match="chunk_samples"):
        plan_measure_chunks(p, min_chunk(256) - 1)
    assert len(_plan(ok, rows=[])) == 0 and plan_measure_chunks(_plan(ok, rows=[]), 1 << 20) == []


# ------------------------------------------------------------------------------------------------------------- chunks
@pytest.mark.parametrize("chunk", ["smallest", 1 << 24])
def test_every_item_sits_whole_in_exactly_one_chunk(chunk):
    from sy11.data.measure import min_chunk, plan_measure_chunks
    N, n = 256, 1 << 20
    g = np.random.default_rng(5)
    t0 = g.uniform(-0.01, n / FS, 200)
    f0 = g.uniform(-4.5e5, 4.0e5, 200)
    tf = np.stack((t0, f0, t0 + g.uniform(0, 0.05, 200), f0 + g.uniform(0, 5.0e4, 200)), 1)
    p = _plan(tf, n=n, n_fft=N)
    chunk_samples = min_chunk(N) if chunk == "smallest" else chunk
    chunks = plan_measure_chunks(p, chunk_samples)
    assert (len(chunks) > 20) if chunk == "smallest" else (len(chunks) == 1)
    it_all, box = p.items()
    assert it_all["row"].tolist() == list(range(p.total_rows)) and int(it_all["nf"].sum()) == p.total_frames
    assert (it_all["j0"] // p.G == (it_all["j0"] + it_all["nf"] - 1) // p.G).all() and (it_all["nf"] >= 1).all()
    seen = np.zeros(p.total_rows, dtype=np.int64)
    frames = np.zeros(p.total_frames, dtype=np.int64)
    for ch in chunks:
        assert 0 <= ch.a < ch.b <= n and ch.b - ch.a <= chunk_samples
        assert all(ch.a <= lo < hi <= ch.b for lo, hi in ch.reads) and all(r[1] < s[0] for r, s in zip(ch.reads, ch.reads[1:]))
        for it in ch.items:
            lo, hi = int(it["j0"]) * (N // 2), (int(it["j0"]) + int(it["nf"]) - 1) * (N // 2) + N
            assert any(r[0] <= lo and hi <= r[1] for r in ch.reads)
            seen[int(it["row"])] += 1
            frames[int(it["env_off"]):int(it["env_off"]) + int(it["nf"])] += 1
    assert (seen == 1).all() and (frames == 1).all()


# ------------------------------------------------------------------------------------------------------------- the reference
def test_tone_on_a_bin_centre_has_power_a_squared_within_the_hann_leakage():
    """x = A e^{2 pi i k0 n / N}: |x|^2 = A^2, so sum_k P[k] = A^2 by Parseval whatever the window.  The exact periodic Hann puts
    X[k0] = A N / 2, X[k0 +- 1] = -A N / 4 and nothing elsewhere, W2 = 3 N / 8, so P[k0] = 2/3 A^2 and P[k0 +- 1] = A^2 / 6: a box
    holding k0 alone misses exactly A^2 / 3.  The window is rounded to f32 (|dw| <= 2^-25), which leaks |X[k]| <= A N 2^-25 into every
    other bin: at most N (A N 2^-25)^2 / (N W2) = (8 / 3) N 2^-50 A^2 outside a box that holds k0 - 1 .. k0 + 1."""
    N, A, k0 = 256, 0.37, 40
    n = 20 * N
    x = A * np.exp(2j * np.pi * k0 * np.arange(n) / N)
    bw = FS / N
    wide, one = R.measure(x, [(0.0, (k0 - 1.2) * bw, n / FS, (k0 + 1.2) * bw), (0.0, (k0 - 0.2) * bw, n / FS, (k0 + 0.2) * bw)], FS, 0.0, N)
    assert (wide["n_in"], one["n_in"]) == (3, 1) and wide["J"] == 2 * 20 - 1
    bound = (8.0 / 3.0) * N * 2.0 ** -50 + 1e-12
    assert abs(wide["power"] - A * A) <= bound * A * A, (wide["power"], A * A)
    assert abs(one["power"] - 2.0 / 3.0 * A * A) <= (bound + 2.0 ** -23) * A * A          # 2/3 itself moves with the rounded window
    assert abs(wide["centroid"] - k0 * bw) <= 1e-6 * bw and wide["snr_db"] > 100
    assert np.allclose(wide["E"], A * A, rtol=1e-9) and len(wide["E"]) == wide["J"]


def test_white_noise_density_within_three_of_the_references_own_standard_deviations():
    """noise_density fs estimates sigma^2.  The bar is 3 x the standard deviation of the reference's own estimate over 32 seeds at the same
    (N, J); it holds for a further seed and, divided by sqrt(32), for the mean of the 32 (the Wilson-Hilferty correction leaves a bias of
    about 1.004 at J = 64)."""
    N, J, sigma2 = 64, 64, 0.25
    n = (J - 1) * (N // 2) + N
    tf = [(0.0, 1.0e5, n / FS, 1.5e5)]

    def estimate(seed):
        g = np.random.default_rng(seed)
        x = (g.standard_normal(n) + 1j * g.standard_normal(n)) * math.sqrt(sigma2 / 2)
        r = R.measure(x, tf, FS, 0.0, N)[0]
        assert r["J"] == J
        return r["noise_density"] * FS
    est = np.array([estimate(s) for s in range(32)])
    sd = est.std(ddof=1)
    one = estimate(1000)
    print(f"white noise N={N} J={J}: mean {est.mean() / sigma2:.4f} x sigma^2, sd {sd / sigma2:.4f} x sigma^2, seed 1000 {one / sigma2:.4f}")
    assert 0.01 * sigma2 < sd < 0.1 * sigma2
    assert abs(one - sigma2) <= 3 * sd
    assert abs(est.mean() - sigma2) <= 3 * sd / math.sqrt(32) + 0.005 * sigma2


def test_band_limited_emission_measures_as_the_design_quotes():
    """A 100 kHz emission at +150 kHz, 10 dB above the noise inside its band, in a 1 MS/s capture at N = 256 (DESIGN.md quotes 0.00997 for
    a noise of 0.01, 9.97 dB, 105.5 kHz and 148.8 kHz for one draw).  Each figure to its resolution: the noise to 3 %, the SNR to
    0.3 dB, the bandwidth to one bin (3.9 kHz) around 27 bins, the centroid to half a bin around the true 150 kHz."""
    N, n = 256, 1 << 17
    g = np.random.default_rng(11)
    noise = (g.standard_normal(n) + 1j * g.standard_normal(n)) * math.sqrt(0.01 / 2)
    spec = np.fft.fft(g.standard_normal(n) + 1j * g.standard_normal(n))
    f = np.fft.fftfreq(n, 1 / FS)
    spec[(f < 1.0e5) | (f > 2.0e5)] = 0
    sig = np.fft.ifft(spec)
    sig *= math.sqrt(0.01 / np.mean(np.abs(sig) ** 2))          # in-band noise power is 0.01 * 0.1 = 0.001: 10 dB
    r = R.measure(noise + sig, [(0.0, 1.0e5, n / FS, 2.0e5)], FS, 0.0, N)[0]
    print(f"band-limited: noise {r['noise_density'] * FS:.5f}, snr {r['snr_db']:.2f} dB, bandwidth {r['bandwidth']:.1f} Hz, centroid {r['centroid']:.1f} Hz")
    assert abs(r["noise_density"] * FS - 0.01) <= 0.03 * 0.01
    assert abs(r["snr_db"] - 10.0) <= 0.3
    assert abs(r["bandwidth"] - 105468.75) <= FS / N
    assert abs(r["centroid"] - 1.5e5) <= FS / N / 2


def test_a_running_sum_that_lands_on_the_threshold_takes_that_bin():
    """c = [v, v, 2 v] sums exactly to v, 2 v, 4 v.  beta = 0.5: the lower threshold 0.25 * 4 v = v is reached AT bin 0, the upper
    0.75 * 4 v = 3 v only at bin 2.  c = [v, v] with beta -> 0: both thresholds equal v and take bin 0; a little above, the upper moves on."""
    N, J = 64, 3
    part = np.zeros((1, N))
    part[0, [5, 6, 7]] = [1.0, 1.0, 2.0]
    r = R.reduce(part, N, J, 5, 7, 5, 7, 0, beta=0.5)                        # L = 0: no noise bins, c = P
    assert r["n_noise"] == 0 and r["sum_c"] == 4 * r["P"][5 + 32] and (r["k_dn"], r["k_up"]) == (5, 7)
    part[0, 7] = 0.0
    assert [(q["k_dn"], q["k_up"]) for q in (R.reduce(part, N, J, 5, 6, 5, 6, 0, beta=0.0), R.reduce(part, N, J, 5, 6, 5, 6, 0, beta=0.01))] \
        == [(5, 5), (5, 6)]
    v = float(r["P"][5 + 32])
    assert R.reduce(part, N, J, 5, 6, 5, 6, 0)["sum_kc"] == 5.0 * v + 6.0 * v          # product and sum rounded one by one
