"""GPU: the kernels of csrc/stft.hip one by one against the float64 reference of tests/_stft_ref.py.

The shape of a call selects the FFT kernel (sy11_stft_logmel): n_fft 1024 with hop 256, 8 taps and a 16-byte aligned `mel_w` is
the wave-per-frame kernel ("wave"), n_fft 1024 otherwise the Stockham radix-4 kernel ("stockham"), any other n_fft the radix-2
kernel ("radix2"); `_kernel_of` mirrors that and every test names the kernel it means to reach.

Per bin.  Through the identity bank (filter j = bin j, the unit weight in every tap slot) each dB value stands for one bin:
p^ = 10^(dB / 10) against p = P + 1e-10 under the measure u of _stft_ref (relative to p + sqrt(p * frame peak), in units of
2^-24), bounded by 4 * u_ref where u_ref is the worst u of the same chain in complex64 / f32 on the CPU, on the same inputs.
The window is random and asymmetric, rows carry 37 spare samples, signals are a tone 30 x over unit noise at amplitude 1 and
1e-3 and an on-bin tone under a rectangular window (peak 0 dB, every other bin on the -100 dB floor within 1e-3 dB).

Measured worst u per kernel and input class (MI355X) are in DESIGN.md section 5, "STFT kernels, measured".
"""
import functools

import numpy as np
import pytest
import torch

from tests import _stft_ref as R
from tests._kernel_ref import DEV, lib, ops, same_bits

gpu = pytest.mark.gpu
B = 2


def _kernel_of(n_fft, hop, taps, aligned=True):
    if n_fft == 1024:
        return "wave" if hop == 256 and taps == 8 and aligned else "stockham"
    return "radix2"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _logmel(iq, win, start, wts, n_fft, hop, n_frames, mel_w_dev=None):
    """-> (db numpy (B, n_frames, n_mel) f32, minmax numpy (B, 2) f32, the two device tensors)"""
    o = ops()
    w = _dev(wts) if mel_w_dev is None else mel_w_dev
    db, mm = o.stft_logmel(_dev(iq), _dev(np.asarray(win, dtype=np.float32)), _dev(start), w, n_fft, hop, n_frames, len(start))
    torch.cuda.synchronize()
    return db.cpu().numpy(), mm.cpu().numpy(), db, mm


@functools.lru_cache(maxsize=None)
def _signal(kind, n_fft, hop, n_frames):
    """(iq (B, L) complex64, window f32): L has 37 samples more than the frames use."""
    L = R.n_samples(n_fft, hop, n_frames) + R.SPARE
    amp = {"strong": 1.0, "weak": 1e-3, "loud": 100.0, "faint": 1e-5}[kind]
    return R.tone_in_noise(B, L, n_fft, amp=amp, seed=11 + n_fft % 97 + hop % 89), R.random_window(n_fft)


def _check_u(tag, kernel, kind, db, iq, win, n_fft, hop, n_frames, start, wts):
    p = R.exact_p(iq, win, n_fft, hop, n_frames, start, wts)
    u_ref = R.u_ref(iq, win, n_fft, hop, n_frames, start, wts, p=p)
    assert np.isfinite(db).all()
    u = R.u_measure(R.from_db(db), p)
    at = np.unravel_index(int(u.argmax()), u.shape)
    print(f"[stft-u] {kernel} {tag} {kind}: u {u.max():.2f} u_ref {u_ref:.2f} ratio {u.max() / u_ref:.2f} at (b, frame, k) = {tuple(int(i) for i in at)}")
    assert u.max() <= R.FACTOR * u_ref, (kernel, tag, kind, float(u.max()), u_ref, at)


def _check_minmax_exact(db, mm):
    assert np.array_equal(mm[:, 0], db.min(axis=(1, 2))) and np.array_equal(mm[:, 1], db.max(axis=(1, 2))), (mm, db.min(axis=(1, 2)), db.max(axis=(1, 2)))


# ------------------------------------------------------------------------------------------------ 2. per-bin parity
#        kernel      n_fft  hop  taps  n_frames
PER_BIN = [
    ("wave", 1024, 256, 8, 3),            # run 1
    ("wave", 1024, 256, 8, 21),           # run 2: the last wave has one frame, the last workgroup three waves
    ("wave", 1024, 256, 8, 322),          # run 5: the last wave has two frames, the last workgroup one wave
    ("stockham", 1024, 128, 8, 9),
    ("stockham", 1024, 512, 8, 9),
    ("stockham", 1024, 256, 1, 9),        # the general tap loop
    ("stockham", 1024, 256, 3, 9),
    ("stockham", 1024, 256, 11, 9),
    ("stockham", 1024, 128, 8, 260),      # four frames per workgroup, 65 workgroups
    ("stockham", 1024, 256, 3, 262),      # ... with a remainder of two frames
    ("radix2", 64, 16, 8, 5),             # 32 butterflies, 256 threads
    ("radix2", 64, 16, 3, 5),
    ("radix2", 256, 64, 8, 3), ("radix2", 256, 64, 3, 3),
    ("radix2", 2048, 512, 8, 3), ("radix2", 2048, 512, 3, 3),
    ("radix2", 4096, 1024, 8, 3), ("radix2", 4096, 1024, 3, 3),
    ("radix2", 8192, 2048, 8, 2),         # 96 KiB of dynamic LDS
]
per_bin = pytest.mark.parametrize("kernel,n_fft,hop,taps,n_frames", PER_BIN, ids=lambda v: str(v))


@gpu
@pytest.mark.parametrize("kind", ["strong", "weak"])
@per_bin
def test_per_bin_parity(kernel, n_fft, hop, taps, n_frames, kind):
    assert _kernel_of(n_fft, hop, taps) == kernel
    iq, win = _signal(kind, n_fft, hop, n_frames)
    start, wts = R.identity(n_fft, taps)
    db, mm, _, _ = _logmel(iq, win, start, wts, n_fft, hop, n_frames)
    assert db.shape == (B, n_frames, n_fft)
    _check_u(f"identity n_fft {n_fft} hop {hop} taps {taps} frames {n_frames}", kernel, kind, db, iq, win, n_fft, hop, n_frames, start, wts)
    _check_minmax_exact(db, mm)


@gpu
@per_bin
def test_on_bin_tone_leaves_every_other_bin_on_the_floor(kernel, n_fft, hop, taps, n_frames):
    """exp(2 pi i k n / n_fft) / n_fft under a rectangular window: |X_k|^2 = 1, the rest is exactly 0 + 1e-10.  The floor bound
    (1e-3 dB = 2.3e-14 in power = 1.5e-7 in amplitude beside a peak of 1) is met by a correct f32 FFT and by nothing that leaks."""
    assert _kernel_of(n_fft, hop, taps) == kernel
    L = R.n_samples(n_fft, hop, n_frames) + R.SPARE
    iq, k = R.on_bin_tone(B, L, n_fft)
    start, wts = R.identity(n_fft, taps)
    db, mm, _, _ = _logmel(iq, np.ones(n_fft, dtype=np.float32), start, wts, n_fft, hop, n_frames)
    for b in range(B):
        ks = (int(k[b]) + n_fft // 2) % n_fft                                  # the fftshift-ed index of fft bin k
        peak = db[b, :, ks]
        # 12 radix-2 stages of relative 2^-24 each on the amplitude, twice for the power: 1.5e-6 = 6e-6 dB; 1e-4 dB is 16 x that
        assert np.abs(peak).max() <= 1e-4, (kernel, b, peak)
        rest = np.delete(db[b], ks, axis=1)
        worst = np.abs(rest + 100.0).max()
        print(f"[stft-floor] {kernel} n_fft {n_fft} hop {hop} taps {taps} frames {n_frames} row {b}: peak {np.abs(peak).max():.2e} dB, floor off by {worst:.2e} dB")
        assert worst <= 1e-3, (kernel, b, worst)
    _check_minmax_exact(db, mm)


# ------------------------------------------------------------------------------------------------------- 3. banks
BANK_SHAPES = [("wave", 1024, 256, 8, 21), ("stockham", 1024, 128, 8, 9), ("stockham", 1024, 256, 3, 9),
               ("radix2", 256, 64, 8, 3), ("radix2", 256, 64, 3, 3)]


@gpu
@pytest.mark.parametrize("kernel,n_fft,hop,taps,n_frames", BANK_SHAPES, ids=lambda v: str(v))
def test_overhang_bank_drops_the_taps_past_the_last_bin(kernel, n_fft, hop, taps, n_frames):
    assert _kernel_of(n_fft, hop, taps) == kernel
    start, wts = R.overhang(n_fft, taps)
    for kind in ("strong", "weak"):
        iq, win = _signal(kind, n_fft, hop, n_frames)
        db, mm, _, _ = _logmel(iq, win, start, wts, n_fft, hop, n_frames)
        _check_u(f"overhang n_fft {n_fft} hop {hop} taps {taps}", kernel, kind, db, iq, win, n_fft, hop, n_frames, start, wts)
        _check_minmax_exact(db, mm)


@gpu
@pytest.mark.parametrize("kernel,n_fft,hop,n_frames,n_mel,rows", [
    ("wave", 1024, 256, 21, 640, None),
    ("wave", 1024, 256, 21, 600, None),          # a filter count that is no multiple of 64
    ("wave", 1024, 256, 21, 640, 37),            # fewer filters than lanes: 37 of the oracle's 640, evenly spread
    ("stockham", 1024, 128, 9, 640, None),
    ("radix2", 256, 64, 3, 160, None),
    ("radix2", 64, 16, 5, 40, None),
], ids=lambda v: str(v))
def test_oracle_bank(kernel, n_fft, hop, n_frames, n_mel, rows):
    assert _kernel_of(n_fft, hop, 8) == kernel
    start, wts = R.oracle_bank(n_mel, n_fft, rows)
    for kind in ("strong", "weak"):
        iq, win = _signal(kind, n_fft, hop, n_frames)
        db, mm, _, _ = _logmel(iq, win, start, wts, n_fft, hop, n_frames)
        assert db.shape == (B, n_frames, rows or n_mel)
        _check_u(f"oracle bank n_fft {n_fft} hop {hop} n_mel {rows or n_mel}", kernel, kind, db, iq, win, n_fft, hop, n_frames, start, wts)
        _check_minmax_exact(db, mm)


@gpu
@pytest.mark.parametrize("n_fft,hop,n_frames,bank", [(1024, 256, 21, "overhang"), (1024, 128, 9, "oracle"), (256, 64, 3, "overhang")],
                         ids=lambda v: str(v))
def test_mel_w_that_is_not_16_byte_aligned_is_refused_or_right(n_fft, hop, n_frames, bank):
    """An 8-tap `mel_w` one float into a larger buffer.  Measured: the n_fft = 1024 shapes are refused (the 8-tap paths load the
    weights as two 16-byte vectors), the radix-2 kernel reads them one by one and is right."""
    start, wts = R.overhang(n_fft, 8) if bank == "overhang" else R.oracle_bank(640, n_fft)
    buf = torch.full((wts.size + 5,), float("nan"), device=DEV)
    w = buf[1:1 + wts.size].view(wts.shape)
    w.copy_(torch.from_numpy(wts))
    assert w.is_contiguous() and w.data_ptr() % 16 == 4
    iq, win = _signal("strong", n_fft, hop, n_frames)
    try:
        db, mm, _, _ = _logmel(iq, win, start, wts, n_fft, hop, n_frames, mel_w_dev=w)
    except lib().Sy11Error as e:
        print(f"[stft-align] n_fft {n_fft} hop {hop}: refused ({e})")
        assert "aligned" in str(e)
        return
    print(f"[stft-align] n_fft {n_fft} hop {hop}: accepted")
    _check_u(f"unaligned mel_w n_fft {n_fft} hop {hop}", _kernel_of(n_fft, hop, 8, aligned=False), "strong", db, iq, win, n_fft, hop, n_frames, start, wts)
    _check_minmax_exact(db, mm)


# --------------------------------------------------------------------------------------------- 4. min / max, normalise
MM_SHAPES = [("wave", 1024, 256, 8, 21), ("stockham", 1024, 512, 8, 9), ("radix2", 256, 64, 3, 12)]   # the first and last frame do not overlap the middle one


def _check_normalise(db_dev, mm_dev, db, mm):
    img = ops().stft_normalize(db_dev, mm_dev).cpu().numpy()
    want = R.normalise(db, mm)
    assert img.shape == want.shape and np.isfinite(img).all()
    # (db - min) rounded, 1 / (max - min) rounded twice, the product rounded: four roundings of 2^-24 on values <= 1; 1e-6 is eight
    assert np.abs(img - want).max() <= 1e-6, np.abs(img - want).max()
    assert np.array_equal(img[:, 0], img[:, 1]) and np.array_equal(img[:, 0], img[:, 2])
    return img


@gpu
@pytest.mark.parametrize("sign", ["positive", "negative", "mixed"])
@pytest.mark.parametrize("kernel,n_fft,hop,taps,n_frames", MM_SHAPES, ids=lambda v: str(v))
def test_minmax_is_exact_whatever_the_sign(kernel, n_fft, hop, taps, n_frames, sign):
    """atomic_min_f / atomic_max_f take a signed integer atomic for v >= 0 and an unsigned one for v < 0: all three mixtures."""
    assert _kernel_of(n_fft, hop, taps) == kernel
    if sign == "mixed":
        iq, win = R.one_loud_frame(B, R.n_samples(n_fft, hop, n_frames) + R.SPARE, n_fft, hop, n_frames // 2), R.random_window(n_fft)
    else:
        iq, win = _signal("loud" if sign == "positive" else "faint", n_fft, hop, n_frames)
    start, wts = R.identity(n_fft, taps)
    db, mm, db_dev, mm_dev = _logmel(iq, win, start, wts, n_fft, hop, n_frames)
    per_frame = db.max(axis=2)
    if sign == "positive":
        assert db.min() > 0
    elif sign == "negative":
        assert db.max() < 0
    else:
        assert (per_frame[:, n_frames // 2] > 0).all() and (per_frame[:, 0] < 0).all() and (per_frame[:, -1] < 0).all() and db.min() < 0
    _check_minmax_exact(db, mm)
    img = _check_normalise(db_dev, mm_dev, db, mm)
    assert img.min() == 0.0 and abs(float(img.max()) - 1.0) <= 1e-6


@gpu
@pytest.mark.parametrize("kernel,n_fft,hop,taps,n_frames", MM_SHAPES, ids=lambda v: str(v))
def test_silence(kernel, n_fft, hop, taps, n_frames):
    assert _kernel_of(n_fft, hop, taps) == kernel
    iq = np.zeros((B, R.n_samples(n_fft, hop, n_frames) + R.SPARE), dtype=np.complex64)
    start, wts = R.identity(n_fft, taps)
    db, mm, db_dev, mm_dev = _logmel(iq, R.random_window(n_fft), start, wts, n_fft, hop, n_frames)
    assert np.abs(db + 100.0).max() <= 1e-4, np.abs(db + 100.0).max()
    assert (mm[:, 0] == mm[:, 1]).all()
    _check_minmax_exact(db, mm)
    img = ops().stft_normalize(db_dev, mm_dev).cpu().numpy()
    assert np.isfinite(img).all() and (img == 0).all()


@gpu
@pytest.mark.parametrize("n_mel,n_frames", [(37, 33), (64, 32), (1, 70)])
def test_normalize_shapes(n_mel, n_frames):
    """stft_normalize on its own: ragged 32 x 32 tiles both ways, exactly two tiles by one, a single filter."""
    rng = np.random.default_rng(n_mel * 100 + n_frames)
    db = (rng.random((B, n_frames, n_mel)) * 90.0 - 70.0).astype(np.float32)
    mm = R.minmax(db).astype(np.float32)
    guard = torch.full((B * 3 * n_mel * n_frames + 64,), 7.0, device=DEV)
    out = guard[:B * 3 * n_mel * n_frames].view(B, 3, n_mel, n_frames)
    got = ops().stft_normalize(_dev(db), _dev(mm), out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and bool((guard[-64:] == 7.0).all())
    img = got.cpu().numpy()
    assert np.abs(img - R.normalise(db, mm)).max() <= 1e-6
    assert np.array_equal(img[:, 0], img[:, 1]) and np.array_equal(img[:, 0], img[:, 2])
    for b in range(B):
        assert img[b].min() == 0.0 and abs(float(img[b].max()) - 1.0) <= 1e-6


# ------------------------------------------------------------------------------- 5. carry-over against fresh load
@gpu
def test_wave_kernel_carried_frames_equal_fresh_frames_bit_for_bit():
    """One buffer as 322 frames (run 5: a frame's samples are carried over from up to four predecessors), as 322 batch rows of one
    frame (run 1: every frame loaded fresh) and as 21 frames from frame 7 and from frame 300 (run 2, another phase of the run)."""
    n_fft, hop, F = 1024, 256, 322
    iq = R.tone_in_noise(1, R.n_samples(n_fft, hop, F), n_fft, seed=29)
    win = R.random_window(n_fft)
    start, wts = R.identity(n_fft, 8)
    whole = _logmel(iq, win, start, wts, n_fft, hop, F)[2][0]                                   # (322, 1024)
    rows = R.frames_of(iq, n_fft, hop, F)[0]                                                    # (322, 1024): B = 322, one frame each
    fresh = _logmel(rows, win, start, wts, n_fft, hop, 1)[2][:, 0]
    assert same_bits(whole, fresh), f"{int((whole != fresh).any(1).sum())} of {F} frames differ between run 5 and run 1"
    for off in (7, 300):
        part = iq[:, off * hop: off * hop + R.n_samples(n_fft, hop, 21)]
        pair = _logmel(part, win, start, wts, n_fft, hop, 21)[2][0]
        assert same_bits(pair, whole[off:off + 21]), f"frames from {off}: run 2 differs from run 5"


# ---------------------------------------------------------------------------------------------- 6. strip windows
@gpu
@pytest.mark.parametrize("F,n_mel,n_frames,shifted", [
    (75, 37, 40, False),       # n_mel % 4 != 0: the scalar min / max path; ragged 32 x 32 tiles
    (330, 36, 300, False),     # more frames than the window reduce has threads
    (75, 36, 40, True),        # n_mel % 4 == 0 but the strip starts 4 bytes off a 16-byte boundary
], ids=lambda v: str(v))
def test_strip_windows(F, n_mel, n_frames, shifted):
    rng = np.random.default_rng(F + n_mel)
    strip = (rng.random((F, n_mel)) * 90.0 - 70.0).astype(np.float32)
    start = np.array([0, F - n_frames, F - n_frames, -5, F - n_frames + 7, F + 10, 3], dtype=np.int32)
    buf = torch.full((F * n_mel + 8,), float("nan"), device=DEV)
    off = 1 if shifted else 0
    d = buf[off:off + F * n_mel].view(F, n_mel)
    d.copy_(torch.from_numpy(strip))
    assert d.data_ptr() % 16 == 4 * off and d.is_contiguous()
    img, mm = ops().stft_windows(d, _dev(start), n_frames)
    torch.cuda.synchronize()
    img, mm = img.cpu().numpy(), mm.cpu().numpy()
    want, want_mm = R.windows(strip, start, n_frames)
    assert np.array_equal(mm.astype(np.float64), want_mm), (mm, want_mm)
    assert np.isfinite(img).all() and np.abs(img - want).max() <= 1e-6, np.abs(img - want).max()
    for w, s in enumerate(start):
        fr = int(s) + np.arange(n_frames)
        outside = (fr < 0) | (fr >= F)
        assert (img[w][:, :, outside] == 0).all()
    assert (img[5] == 0).all() and np.array_equal(img[1], img[2])
    assert np.array_equal(img[:, 0], img[:, 1]) and np.array_equal(img[:, 0], img[:, 2])


# ---------------------------------------------------------------------------------------------------- 7. wrapper
@gpu
def test_wrapper_refuses_tables_it_would_reinterpret():
    o, Sy11Error = ops(), lib().Sy11Error
    n_fft, hop, n_frames = 256, 64, 3
    iq, win = _signal("strong", n_fft, hop, n_frames)
    start, wts = R.identity(n_fft, 8)
    good = dict(window=_dev(win), mel_start=_dev(start), mel_w=_dev(wts))
    bad = {
        "window float64": dict(window=_dev(win.astype(np.float64))),
        "window short": dict(window=_dev(win[:n_fft - 1])),
        "window 2-d": dict(window=_dev(win.reshape(2, -1))),
        "window strided": dict(window=_dev(np.repeat(win, 2))[::2]),
        "mel_start int64": dict(mel_start=_dev(start.astype(np.int64))),
        "mel_start short": dict(mel_start=_dev(start[:-1])),
        "mel_start strided": dict(mel_start=_dev(np.repeat(start, 2))[::2]),
        "mel_start column": dict(mel_start=_dev(start.reshape(-1, 1))),
        "mel_w float64": dict(mel_w=_dev(wts.astype(np.float64))),
        "mel_w float16": dict(mel_w=_dev(wts.astype(np.float16))),
        "mel_w rows": dict(mel_w=_dev(wts[:-1])),
        "mel_w flat": dict(mel_w=_dev(wts.reshape(-1))),
        "mel_w transposed": dict(mel_w=_dev(np.ascontiguousarray(wts.T)).t()),
        "mel_w column slice": dict(mel_w=_dev(np.concatenate((wts, wts), axis=1))[:, :8]),
    }
    for what, kw in bad.items():
        a = {**good, **kw}
        with pytest.raises(Sy11Error, match=next(iter(kw))):
            o.stft_logmel(_dev(iq), a["window"], a["mel_start"], a["mel_w"], n_fft, hop, n_frames, n_fft)
        print(f"[stft-wrapper] refused: {what}")
    db, mm = o.stft_logmel(_dev(iq), good["window"], good["mel_start"], good["mel_w"], n_fft, hop, n_frames, n_fft)
    assert db.shape == (B, n_frames, n_fft) and bool(torch.isfinite(db).all())


@gpu
def test_producer_tables_pass_the_wrapper_checks():
    """SpectrogramProducer's own window and bank go through the checked wrapper (here at 5 frames), and its image is bit for bit
    what the two ops give when called with the oracle's tables."""
    from oracle import stft_ref as S
    from sy11.data.spectrogram import SpectrogramProducer
    prod = SpectrogramProducer(DEV, n_frames=5)
    iq = S.synthetic_iq(1, seed=2)[:, :prod.n_samples + 11].contiguous().to(DEV)
    img = prod(iq)
    start, wts = R.oracle_bank(640, 1024)
    assert torch.equal(prod.mel_start.cpu(), torch.from_numpy(start)) and torch.equal(prod.mel_w.cpu(), torch.from_numpy(wts))
    o = ops()
    db, mm = o.stft_logmel(iq, torch.hann_window(1024, periodic=True).to(DEV), _dev(start), _dev(wts), 1024, 256, 5, 640)
    assert img.shape == (1, 3, 640, 5) and same_bits(img, o.stft_normalize(db, mm))
