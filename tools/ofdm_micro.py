"""Time the OFDM demodulation's three launches (sy11_iq_ofdm_fold, sy11_ofdm_fft, sy11_ofdm_decide: each ONE launch over all clips) and, as the point of comparison for the
FFT launch, ``sy11_iq_cyclo`` (``characterize``) on the SAME packed clips at the same ``n_fft``: the same LDS FFT core doing three transforms per frame where launch 2 does one.
Workload: CLIPS (default 256) clips of PERIODS (default 64) OFDM periods at N = 64 (the 802.11a layout) and at N = 1024 (600 data carriers, 12 pilots, prefix 72), QPSK in noise,
packed in one device buffer as ``Extraction.packed`` holds them.  The launches are timed by the events ``_lib.PROFILE`` records around every call (so a figure holds the library's
own check of the item table), after a warm-up, REPS times; the median is printed, with the bytes each launch must move and the fraction of HBM (8 TB/s) that makes.
Usage: ofdm_micro.py [REPS [CLIPS [PERIODS]]]"""
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "spectrogram-yolov11_amd"))
sys.path.insert(0, str(ROOT))
import numpy as np
import torch
from sy11 import _lib
from sy11.data.characterize import characterize_extraction
from sy11.data.demodulate_ofdm import demodulate_ofdm_extraction
from sy11.data.extract import Extraction, ExtractPlan

dev = torch.device("cuda", 0)
FS, HBM = 1.0e6, 8.0e12
LAYOUTS = {64: (16, 26, tuple(range(-21, 22, 14))), 1024: (72, 306, tuple(range(-275, 276, 50)))}      # prefix, the used carriers +-1 .. +-half, the pilots


def extraction(k, periods, N, seed):
    """``k`` clips of one QPSK OFDM symbol repeated with fresh data ``periods`` times after a lead of N / 2 samples, 0.2 carrier spacings off, 20 dB above the noise."""
    G, half, pk = LAYOUTS[N]
    g = np.random.default_rng(seed)
    used = np.array([c for c in range(-half, half + 1) if c], dtype=np.int64)
    data = used[~np.isin(used, pk)]
    S, M = N + G, N // 2 + periods * (N + G) + N
    X = np.zeros((k * periods, N), dtype=np.complex128)
    X[:, data % N] = ((1 - 2 * g.integers(0, 2, (k * periods, data.shape[0]))) + 1j * (1 - 2 * g.integers(0, 2, (k * periods, data.shape[0])))) / np.sqrt(2.0)
    X[:, np.array(pk) % N] = 1.0
    t = np.fft.ifft(X, axis=1) * N / np.sqrt(used.shape[0])
    s = np.concatenate((t[:, -G:], t), axis=1).reshape(k, periods * S)
    x = np.zeros((k, M), dtype=np.complex128)
    x[:, N // 2:N // 2 + periods * S] = s
    x = x * np.exp(2j * np.pi * 0.2 * np.arange(M) / N)[None, :] + 0.0707 * (g.standard_normal((k, M)) + 1j * g.standard_normal((k, M)))
    Ms = np.full(k, M, dtype=np.int64)
    plan = ExtractPlan(k * M, FS, 0.0, np.arange(k), np.zeros((k, 4)), np.ones(k, dtype=np.int64), np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.int64), Ms)
    return Extraction(plan, torch.from_numpy(x.reshape(-1).astype(np.complex64)).to(dev)), dict(n_fft=N, cp=G, carriers=data, pilots=(pk, [1] * len(pk)))


def launches(fn, reps):
    """-> (the last result, {name: median ms})."""
    d = fn()
    times = {}
    for _ in range(reps):
        _lib.PROFILE = []
        try:
            d = fn()
            torch.cuda.synchronize()
            for name, e0, e1, _ in _lib.PROFILE:
                times.setdefault(name, []).append(e0.elapsed_time(e1))
        finally:
            _lib.PROFILE = None
    return d, {k: float(np.median(v)) for k, v in times.items()}


def main(reps=5, k=256, periods=64):
    print(f"demodulate_ofdm, {torch.cuda.get_device_name(0)}: {k} clips of {periods} periods, {reps} repeats")
    for N in (64, 1024):
        ext, kw = extraction(k, periods, N, 7)
        d, ms = launches(lambda: demodulate_ofdm_extraction(ext, **kw), reps)
        t1, t2, t3 = ms["sy11_iq_ofdm_fold"], ms["sy11_ofdm_fft"], ms["sy11_ofdm_decide"]
        lay, n_in = d.plan.lay(0), ext.packed.shape[0]
        frames = int(d.n_ofdm.sum())
        b1 = 2 * 8 * int((d.plan.periods * lay.S).sum())                      # launch 1: every folded sample is read twice
        b2 = 8 * frames * lay.n_fft + 8 * frames * lay.n_used                 # launch 2: the windows in, Yc out
        print(f"  N {N:4d}, G {lay.cp}: {n_in} samples, {frames} OFDM symbols ({int(d.n_active.sum())} active), {lay.n_data} data carriers, evm {float(np.nanmedian(d.evm)):.3f}, "
              f"cfo {float(np.nanmedian(d.cfo)):+.4f}, {d.raw['tables']['fold'].shape[0]} / {d.raw['tables']['fft'].shape[0]} / {d.raw['tables']['dec'].shape[0]} items")
        print(f"    fold {t1:8.3f} ms: {b1 / 1e6:8.2f} MB = {b1 / t1 / 1e9:7.3f} TB/s ({b1 / t1 * 1e3 / HBM:.3f} of HBM);  fft {t2:8.3f} ms: {b2 / 1e6:8.2f} MB = "
              f"{b2 / t2 / 1e9:7.3f} TB/s ({b2 / t2 * 1e3 / HBM:.3f} of HBM), {t2 / frames * 1e6:7.1f} ns per frame;  decide {t3:7.3f} ms;  three launches {t1 + t2 + t3:8.3f} ms = "
              f"{(t1 + t2 + t3) / k * 1e3:8.2f} us per clip")
        c, ms = launches(lambda: characterize_extraction(ext, n_fft=N), reps)
        tc = ms["sy11_iq_cyclo"]
        cf = int(((ext.plan.M - N) // (N // 2) + 1).sum())                    # frames of N samples, hop N / 2, three transforms each
        print(f"    iq_cyclo at n_fft {N}: {tc:8.3f} ms for {cf} frames of three transforms = {tc / cf * 1e6:7.1f} ns per frame, {tc / cf / 3 * 1e6:7.1f} ns per transform")


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:]))
