"""Time the frequency-keyed demodulation's three launches (sy11_iq_fsk_filter, sy11_fsk_symbols, sy11_fsk_decide: each ONE launch over all clips)
and, as the point of comparison, the three launches of the PSK demodulation (``demodulate``, order 2) on the SAME packed clips with the same number
of taps.  Workload: CLIPS (default 256) clips of M (default 16 384) samples of GFSK (h = 0.5, bt = 0.5) in noise at 4 and at 16 samples per symbol,
packed in one device buffer as ``Extraction.packed`` holds them; block 32; the Gaussian filter at its default span 2 (17 / 65 taps) and at span 8
(65 / 257 taps, what the PSK filter has at its default span 8).  The launches are timed by the events ``_lib.PROFILE`` records around every call
(so a figure holds the library's own check of the item table), after a warm-up, REPS times; the median is printed.
Usage: demodulate_fsk_micro.py [REPS [CLIPS [M]]]"""
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "spectrogram-yolov11_amd"))
sys.path.insert(0, str(ROOT))
import numpy as np
import torch
from sy11 import _lib
from sy11.data.demodulate import demodulate_extraction
from sy11.data.demodulate_fsk import demodulate_fsk_extraction
from sy11.data.extract import Extraction, ExtractPlan

dev = torch.device("cuda", 0)
FS = 1.0e6


def extraction(k, M, sps, seed):
    """``k`` clips of ``M`` samples of one long GFSK stream: NRZ levels held for ``sps`` samples, smoothed by a Gaussian of bt 0.5, h = 0.5, 0.01 cycles per
    sample off the centre, 20 dB above the noise."""
    g = np.random.default_rng(seed)
    n = k * M
    nrz = np.repeat(1.0 - 2.0 * g.integers(0, 2, n // sps + 2), sps)[3:3 + n]
    t = np.arange(-2 * sps, 2 * sps + 1) / sps
    h = np.exp(-2.0 * np.pi ** 2 * 0.25 * t * t / np.log(2.0))
    f = 0.25 / sps * np.convolve(nrz, h / h.sum(), mode="same") + 0.01
    x = np.exp(2j * np.pi * np.cumsum(f)) + 0.0707 * (g.standard_normal(n) + 1j * g.standard_normal(n))
    Ms = np.full(k, M, dtype=np.int64)
    plan = ExtractPlan(n, FS, 0.0, np.arange(k), np.zeros((k, 4)), np.ones(k, dtype=np.int64), np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.int64), Ms)
    return Extraction(plan, torch.from_numpy(x.astype(np.complex64)).to(dev))


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


def main(reps=5, k=256, M=16384):
    print(f"demodulate_fsk, {torch.cuda.get_device_name(0)}: {k} clips of {M} samples, block 32, {reps} repeats")
    for sps in (4, 16):
        ext = extraction(k, M, sps, 7)
        for span in (2, 8):
            d, ms = launches(lambda: demodulate_fsk_extraction(ext, symbol_rate=FS / sps, offset=0.01 * FS, span=span), reps)
            f, s2, s3 = ms["sy11_iq_fsk_filter"], ms["sy11_fsk_symbols"], ms["sy11_fsk_decide"]
            n_taps = int(d.plan.n_taps[0])
            fma = k * M * 8 * ((n_taps + 7) // 8)                        # real x real FMAs issued: the taps padded to blocks of 8
            print(f"  fsk  sps {sps:2d}, span {span}: {n_taps:3d} taps, {d.plan.total_rows} items, {int(d.n_symbols[d.valid].sum())} symbols, {int(d.valid.sum())} valid, "
                  f"evm {float(np.nanmedian(d.evm)):.3f}, mod_index {float(np.nanmedian(d.mod_index)):.3f}")
            print(f"    filter {f:8.3f} ms: {k * M / f / 1e6:8.2f} G samples/s, {fma / f / 1e9:7.2f} T FMA/s;  symbols {s2:7.3f} ms;  decide {s3:7.3f} ms;  "
                  f"three launches {f + s2 + s3:8.3f} ms = {(f + s2 + s3) / k * 1e3:8.2f} us per clip")
        p, ms = launches(lambda: demodulate_extraction(ext, symbol_rate=FS / sps, offset=0.01 * FS, order=2), reps)
        f, s2, s3 = ms["sy11_iq_demod_filter"], ms["sy11_demod_symbols"], ms["sy11_demod_decide"]
        n_taps = int(p.plan.n_taps[0])
        fma = 2 * k * M * 8 * ((n_taps + 7) // 8)                        # complex x real
        print(f"  psk  sps {sps:2d}, span 8: {n_taps:3d} taps, {p.plan.total_rows} items (the same clips read as BPSK: the work, not the result)")
        print(f"    filter {f:8.3f} ms: {k * M / f / 1e6:8.2f} G samples/s, {fma / f / 1e9:7.2f} T FMA/s;  symbols {s2:7.3f} ms;  decide {s3:7.3f} ms;  "
              f"three launches {f + s2 + s3:8.3f} ms = {(f + s2 + s3) / k * 1e3:8.2f} us per clip")


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:]))
