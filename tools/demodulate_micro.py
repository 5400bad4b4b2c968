"""Time the demodulation's three launches (sy11_iq_demod_filter, sy11_demod_symbols, sy11_demod_decide: each ONE launch over all clips)
against a per-clip torch loop on the same device doing the same work: de-rotation, one ``conv1d`` with the clip's taps over its two planes,
and a four-point gather with the cubic weights at the symbol instants.  Workload: 1 / 64 / 1 024 clips (or CLIPS ...) of 8 192 samples, NRZ
BPSK in noise at 4 and at 16 samples per symbol, packed in one device buffer as ``Extraction.packed`` holds them; span 8, so 65 and 257 taps.
The launches are timed by the events ``_lib.PROFILE`` records around every call, after a warm-up, REPS times (the median is printed); the
loop's symbols are compared with the kernels' so that the two do the same work.  Usage: demodulate_micro.py [REPS [CLIPS ...]]"""
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "spectrogram-yolov11_amd"))
sys.path.insert(0, str(ROOT))
import numpy as np
import torch
from sy11 import _lib
from sy11.data.demodulate import demodulate_extraction
from sy11.data.extract import Extraction, ExtractPlan

dev = torch.device("cuda", 0)
FS, M = 1.0e6, 8192


def extraction(k, sps, seed):
    g = np.random.default_rng(seed)
    n = k * M
    sym = 2.0 * g.integers(0, 2, n // sps + 2) - 1.0
    x = np.repeat(sym, sps)[3:3 + n] * np.exp(2j * np.pi * (0.01 * np.arange(n) + 0.1)) + 0.1 * (g.standard_normal(n) + 1j * g.standard_normal(n))
    Ms = np.full(k, M, dtype=np.int64)
    plan = ExtractPlan(n, FS, 0.0, np.arange(k), np.zeros((k, 4)), np.ones(k, dtype=np.int64), np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.int64), Ms)
    return Extraction(plan, torch.from_numpy(x.astype(np.complex64)).to(dev))


def launches(ext, sps, reps):
    """-> (the last Demodulation, {name: median ms})."""
    kw = dict(symbol_rate=FS / sps, offset=0.01 * FS, order=2)
    d = demodulate_extraction(ext, **kw)
    times = {}
    for _ in range(reps):
        _lib.PROFILE = []
        try:
            d = demodulate_extraction(ext, **kw)
            torch.cuda.synchronize()
            for name, e0, e1, _ in _lib.PROFILE:
                times.setdefault(name, []).append(e0.elapsed_time(e1))
        finally:
            _lib.PROFILE = None
    return d, {k: float(np.median(v)) for k, v in times.items()}


def torch_loop(ext, d):
    """The same work with torch, clip by clip -> the interpolated symbols of every clip, packed."""
    plan = d.plan
    out = []
    for i in range(len(plan)):
        a, hw = int(plan.offset[i]), int(plan.hw[i])
        x = ext.packed[a:a + M]
        n = torch.arange(M, device=dev, dtype=torch.float64)
        xr = x * torch.exp(-2j * np.pi * torch.remainder(n * (plan.Wc[i] / 2.0 ** 64), 1.0)).to(torch.complex64)
        h = torch.from_numpy(plan.taps[int(plan.tap_off[i]):int(plan.tap_off[i + 1])].copy()).to(dev)
        y = torch.nn.functional.conv1d(torch.view_as_real(xr).t().unsqueeze(0), h.flip(0).expand(2, 1, -1).contiguous(), padding=hw, groups=2)[0]
        t = d.raw["T0"][i] + (d.raw["i_first"][i] + torch.arange(int(d.n_symbols[i]), device=dev, dtype=torch.int64)) * d.raw["STEP"][i]
        k, mu = t >> 32, (((t & 0xffffffff) >> 8).to(torch.float32) * 2.0 ** -24)
        c = (-mu * (mu - 1) * (mu - 2) / 6, (mu + 1) * (mu - 1) * (mu - 2) / 2, -(mu + 1) * mu * (mu - 2) / 2, (mu + 1) * mu * (mu - 1) / 6)
        s = sum(c[j] * y[:, k - 1 + j] for j in range(4))
        out.append(torch.complex(s[0], s[1]))
    return torch.cat(out)


def timed(fn, reps):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main(reps=5, *clips):
    print(f"demodulate, {torch.cuda.get_device_name(0)}: clips of {M} samples, span 8, block 32, {reps} repeats")
    for sps in (4, 16):
        for k in (clips or (1, 64, 1024)):
            ext = extraction(k, sps, 7)
            d, ms = launches(ext, sps, reps)
            f, s2, s3 = ms["sy11_iq_demod_filter"], ms["sy11_demod_symbols"], ms["sy11_demod_decide"]
            n_taps, items = int(d.plan.n_taps[0]), d.plan.total_rows
            macs = k * M * 8 * ((n_taps + 7) // 8)                       # complex x real MACs issued: the taps padded to blocks of 8
            ms_t = timed(lambda: torch_loop(ext, d), max(1, reps // 2 if k > 64 else reps))
            err = float((torch_loop(ext, d) - d.raw["s"]).abs().max() / d.raw["s"].abs().max())
            print(f"  sps {sps:2d}, {k:4d} clips: {n_taps} taps, {items} items, {int(d.n_symbols.sum())} symbols; the loop's symbols agree to {err:.1e} of their maximum")
            print(f"    filter {f:8.3f} ms: {k * M / f / 1e6:8.2f} G samples/s, {2 * macs / f / 1e9:7.2f} T FMA/s;  symbols {s2:7.3f} ms;  decide {s3:7.3f} ms;  "
                  f"three launches {f + s2 + s3:8.3f} ms = {(f + s2 + s3) / k * 1e3:8.2f} us per clip")
            print(f"    torch conv1d + gather loop {ms_t:9.3f} ms = {ms_t / k * 1e3:8.2f} us per clip: {ms_t / (f + s2 + s3):6.1f} x the three launches")


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:]))
