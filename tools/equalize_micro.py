"""Time the two launches of the equaliser (sy11_eq_solve: one wavefront per frame; sy11_eq_apply: one workgroup per 256 symbols of a segment) on 4 096 frames of
32 + 1 024 symbols, one clip of 1 056 symbols each (4.3 million symbols), four-phase behind the three-path channel [1, 0.45 e^{2.0i}, 0.2 e^{-1.0i}] at 22 dB, at 7
and 15 taps: the first pass (trained on the 32-symbol word) and the second pass of refine = 256 (trained on 256 symbols, 224 of them the first pass's
decisions).  Per launch one warm-up call, then REPS calls, each between two events on the stream; the median is printed.  A call is the library's entry point
with the tables already on the device: its host-side checks and the kernel.  The taps of the first frames are compared with the numpy reference
(tests/_eq_ref.py) within its rounding bound, their symbols and decisions bit for bit.
Usage: equalize_micro.py [REPS]"""
import ctypes as C
import sys
import time
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "spectrogram-yolov11_amd"))
sys.path.insert(0, str(ROOT))
import numpy as np
import torch
from sy11 import _lib
from sy11.data.equalize import EQFRAME, EQITEM, EQSEGMENT
from tests import _eq_ref as E
from tests import _frames_ref as F
from tests._demod_ref import point

dev = torch.device("cuda", 0)
FRAMES, L, PAYLOAD, REFINE, REG, ORDER = 4096, 32, 1024, 256, 1e-3, 4
CHANNEL = [1.0, 0.45 * np.exp(2.0j), 0.2 * np.exp(-1.0j)]


def timed(name, args, reps):
    _lib.call(name, *args)
    torch.cuda.synchronize()
    ms, host = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        _lib.call(name, *args)
        host.append((time.perf_counter() - t0) * 1e3)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), min(ms), max(ms), float(np.median(host))


def main(reps=10):
    n = L + PAYLOAD
    total = FRAMES * n
    print(f"equaliser, {torch.cuda.get_device_name(0)}: {FRAMES} frames of {L} + {PAYLOAD} symbols ({total / 1e6:.2f} M symbols), reg {REG}, {reps} calls after one warm-up, the median")
    g = np.random.default_rng(5)
    d = g.integers(0, ORDER, total).astype(np.uint8)
    r = E.channel(point(d, ORDER), CHANNEL, 22.0, 6)
    words = np.ascontiguousarray(d.reshape(FRAMES, n)[:, :L]).reshape(-1)
    fr = np.zeros(FRAMES, dtype=EQFRAME)
    fr["sym_off"], fr["n_sym"], fr["word_off"], fr["L"], fr["Lt"], fr["order"], fr["row"], fr["gain"] = np.arange(FRAMES) * n, n, np.arange(FRAMES) * L, L, L, ORDER, np.arange(FRAMES), 1.0
    fr2 = fr.copy()
    fr2["Lt"] = REFINE
    sg = np.zeros(FRAMES, dtype=EQSEGMENT)
    sg["sym_off"], sg["n_sym"], sg["end"], sg["frame"], sg["order"] = fr["sym_off"], n, n, np.arange(FRAMES), ORDER
    tiles = -(-n // 256)
    it = np.zeros(FRAMES * tiles, dtype=EQITEM)
    it["seg"], it["tile"] = np.repeat(np.arange(FRAMES), tiles), np.tile(np.arange(tiles), FRAMES)
    p = lambda t: C.c_void_p(t.data_ptr())                                     # noqa: E731
    up = lambda a: torch.from_numpy(a.view(np.uint8)).to(dev)                  # noqa: E731
    sym, wd = torch.from_numpy(r).to(dev), torch.from_numpy(words).to(dev)
    t1, t2, ts, ti = up(fr), up(fr2), up(sg), up(it)
    out, dec = torch.zeros_like(sym), torch.zeros(total, dtype=torch.uint8, device=dev)
    w = torch.zeros((FRAMES, 15), dtype=torch.complex128, device=dev)
    rows = torch.zeros((FRAMES, 4), dtype=torch.float64, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for N in (7, 15):
        solve1 = (FRAMES, C.c_void_p(fr.ctypes.data), p(t1), N, REG, words.shape[0], p(wd), total, p(sym), None, FRAMES, p(w), p(rows), stream)
        solve2 = (FRAMES, C.c_void_p(fr2.ctypes.data), p(t2), N, REG, words.shape[0], p(wd), total, p(sym), p(dec), FRAMES, p(w), p(rows), stream)
        apply = (it.shape[0], C.c_void_p(it.ctypes.data), p(ti), FRAMES, C.c_void_p(sg.ctypes.data), p(ts), N, FRAMES, p(w), total, p(sym), p(out), p(dec), stream)
        s1 = timed("sy11_eq_solve", solve1, reps)
        a1 = timed("sy11_eq_apply", apply, reps)
        w1, e1, d1 = w.cpu().numpy(), out.cpu().numpy(), dec.cpu().numpy()
        s2 = timed("sy11_eq_solve", solve2, reps)
        a2 = timed("sy11_eq_apply", apply, reps)
        w2, e2, d2, h = w.cpu().numpy(), out.cpu().numpy(), dec.cpu().numpy(), rows.cpu().numpy()
        same, worst = True, 0.0
        for k in (0, 1, FRAMES - 1):
            clip = r[k * n:(k + 1) * n]
            t = E.target(words[k * L:(k + 1) * L], ORDER, 0, 1.0)
            for wk, ek, dk, tk in ((w1, e1, d1, t), (w2, e2, d2, np.concatenate((t, point(d1[k * n + L:k * n + REFINE], ORDER))))):
                ref = E.solve(clip, 0, tk, N, REG)
                worst = max(worst, np.linalg.norm(wk[k, :N] - ref["w"]) / (8.0 * (len(tk) + N * N) * ref["cond"] * 2.0 ** -53 * np.linalg.norm(ref["w"])))
                want = E.fir(clip, wk[k, :N], np.arange(n))
                same = same and np.array_equal(ek[k * n:(k + 1) * n].view(np.uint32), want.view(np.uint32)) and np.array_equal(dk[k * n:(k + 1) * n], F.decide(want, ORDER))
        err0, err1, err2 = (int((x != d).sum()) for x in (F.decide(r, ORDER), d1, d2))
        for label, (t, lo, hi, host), unit in ((f"solve, Lt = {L}", s1, FRAMES), ("apply", a1, total), (f"solve, Lt = {REFINE}", s2, FRAMES), ("apply", a2, total)):
            rate = f"{t / unit * 1e6:8.1f} ns per frame" if unit == FRAMES else f"{unit / t / 1e6:8.2f} G symbols/s, {unit * 17 / t / 1e9:6.2f} TB/s of HBM traffic, {unit * 8 * N / t / 1e9:6.2f} T float64 operations/s"
            print(f"  {N:2d} taps, {label:16s}: {t:8.3f} ms (min {lo:.3f}, max {hi:.3f}; of which the host's checks and the enqueue {host:.3f}) = {rate}")
        print(f"  {N:2d} taps: decision errors {err0} -> {err1} -> {err2} of {total}; mse {h[:, 0].mean():.4f} -> {h[:, 1].mean():.4f}; the taps of frames 0, 1 and {FRAMES - 1} within {worst:.4f} of "
              f"the reference's bound, their symbols and decisions {'equal' if same else 'DIFFER FROM'} numpy's")


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:]))
