"""Time the frame search's three launches (sy11_sync_correlate, sy11_sync_peaks, sy11_sync_frames: each ONE launch over all clips and words)
and the numpy definition on the same data.  Workload: 1 / 64 / 1 024 clips (or CLIPS ...) of 8 192 symbols, half BPSK and half four-phase
(one clip: BPSK), unit points at a random rotation in noise, packed in one device buffer as ``Demodulation.symbols`` are; two words of 64 and
128 bits (64 and 128 symbols at order 2, 32 and 64 at order 4), the first embedded every 1 024 symbols; 256 payload symbols per frame.  Each
launch is repeated REPS times after a warm-up between two events on the stream (the mean is printed; one launch alone is too short a window
for the small sizes); the numpy loop (the correlation over k, the peaks among the positions at or above the threshold) runs once on the
first clips, at most 8 of them, and is quoted per clip.  The kernels' rho2 and hits are compared with numpy's on those clips.  A launch's
time is that of the whole call as a user pays it: the checks of the item table on the host, its copy to the device, and the kernel.
Usage: frames_micro.py [REPS [CLIPS ...]]"""
import sys
import time
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "spectrogram-yolov11_amd"))
sys.path.insert(0, str(ROOT))
import numpy as np
import torch
from sy11 import ops
from sy11.data.frames import FRAME, plan_frames, word_decisions

dev = torch.device("cuda", 0)
N, EVERY, PAYLOAD, THRESHOLD = 8192, 1024, 256, 0.8


def workload(k, words, seed):
    g = np.random.default_rng(seed)
    orders = np.array([2 if i % 2 == 0 else 4 for i in range(k)])
    clips = []
    for o in orders:
        d = g.integers(0, o, N).astype(np.uint8)
        w = word_decisions(np.array(words[0], dtype=np.uint8), int(o))
        for p in range(100, N - len(w), EVERY):
            d[p:p + len(w)] = w
        pts = (1.0 - 2.0 * (d & 1)) + 0j if o == 2 else ((1.0 - 2.0 * (d >> 1)) + 1j * (1.0 - 2.0 * (d & 1))) / np.sqrt(2.0)
        pts = pts * np.exp(2j * np.pi * g.integers(0, o) / o)
        clips.append((pts + 0.1 * (g.standard_normal(N) + 1j * g.standard_normal(N))).astype(np.complex64))
    return clips, orders


def numpy_pair(r, w, order, thr2):
    """The definition for one pair -> (rho2, hit)."""
    re, im = r.real.astype(np.float64), r.imag.astype(np.float64)
    c = (1.0 - 2.0 * (w & 1)) + 0j if order == 2 else (1.0 - 2.0 * (w >> 1)) + 1j * (1.0 - 2.0 * (w & 1))
    L, P = len(w), len(r) - len(w) + 1
    Cr, Ci, E = np.zeros(P), np.zeros(P), np.zeros(P)
    for k in range(L):
        a, b = re[k:k + P], im[k:k + P]
        Cr = Cr + (a * c[k].real + b * c[k].imag)
        Ci = Ci + (b * c[k].real - a * c[k].imag)
        E = E + (a * a + b * b)
    rho2 = np.where(E == 0.0, 0.0, (Cr * Cr + Ci * Ci) / (float((order // 2) * L) * E))
    hit = np.zeros(P, dtype=np.uint8)
    for p in np.flatnonzero(rho2 >= thr2):
        hit[p] = not ((rho2[max(p - L + 1, 0):p] >= rho2[p]).any() or (rho2[p + 1:p + L] > rho2[p]).any())
    return rho2, hit


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main(reps=50, *counts):
    g = np.random.default_rng(1)
    words = [g.integers(0, 2, 64).tolist(), g.integers(0, 2, 128).tolist()]
    print(f"frame search, {torch.cuda.get_device_name(0)}: clips of {N} symbols, words of 64 and 128 bits, threshold {THRESHOLD}, {PAYLOAD} payload symbols, "
          f"{reps} repeats per launch")
    for k in (counts or (1, 64, 1024)):
        clips, orders = workload(k, words, 7)
        plan = plan_frames((np.full(k, N), orders), words, PAYLOAD, THRESHOLD)
        items = plan.items()[0]
        sym, wbuf = torch.from_numpy(np.concatenate(clips)).to(dev), torch.from_numpy(plan.word_buf).to(dev)
        n_pos = plan.total_positions
        rho2, q = torch.zeros(n_pos, dtype=torch.float64, device=dev), torch.zeros(n_pos, dtype=torch.uint8, device=dev)
        hit = torch.zeros(n_pos, dtype=torch.uint8, device=dev)
        t1 = timed(lambda: ops.sync_correlate(sym, items, wbuf, rho2, q), reps)
        t2 = timed(lambda: ops.sync_peaks(rho2, items, THRESHOLD * THRESHOLD, hit, sym.shape[0], wbuf.shape[0]), reps)
        at = torch.nonzero(hit).squeeze(1).cpu().numpy()
        pair = np.searchsorted(plan.pos0, at, side="right") - 1
        clip = pair // 2
        fr = np.zeros(at.shape[0], dtype=FRAME)
        fr["sym_off"], fr["n_sym"], fr["word_off"], fr["p"] = plan.sym_off[clip], N, plan.word_off.reshape(-1)[pair], at - plan.pos0[pair]
        fr["L"], fr["order"], fr["q"], fr["payload"], fr["row"] = plan.L.reshape(-1)[pair], orders[clip], q[torch.from_numpy(at).to(dev)].cpu().numpy(), PAYLOAD, np.arange(at.shape[0])
        rows = torch.zeros((at.shape[0], 3), dtype=torch.int32, device=dev)
        bits = torch.zeros((at.shape[0], PAYLOAD // 4), dtype=torch.uint8, device=dev)
        t3 = timed(lambda: ops.sync_frames(sym, fr, wbuf, rows, bits), reps)
        steps = int((plan.P * plan.L).sum())                               # position x word-symbol steps of launch 1
        # the definition in numpy on the first clips
        m = min(k, 8)
        rh, hh = rho2.cpu().numpy(), hit.cpu().numpy()
        t0, same = time.perf_counter(), True
        for i in range(m):
            for j in range(2):
                w = word_decisions(np.array(words[j], dtype=np.uint8), int(orders[i]))
                a, b = numpy_pair(clips[i], w, int(orders[i]), THRESHOLD * THRESHOLD)
                sl = slice(int(plan.pos0[i * 2 + j]), int(plan.pos0[i * 2 + j + 1]))
                same = same and np.array_equal(a, rh[sl]) and np.array_equal(b, hh[sl])
        t_np = (time.perf_counter() - t0) / m * 1e3
        print(f"  {k:4d} clips: {items.shape[0]} items, {n_pos} positions, {at.shape[0]} frames ({int(rows[:, 0].sum())} word symbol errors); on the first {m} clips rho2 and hit "
              f"{'equal' if same else 'DIFFER FROM'} numpy's")
        print(f"    correlate {t1:8.3f} ms: {steps / t1 / 1e6:8.2f} G steps/s;  peaks {t2:7.3f} ms;  frames {t3:7.3f} ms;  three launches {t1 + t2 + t3:8.3f} ms = "
              f"{(t1 + t2 + t3) / k * 1e3:8.2f} us per clip;  numpy {t_np:8.2f} ms per clip: {t_np * k / (t1 + t2 + t3):7.1f} x the three launches")


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:]))
