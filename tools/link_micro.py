"""Time one ``ops.scan_link`` (sort by t0, hook-and-compress labelling, un-permute; device tensors in, device labels out) on synthetic
survivor lists of 10^4, 10^5 and 10^6 rows, beside the float64 union-find sweep of tests/_link_ref.py on the host, at the sizes where
that finishes in under a minute (its time at the previous size, times twelve, decides).  Two kinds of list:
  chains   carriers that stay on for 1000 windows at stride 320 frames: n / 1000 chains of 1000 pieces, 64 frequency slots, random starts
  clutter  short bursts (20 .. 400 frames, 0.2 .. 6 MHz) of 8 classes, about 40 of them on the air at any time
After two warm-up calls the kernel path runs REPS times (default 7); best and median wall times around a device synchronise are printed
with the number of hook passes, the number of tracks, and whether the labels equal the host's.
Usage: link_micro.py [REPS [MAX_LOG10_N]]"""
import statistics
import sys
import time
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "spectrogram-yolov11_amd"))
sys.path.insert(0, str(ROOT))
import numpy as np
import torch
from sy11 import ops
from tests._link_ref import link_ref

dev = torch.device("cuda", 0)
FS, FC, HOP = 20e6, 2.4e9, 256
FRAME = HOP / FS
GAP = 8 * FRAME


def chains(n, seed=0):
    g = np.random.default_rng(seed)
    length = min(1000, n)
    m = n // length
    first = g.integers(0, 200 * 320, m)[:, None] + 320 * np.arange(length)[None, :]              # first frame of every piece
    slot = (np.arange(m) % 64)[:, None] + np.zeros((1, length))
    t0 = (first + g.uniform(0, 2, first.shape)) * FRAME
    t1 = (first + 640 - g.uniform(0, 2, first.shape)) * FRAME
    f0 = FC - FS / 2 + slot * (FS / 64) + g.uniform(0, 2e3, first.shape)
    tf = np.stack((t0, f0, t1, f0 + 0.8 * FS / 64), 2).reshape(-1, 4)
    cls = np.repeat(np.arange(m) % 8, length)
    p = g.permutation(tf.shape[0])
    return tf[p], cls[p]


def clutter(n, seed=1):
    g = np.random.default_rng(seed)
    dur = g.uniform(20, 400, n)
    t0 = g.uniform(0, n * dur.mean() / 40, n)
    bw = g.uniform(0.2e6, 6e6, n)
    f0 = FC - FS / 2 + g.uniform(0, 1, n) * (FS - bw)
    return np.stack((t0 * FRAME, f0, (t0 + dur) * FRAME, f0 + bw), 1), g.integers(0, 8, n)


def main(reps=7, max_log10=6):
    print(f"link, {torch.cuda.get_device_name(0)}: gap_t = 8 hops, align = 0.5, class-aware, time branch only; {reps} timed calls after 2 warm-ups")
    for name, make in (("chains", chains), ("clutter", clutter)):
        host_s = 0.0
        for e in range(4, max_log10 + 1):
            n = 10 ** e
            tf, cls = make(n)
            d_tf, d_cls = torch.from_numpy(tf).to(dev), torch.from_numpy(cls).to(dev)
            for _ in range(2):
                lab, passes = ops.scan_link(d_tf, d_cls, GAP, return_passes=True)
            times = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t = time.perf_counter()
                lab = ops.scan_link(d_tf, d_cls, GAP)
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t)
            lab = lab.cpu().numpy()
            line = (f"  {name:<8} n = 10^{e}: kernel path best {min(times) * 1e3:9.3f} ms, median {statistics.median(times) * 1e3:9.3f} ms, "
                    f"{passes} passes, {np.unique(lab).size} tracks")
            if host_s * 12 < 60:
                t = time.perf_counter()
                want = link_ref(tf, cls, GAP)
                host_s = time.perf_counter() - t
                line += f"; host sweep {host_s * 1e3:10.1f} ms ({host_s / statistics.median(times):8.1f} x), labels equal: {bool(np.array_equal(lab, want))}"
            else:
                line += "; host sweep not run (over a minute)"
            print(line, flush=True)


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]))
