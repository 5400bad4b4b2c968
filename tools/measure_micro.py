"""Time the measurement (sy11_iq_psd, one launch per staged chunk, and sy11_psd_measure, one launch) in frames per second, bytes read per
second (sum of J H 8 over the boxes: what the frames cover, every sample counted once per box) and wall time per box, at n_fft = 1024 and
256.  Workload: a synthetic capture of 2^LOG2N samples (default 24) resident on the device and BOXES (default 1000) seeded boxes of
2^14 .. 2^18 samples each, anywhere in the capture (so they overlap in time and recompute the same frames: the redundancy is printed).
Both stages are timed with events after a warm-up, REPS times (default 5).  The yardstick printed beside them is the frame rate of the
scan's own STFT kernel (sy11_stft_logmel, n_fft = 1024, hop = 256) over the same capture in the same process.
Usage: measure_micro.py [LOG2N [BOXES [REPS]]]"""
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "spectrogram-yolov11_amd"))
sys.path.insert(0, str(ROOT))
import numpy as np
import torch
from sy11 import ops
from sy11.data.measure import measure_capture, plan_measure, plan_measure_chunks, tables_on

dev = torch.device("cuda", 0)
FS, FC = 61.44e6, 3.5e9


def boxes(n, k, seed=1):
    g = np.random.default_rng(seed)
    length = (2.0 ** g.uniform(14, 18, k)).astype(np.int64)
    start = g.integers(0, n - (1 << 18), k)
    bw = FS * g.uniform(0.01, 0.2, k)
    centre = FC + g.uniform(-0.5, 0.5, k) * (FS - bw)
    return np.stack((start / FS, centre - bw / 2, (start + length) / FS, centre + bw / 2), 1)


def timed(fn, reps):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main(log2n=24, k=1000, reps=5):
    n = 1 << log2n
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.view_as_complex(torch.randn((n, 2), generator=g, device=dev, dtype=torch.float32) * 0.1)
    tf = boxes(n, k)
    print(f"measure, {torch.cuda.get_device_name(0)}: capture of 2^{log2n} samples on the device, {k} boxes")
    for N in (1024, 256):
        plan = plan_measure(tf, n, FS, FC, n_fft=N)
        H = N // 2
        chunks = plan_measure_chunks(plan, 1 << 24)
        items = np.concatenate([c.items for c in chunks])
        window, twiddle, nw2 = tables_on(dev, N)
        partial = torch.empty((plan.total_rows, N), dtype=torch.float32, device=dev)
        env = torch.empty((plan.total_frames,), dtype=torch.float32, device=dev)
        distinct = np.unique(np.concatenate([np.arange(j, j + J) for j, J in zip(plan.j_first.tolist(), plan.J.tolist())])).shape[0]

        def stage1():
            for c in chunks:
                ops.iq_psd(x[c.a:c.b], c.a, n, N, c.items, window, twiddle, nw2, partial, env)
        bx = plan.boxes()
        ms1 = timed(stage1, reps)
        ms2 = timed(lambda: ops.psd_measure(partial, bx, plan.frac_lo, plan.frac_hi), reps)
        ms = timed(lambda: measure_capture(x, plan, dev), reps)
        frames, nbytes = plan.total_frames, plan.total_frames * H * 8
        print(f"  n_fft {N:4d}: {frames} frames in {items.shape[0]} items ({frames / distinct:.2f} x the {distinct} distinct frames), {len(chunks)} chunk(s)")
        print(f"    stage 1 {ms1:8.3f} ms: {frames / ms1 / 1e3:9.2f} M frames/s, {nbytes / ms1 / 1e6:8.1f} GB/s read (sum J H 8)")
        print(f"    stage 2 {ms2:8.3f} ms; whole measure_capture (tables, launches, results to the host) {ms:8.3f} ms = {ms / k * 1e3:7.2f} us per box")
    from sy11.data.spectrogram import SpectrogramProducer                  # the yardstick: the scan's STFT at n_fft = 1024
    p = SpectrogramProducer(dev)
    n_frames = (n - p.n_fft) // p.hop + 1
    db = lambda: ops.stft_logmel(x[None, :], p.window, p.mel_start, p.mel_w, p.n_fft, p.hop, n_frames, p.n_mel)      # noqa: E731
    ms = timed(db, reps)
    print(f"  sy11_stft_logmel, n_fft {p.n_fft}, hop {p.hop}: {n_frames} frames in {ms:8.3f} ms = {n_frames / ms / 1e3:9.2f} M frames/s, "
          f"{n * 8 / ms / 1e6:8.1f} GB/s of input")


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:4]))
