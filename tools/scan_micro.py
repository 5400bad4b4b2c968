"""Windows per second of the long-capture scan on one MI355X, against the composition the package offered before it
(slice the windows on the host, SpectrogramProducer.__call__, DetectionPredictor.__call__) on the same capture:
  (a) images only: producer.scan vs producer(stacked host slices)
  (b) whole path:  predictor.scan (merge "ios") vs predictor(stacked host slices), yolo11s f16
at overlap 0, 0.5 and 0.75.  Wall clock around a device synchronisation (the host -> device copies are part of both paths);
2 warm-up runs (graph capture of both batch signatures happens there), 5 timed repeats, median and min..max shown.
    python tools/scan_micro.py [--windows 192] [--out profiles/r06/scan_micro.txt]"""
import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "spectrogram-yolov11_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from sy11.data import spectrogram as sp  # noqa: E402
from sy11.engine.predictor import DetectionPredictor  # noqa: E402
from sy11.nn.tasks import DetectionModel  # noqa: E402


def timed(fn, warmup=2, repeats=5):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=192, help="length of the capture in non-overlapping windows")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    p = sp.SpectrogramProducer(dev)
    n = p.n_fft + (a.windows * p.n_frames - 1) * p.hop
    rng = np.random.default_rng(0)
    iq = (rng.standard_normal(n, dtype=np.float32) + 1j * rng.standard_normal(n, dtype=np.float32)).astype(np.complex64) * 0.1
    t = np.arange(n // 4, dtype=np.float32)
    iq[n // 8:n // 8 + n // 4] += np.exp(2j * np.pi * (0.05 * t + 0.1 * t * t / t.size)).astype(np.complex64)
    model = DetectionModel("yolo11s.yaml", nc=2, verbose=False)
    pred = DetectionPredictor(model, device=dev, conf=0.25, iou=0.7, half=True, producer=p)
    lines = [f"scan_micro: capture of {a.windows} windows ({n} samples, {n * 8 / 1e6:.0f} MB), batch {a.batch}, yolo11s f16, "
             f"{torch.cuda.get_device_name(0)}", "windows/s: median (min .. max) of 5 repeats after 2 warm-up runs",
             f"{'overlap':>8} {'windows':>8} | {'(a) producer.scan':>28} {'(a) slices + producer()':>28} | {'(b) predictor.scan':>28} "
             f"{'(b) slices + predictor()':>28}"]

    def rate(ts, w):
        r = sorted(w / x for x in ts)
        return f"{statistics.median(r):9.1f} ({r[0]:7.1f} .. {r[-1]:7.1f})"

    for overlap in (0.0, 0.5, 0.75):
        start = sp.plan_windows(n, overlap)
        W = start.size

        def slices():
            for w0 in range(0, W, a.batch):
                yield torch.from_numpy(np.stack([iq[s * p.hop:s * p.hop + p.n_samples] for s in start[w0:w0 + a.batch]]))

        def a_scan():
            for _img, _st in p.scan(iq, start, chunk_windows=a.batch):
                pass

        def a_old():
            for x in slices():
                p(x.to(dev))

        def b_scan():
            pred.scan(iq, 20e6, overlap=overlap, batch=a.batch, merge="ios")

        def b_old():
            for x in slices():
                pred(x)

        cols = [rate(timed(f), W) for f in (a_scan, a_old, b_scan, b_old)]
        lines.append(f"{overlap:8.2f} {W:8d} | {cols[0]:>28} {cols[1]:>28} | {cols[2]:>28} {cols[3]:>28}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
