"""Time the extraction (sy11_iq_extract, one launch per staged chunk) in clips per second and input samples per second, beside what a user
had to write before it existed: one ``plan_resample`` + one host-to-device copy of the box's own span + one ``ops.iq_resample`` per
detection.  Workload: a synthetic host capture of 2^LOG2N samples (default 24) and BOXES (default 1000) seeded boxes whose bandwidths
give D in {2, 8, 32} in equal shares, each 2^14 .. 2^16 input samples long, anywhere in the capture (so they overlap).  Both paths
start from the host array and end with all clips on the device; the two alternate, REPS times each, and the best and the median of
each are printed with the ratio of the medians; the outputs are compared bit for bit.
Usage: extract_micro.py [LOG2N [BOXES [REPS]]]"""
import statistics
import sys
import time
from fractions import Fraction
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "spectrogram-yolov11_amd"))
sys.path.insert(0, str(ROOT))
import numpy as np
import torch
from sy11 import ops
from sy11.data.extract import extract_capture, plan_extract, plan_extract_chunks, support
from sy11.data.resample import plan_resample

dev = torch.device("cuda", 0)
FS, FC = 61.44e6, 3.5e9


def boxes(n, k, seed=1):
    g = np.random.default_rng(seed)
    D = np.array([2, 8, 32])[np.arange(k) % 3]
    bw = 0.84 * FS / D / 1.2 * g.uniform(0.6, 0.95, k)                    # padded band within (0.5, 1] of the usable width: D as drawn
    length = g.integers(1 << 14, 1 << 16, k)
    start = g.integers(0, n - (1 << 16), k)
    centre = FC + g.uniform(-0.5, 0.5, k) * (FS - bw)
    return np.stack((start / FS, centre - bw / 2, (start + length) / FS, centre + bw / 2), 1), D


def per_detection(x, plan):
    """The parent commit's way: per box its own plan, its own copy of its own span, its own launch."""
    clips = []
    n = x.shape[0]
    for k in range(len(plan)):
        rp = plan_resample(FS, Fraction(FS) / int(plan.D[k]), plan.center_freq[k] - FC)
        m0, M = int(plan.m_first[k]), int(plan.M[k])
        a, b = rp.support(m0, m0 + M)
        a, b = max(a, 0), min(b, n)
        clips.append(ops.iq_resample(torch.from_numpy(x[a:b]).to(dev), rp, a, m0, M, n_total=n))
    return clips


def main(log2n=24, k=1000, reps=5):
    n = 1 << log2n
    g = np.random.default_rng(0)
    x = (g.standard_normal(n, dtype=np.float32) + 1j * g.standard_normal(n, dtype=np.float32)).astype(np.complex64) * np.float32(0.1)
    tf, D = boxes(n, k)
    plan = plan_extract(tf, n, FS, FC)
    assert plan.D.tolist() == D.tolist()
    chunks = plan_extract_chunks(plan, 1 << 24)
    read = sum(hi - lo for c in chunks for lo, hi in c.reads)
    each = sum(np.diff(support(plan.m_first[i], plan.M[i], plan.log2d[i], n))[0] for i in range(k))
    print(f"extract, {torch.cuda.get_device_name(0)}: capture of 2^{log2n} samples on the host, {k} boxes, D in {sorted(set(D.tolist()))}, "
          f"{plan.total} output samples; supports {each} samples box by box, {read} as their union; {len(chunks)} chunk(s)")
    got = extract_capture(x, plan, dev)                                     # warm-up of both paths, and the comparison
    want = per_detection(x, plan)
    torch.cuda.synchronize()
    same = all(torch.equal(torch.view_as_real(a), torch.view_as_real(b)) for a, b in zip(got.samples, want))
    t = {"batched": [], "per detection": []}
    for _ in range(reps):
        for name, fn in (("batched", lambda: extract_capture(x, plan, dev)), ("per detection", lambda: per_detection(x, plan))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t[name].append(time.perf_counter() - t0)
    for name, v in t.items():
        med = statistics.median(v)
        print(f"  {name:<14} best {min(v) * 1e3:9.2f} ms, median {med * 1e3:9.2f} ms of {reps}: {k / med:10.0f} clips/s, "
              f"{each / med / 1e6:9.1f} M input samples/s (box by box), {plan.total / med / 1e6:8.1f} M output samples/s")
    print(f"  ratio of the medians (per detection / batched): {statistics.median(t['per detection']) / statistics.median(t['batched']):.2f}; "
          f"outputs bit-identical: {same}")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)          # the launch alone, from a device capture
    xd = torch.from_numpy(x).to(dev)
    extract_capture(xd, plan, dev)
    e0.record()
    for _ in range(reps):
        extract_capture(xd, plan, dev)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    print(f"  device-resident capture (no copy): {ms:9.3f} ms per extraction = {each / ms / 1e3:9.1f} M input samples/s (box by box)")


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:4]))
