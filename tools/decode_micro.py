"""Time the Viterbi launch of the frame decoder (sy11_fec_viterbi: ONE launch over all frames, one wavefront per frame) and the numpy definition
(tests/_fec_ref.py, batched over the frames) on the same soft bits.  Workloads: 512 frames of T = 1 024 and 8 frames of T = 8 192 trellis steps,
with a tail, noisy codewords (sigma 0.7 per coded bit at soft_scale 32).  Per workload one warm-up call, then REPS calls, each between two events on
the stream; the median is printed.  A call is the library's entry point with the frame table already on the device: its host-side checks and
the kernel.  The decided bits, metrics and end states are compared with numpy's.
Usage: decode_micro.py [REPS]"""
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
from sy11.data.decode import FECFRAME
from tests import _fec_ref as R

dev = torch.device("cuda", 0)


def main(reps=10):
    print(f"frame decoder, launch 2, {torch.cuda.get_device_name(0)}: generators 171 133, tail, {reps} calls after one warm-up, the median")
    for n, T in ((512, 1024), (8, 8192)):
        g = np.random.default_rng(T)
        u = g.integers(0, 2, (n, T - 6))
        y = np.stack([R.quantize((1.0 - 2.0 * R.encode(u[k]).astype(np.float64)) + 0.7 * g.standard_normal(2 * T), 32.0) for k in range(n)])
        fr = np.zeros(n, dtype=FECFRAME)
        fr["T"], fr["order"], fr["tail"], fr["row"], fr["scale"] = T, 2, 1, np.arange(n), 1.0
        table = torch.from_numpy(fr.view(np.uint8)).to(dev)
        soft = torch.from_numpy(y).to(dev)
        bits = torch.zeros((n, T // 8), dtype=torch.uint8, device=dev)
        out = torch.zeros((n, 2), dtype=torch.int32, device=dev)
        p = lambda t: C.c_void_p(t.data_ptr())                                 # noqa: E731
        args = (n, C.c_void_p(fr.ctypes.data), p(table), R.POLYS[0], R.POLYS[1], n, 2 * T, p(soft), T // 8, p(bits), p(out), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        _lib.call("sy11_fec_viterbi", *args)
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.call("sy11_fec_viterbi", *args)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        t = float(np.median(ms))
        t0 = time.perf_counter()
        ru, rm, re = R.viterbi(y)
        t_np = (time.perf_counter() - t0) * 1e3
        h = out.cpu().numpy()
        same = np.array_equal(np.unpackbits(bits.cpu().numpy(), axis=1)[:, :T], ru) and np.array_equal(h[:, 0], rm) and np.array_equal(h[:, 1], re)
        wrong = int((ru[:, :T - 6] != u).sum())
        print(f"  {n:4d} frames of T = {T:5d}: {t:8.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}) = {n * T * 64 / t / 1e6:8.2f} G state steps/s, {t / n * 1e3:8.2f} us per frame;  "
              f"numpy {t_np:9.1f} ms: {t_np / t:7.1f} x;  bits, metrics and end states {'equal' if same else 'DIFFER FROM'} numpy's ({wrong} decoded bit errors)")


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:]))
