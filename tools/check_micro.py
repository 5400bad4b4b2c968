"""Time the check launches of the two frame decoders on their own (``ops.fec_check``: sy11_fec_check; ``ops.ldpc_check``: sy11_ldpc_check; the corrector's is timed with its
decoder by tools/correct_micro.py) over FRAMES frames at the sizes tools/decode_micro.py and tools/ldpc_micro.py use: T = 1 024 and T = 8 192 trellis steps with a tail,
and the 12 x 24, Z = 81 code (N = 1 944, K = 972); random decided bits and soft bits, whitening on, crc16-ccitt-false.  Per workload one warm-up call, then REPS calls, each
between two events on the stream; the median is printed.  A call is the ``ops`` entry point: its host-side checks, the upload of the frame table and the kernel.  The rows
and data bytes of the first CHECK frames are compared with the numpy definition's (tests/_fec_ref.py).
Usage: check_micro.py [REPS [FRAMES [CHECK]]]"""
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "spectrogram-yolov11_amd"))
sys.path.insert(0, str(ROOT))
import numpy as np
import torch
from sy11 import ops
from sy11.data.decode import CRCS, FECFRAME
from tests import _fec_ref as R

dev = torch.device("cuda", 0)


def timed(call, reps):
    call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), min(ms), max(ms)


def main(reps=10, frames=4096, check=4):
    print(f"check launches of the frame decoders, {torch.cuda.get_device_name(0)}: {frames} frames, whitened, crc16-ccitt-false, {reps} calls after one warm-up, the median")
    spec = CRCS["crc16-ccitt-false"]
    for label, n_bits, n_info in (("fec_check, T = 1024", 2 * 1024, 1018), ("fec_check, T = 8192", 2 * 8192, 8186), ("ldpc_check, N = 1944", 1944, 972)):
        g = np.random.default_rng(n_bits)
        ldpc = label.startswith("ldpc")
        n_dec = n_bits if ldpc else n_bits // 2                                 # decided bits of a frame: the N of the codeword, or the T steps
        y = g.integers(-127, 128, (frames, n_bits)).astype(np.int8)
        y[g.random(y.shape) < 0.05] = 0                                          # erasures
        u = g.integers(0, 2, (frames, n_dec)).astype(np.uint8)
        w = g.integers(0, 2, n_info).astype(np.uint8)
        soft, bits, whiten = torch.from_numpy(y).to(dev), torch.from_numpy(np.packbits(u, axis=1)).to(dev), torch.from_numpy(w).to(dev)
        data = torch.zeros((frames, (n_info + 7) // 8), dtype=torch.uint8, device=dev)
        rows = torch.zeros((frames, 5), dtype=torch.int32, device=dev)
        if ldpc:
            at = np.arange(frames)
            call = lambda: ops.ldpc_check(soft, bits, at, n_bits, n_info, data, rows, whiten=whiten, crc=spec)                      # noqa: E731
        else:
            fr = np.zeros(frames, dtype=FECFRAME)
            fr["T"], fr["order"], fr["tail"], fr["row"], fr["scale"] = n_dec, 2, 1, np.arange(frames), 1.0
            call = lambda: ops.fec_check(soft, bits, fr, R.POLYS, n_info, data, rows, whiten=whiten, crc=spec)                      # noqa: E731
        t, lo, hi = timed(call, reps)
        h, d = rows.cpu().numpy(), data.cpu().numpy()
        same = True
        for k in range(min(check, frames)):
            v = u[k, :n_info] ^ w
            c = u[k] if ldpc else R.encode(u[k], tail=False)                     # what the signs of the soft bits are compared with
            calc, recv = R.crc(v[:n_info - 16], spec), int("".join(str(b) for b in v[n_info - 16:]), 2)
            want = [calc, recv, int(calc == recv), int(((y[k] != 0) & ((y[k] < 0) != c)).sum()), int((y[k] != 0).sum())]
            same = same and h[k].tolist() == want and np.array_equal(d[k], np.packbits(v))
        print(f"  {label}: {t:8.3f} ms (min {lo:.3f}, max {hi:.3f}) = {t / frames * 1e3:7.3f} us per frame;  the first {min(check, frames)} frames "
              f"{'equal' if same else 'DIFFER FROM'} numpy's")


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:]))
