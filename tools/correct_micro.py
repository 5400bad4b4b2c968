"""Time the two launches of the frame corrector (sy11_rs_decode: one wavefront per codeword; sy11_rs_check: one workgroup per frame) and the numpy / Python
reference (tests/_rs_ref.py) on the same rows.  Workload: 4 096 frames of I = 4 interleaved ccsds-255-223 codewords (1 020 bytes a frame, the CCSDS frame
that fills T_MAX), with 0, 8 and 16 byte errors in every codeword and a crc32 over each frame's information.  Per workload one warm-up pair, then REPS
pairs, each pair between two events on the stream; the median is printed.  A call is the library's entry point with the row table already on the
device: its host-side checks and the kernel.  The reference decodes word by word in Python, at milliseconds a word: it is timed on the first
REF_FRAMES frames, whose results are compared with the device's, and that time is ALSO given scaled to all frames, named as a scaling.
Usage: correct_micro.py [REPS [REF_FRAMES]]"""
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
from sy11.data.decode import CRCS
from tests import _rs_ref as R

dev = torch.device("cuda", 0)


def main(reps=20, ref_frames=64, frames=4096):
    cd, I = R.CODES["ccsds-255-223"], 4
    n, k = cd["n"], cd["k"]
    print(f"frame corrector, both launches, {torch.cuda.get_device_name(0)}: {frames} frames x {I} x RS({n}, {k}), crc32, {reps} pairs after one warm-up, the median")
    code = _lib.RsCode(n, k, cd["fcr"], cd["prim"], I, cd["poly"])
    c32 = CRCS["crc32"]
    crc = _lib.FecCrc(c32["width"], c32["poly"], c32["init"], c32["xorout"], int(c32["refin"]), int(c32["refout"]))
    for errors in (0, 8, 16):
        g = np.random.default_rng(errors)
        sent = R.encode(g.integers(0, 256, (frames * I, k)), cd)
        rx = sent.copy()
        for w in range(frames * I):
            at = g.choice(n, errors, replace=False)
            rx[w, at] ^= g.integers(1, 256, errors).astype(np.uint8)
        data_h = np.stack([R.interleave(rx[f * I:(f + 1) * I]) for f in range(frames)])
        row = np.arange(frames, dtype=np.int32)
        table, data = torch.from_numpy(row).to(dev), torch.from_numpy(data_h).to(dev)
        info = torch.zeros((frames, I * k), dtype=torch.uint8, device=dev)
        cw = torch.zeros((frames, I, 2), dtype=torch.int32, device=dev)
        rows = torch.zeros((frames, 6), dtype=torch.int32, device=dev)
        p = lambda t: C.c_void_p(t.data_ptr())                                 # noqa: E731
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        a1 = (frames, C.c_void_p(row.ctypes.data), p(table), C.byref(code), 0, frames, I * n, p(data), I * k, p(info), p(cw), stream)
        a2 = (frames, C.c_void_p(row.ctypes.data), p(table), C.byref(code), C.byref(crc), frames, I * k, p(info), p(cw), p(rows), stream)
        _lib.call("sy11_rs_decode", *a1)
        _lib.call("sy11_rs_check", *a2)
        torch.cuda.synchronize()
        both, first = [], []
        for _ in range(reps):
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record()
            _lib.call("sy11_rs_decode", *a1)
            e1.record()
            _lib.call("sy11_rs_check", *a2)
            e2.record()
            torch.cuda.synchronize()
            both.append(e0.elapsed_time(e2)), first.append(e0.elapsed_time(e1))
        t, t1 = float(np.median(both)), float(np.median(first))
        t0 = time.perf_counter()
        ri, rc = R.correct_rows(data_h, np.arange(ref_frames), cd, I, 0)
        t_ref = (time.perf_counter() - t0) * 1e3
        hi, hc = info.cpu().numpy(), cw.cpu().numpy()
        same = np.array_equal(hi[:ref_frames], ri) and np.array_equal(hc[:ref_frames], rc)
        exact = np.array_equal(hi.reshape(-1, k), sent[:, :k]) and bool((hc[:, :, 0] == errors).all()) and bool((rows.cpu().numpy()[:, 0] == 0).all())
        print(f"  {errors:2d} errors a codeword: {t:8.3f} ms (min {min(both):.3f}, max {max(both):.3f}), of which launch 1 {t1:8.3f} ms = {t1 / (frames * I) * 1e3:7.3f} us per codeword, "
              f"{frames * I * n / t / 1e6:8.2f} GB/s of received bytes;  reference {t_ref:9.1f} ms for the first {ref_frames} frames (scaled to all: {t_ref * frames / ref_frames:10.0f} ms, "
              f"{t_ref * frames / ref_frames / t:9.0f} x);  those frames {'equal' if same else 'DIFFER FROM'} the reference's, all frames {'are' if exact else 'ARE NOT'} what was sent")


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:]))
