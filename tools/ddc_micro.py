"""Time the DDC kernel (sy11_iq_resample) in input samples per second for a set of ratios, beside a plain-torch baseline (complex
mixer + one strided conv1d per polyphase row), and a scan with and without resampling.  Usage: ddc_micro.py [log2 of the input length]"""
import sys
import time
from fractions import Fraction
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "spectrogram-yolov11_amd"))
sys.path.insert(0, str(ROOT))
import torch
import torch.nn.functional as F
from sy11 import ops
from sy11.data.resample import plan_resample

dev = torch.device("cuda", 0)
RATIOS = [(1, 2), (2, 3), (3, 2), (5, 16), (125, 192), (1, 8), (4, 1), (25, 64), (1, 1)]
FS_IN = 61.44e6


def timed(fn, reps=10, warm=2):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3


def torch_ddc(x, plan, M):
    """The same outputs with torch alone: mixer in complex64, then for every residue m_s of m mod P one conv1d with stride Q of the
    (real, imag) pair against that residue's polyphase row."""
    n = x.shape[0]
    if plan.dphi:
        i = torch.arange(n, device=x.device, dtype=torch.int64)
        ph = ((i * plan.dphi) & 0xFFFFFFFF).to(torch.float64) / 2.0 ** 32
        x = x * torch.polar(torch.ones_like(ph), 2 * torch.pi * ph).to(torch.complex64)
    if not plan.filters:
        return x[:M]
    P, Q, T, c = plan.P, plan.Q, plan.T, plan.c
    taps = plan.taps_on(x.device)
    last = ((M - 1) * Q + c) // P
    xp = F.pad(torch.view_as_real(x).T.contiguous(), (T - 1, max(last + 1 - n, 0)))[:, None, :]          # (2, 1, T - 1 + n + ...)
    y = torch.empty((M,), dtype=torch.complex64, device=x.device)
    yr = torch.view_as_real(y)
    for ms in range(min(P, M)):
        q = ms * Q + c
        cnt = (M - 1 - ms) // P + 1
        seg = xp[:, :, q // P:q // P + (cnt - 1) * Q + T]                  # padded index of sample i is i + T - 1
        out = F.conv1d(seg, taps[q % P].flip(0)[None, None, :], stride=Q)  # (2, 1, cnt)
        yr[ms::P] = out[:, 0, :].T
    return y


def kernels(log2n):
    n = 1 << log2n
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.view_as_complex(torch.randn(n, 2, generator=g, device=dev))
    print(f"ddc kernel, {n} input samples (2^{log2n}), {torch.cuda.get_device_name(0)}")
    print(f"{'P/Q':>8} {'T':>5} {'mixer':>6} {'kernel ms':>10} {'MS/s in':>9} {'torch ms':>9} {'MS/s in':>9} {'speed-up':>8} {'max diff':>9}")
    for P, Q in RATIOS:
        for shift in (0.0, 1.0e6):
            if P == Q and shift == 0.0:
                continue                                                   # the identity: no launch
            plan = plan_resample(FS_IN, Fraction(FS_IN) * P / Q, shift)
            M = plan.n_out(n)
            out = torch.empty((M,), dtype=torch.complex64, device=dev)
            t_k = timed(lambda: ops.iq_resample(x, plan, 0, 0, M, out=out))
            if P > 32:                                                     # one conv1d shape per row: the baseline's set-up alone takes minutes
                print(f"{P:>4}/{Q:<3} {plan.T:>5} {'on' if plan.dphi else 'off':>6} {t_k * 1e3:>10.3f} {n / t_k / 1e6:>9.0f} {'-':>9} {'-':>9} {'-':>8} {'-':>9}")
                continue
            t_t = timed(lambda: torch_ddc(x, plan, M), reps=3, warm=1)
            diff = (torch_ddc(x, plan, M) - out).abs().max().item()
            print(f"{P:>4}/{Q:<3} {plan.T:>5} {'on' if plan.dphi else 'off':>6} {t_k * 1e3:>10.3f} {n / t_k / 1e6:>9.0f} {t_t * 1e3:>9.2f} "
                  f"{n / t_t / 1e6:>9.0f} {t_t / t_k:>8.1f} {diff:>9.1e}")


def scans():
    from sy11.data.spectrogram import SpectrogramProducer, open_iq
    from sy11.engine.predictor import DetectionPredictor
    from sy11.nn.tasks import DetectionModel
    torch.manual_seed(0)
    m = DetectionModel("yolo11n.yaml", nc=2, verbose=False)
    m.names = {0: "a", 1: "b"}
    pred = DetectionPredictor(m, device=dev, conf=0.25, iou=0.7, producer=SpectrogramProducer(dev))
    fs = 15.36e6
    n_out = 1024 + (64 * 640 - 1) * 256                                     # 64 windows at overlap 0
    y = (torch.randn(n_out, dtype=torch.complex64) * 0.1).numpy()
    print(f"scan of {n_out / fs:.3f} s at {fs / 1e6} MS/s (64 windows, batch 64, host array source):")
    for name, fs_in, kw in (("as recorded", fs, {}), ("from 4x the rate, retuned", 4 * fs, {"resample_to": fs, "tune_to": 3.5e9 + 10e6}),
                            ("from 5/4 the rate", fs * 5 / 4, {"resample_to": fs})):
        n_in = int(n_out * fs_in / fs)
        x = y if fs_in == fs else (torch.randn(n_in, dtype=torch.complex64) * 0.1).numpy()
        best = None
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pred.scan(open_iq(x), fs_in, 3.5e9, overlap=0.0, batch=64, **kw)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        print(f"  {name:<28} {n_in:>10} input samples: {best * 1e3:8.1f} ms = {n_in / best / 1e6:7.1f} MS/s in, "
              f"{(n_in / fs_in) / best:5.2f} x real time")


if __name__ == "__main__":
    kernels(int(sys.argv[1]) if len(sys.argv) > 1 else 23)
    scans()
