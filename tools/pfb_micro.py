"""Time the polyphase filter bank kernel (sy11_iq_channelize) in input samples per second beside the per-band route that produces
the same rows (K - 1 launches of sy11_iq_resample with ``plan.ddc_plan(k)`` on the same device tensor), and a channelised scan beside
the same bands scanned one ``tune_to`` at a time.  Usage: pfb_micro.py [log2 of the input length]"""
import sys
import time
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "spectrogram-yolov11_amd"))
sys.path.insert(0, str(ROOT))
import torch
from sy11 import ops
from sy11.data.channelize import plan_channels

dev = torch.device("cuda", 0)
FS_IN = 160e6


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


def kernels(log2n):
    n = 1 << log2n
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.view_as_complex(torch.randn(n, 2, generator=g, device=dev))
    print(f"pfb kernel, {n} input samples (2^{log2n}), {torch.cuda.get_device_name(0)}")
    print(f"{'K':>3} {'r':>2} {'D':>3} {'N':>5} {'bank ms':>9} {'MS/s in':>9} {'GB/s':>7} {'K-1 DDC ms':>11} {'MS/s in':>9} {'ratio':>7} {'max diff':>9}")
    for K in (4, 16, 64):
        for r in (2, 1):
            plan = plan_channels(FS_IN, K, r)
            M = plan.n_out(n)
            out = torch.empty((K, M), dtype=torch.complex64, device=dev)
            t_b = timed(lambda: ops.iq_channelize(x, plan, 0, 0, M, out=out))
            bands = plan.default_select()
            ddc = [plan.ddc_plan(k) for k in bands]
            row = torch.empty((M,), dtype=torch.complex64, device=dev)

            def per_band():
                for d in ddc:
                    ops.iq_resample(x, d, 0, 0, M, out=row)
            t_d = timed(per_band, reps=3, warm=1)
            diff = max((ops.iq_resample(x, d, 0, 0, M) - out[k]).abs().max().item() for k, d in zip(bands, ddc))
            gbs = 8.0 * (n + K * M) / t_b / 1e9
            print(f"{K:>3} {r:>2} {plan.D:>3} {plan.N:>5} {t_b * 1e3:>9.3f} {n / t_b / 1e6:>9.0f} {gbs:>7.0f} {t_d * 1e3:>11.3f} "
                  f"{n / t_d / 1e6:>9.0f} {t_d / t_b:>7.1f} {diff:>9.1e}")


def scans():
    from sy11.data.spectrogram import SpectrogramProducer, open_iq
    from sy11.engine.predictor import DetectionPredictor
    from sy11.nn.tasks import DetectionModel
    torch.manual_seed(0)
    m = DetectionModel("yolo11n.yaml", nc=2, verbose=False)
    m.names = {0: "a", 1: "b"}
    pred = DetectionPredictor(m, device=dev, conf=0.25, iou=0.7, producer=SpectrogramProducer(dev))
    K, fc = 16, 2.4e9
    plan = plan_channels(FS_IN, K, 2)
    n_out = 1024 + (8 * 640 - 1) * 256                                      # 8 windows per band at overlap 0
    n_in = n_out * plan.D
    x = (torch.randn(n_in, dtype=torch.complex64) * 0.1).numpy()
    bands = plan.default_select()
    print(f"scan of {n_in / FS_IN * 1e3:.1f} ms at {FS_IN / 1e6} MS/s, {len(bands)} bands of {plan.fs_out / 1e6} MS/s, 8 windows per band, "
          f"batch 64, host array source:")

    def bank():
        return pred.scan(open_iq(x), FS_IN, fc, overlap=0.0, batch=64, channels=plan)

    def per_band():
        return [pred.scan(open_iq(x), FS_IN, fc, overlap=0.0, batch=64, resample_to=plan.ddc_plan(k)) for k in bands]
    best = {}
    for name, fn in (("channelised (one read)", bank), ("one tune_to scan per band", per_band)):
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best[name] = dt if name not in best else min(best[name], dt)
        print(f"  {name:<28} {best[name] * 1e3:8.1f} ms = {n_in / best[name] / 1e6:7.1f} MS/s in, {(n_in / FS_IN) / best[name]:5.2f} x real time")
    a, b = best.values()
    print(f"  ratio {b / a:.2f}")


if __name__ == "__main__":
    kernels(int(sys.argv[1]) if len(sys.argv) > 1 else 23)
    scans()
