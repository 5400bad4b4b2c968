"""Micro-benchmark of the IQ training loader: loader images / s for resident and staged sources at batch 64, 640^2 (L = 164 608),
with augmentation off and with everything on, and the gather / augment kernel's microseconds and GB / s on its own.

    python tools/iq_loader_micro.py [--batch 64] [--captures 8] [--windows 12] [--iters 30] [--out profiles/r06/iq_loader.txt]

Captures are synthetic noise written to a temporary folder (the loader's cost does not depend on the content)."""
import argparse
import random
import sys
import tempfile
import time
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "spectrogram-yolov11_amd"))

from sy11 import ops                                               # noqa: E402
from sy11.data.iq_augment import IQ_HYP                            # noqa: E402
from sy11.data.iq_dataset import IQDataLoader, IQDataset           # noqa: E402

ALL_ON = dict(iq_shift=0.25, iq_conj=0.5, iq_gain_db=6.0, iq_noise_db=10.0, iq_mixup=0.5)


def kernel_times(B, L, iters, lines):
    dev = torch.device("cuda")
    src = torch.view_as_complex(torch.randn(B * L + 4097, 2, device=dev))
    out = torch.empty((B, L), dtype=torch.complex64, device=dev)
    srcs, offs = [src] * B, [b * L + 1 for b in range(B)]
    cases = {"gather only": (ops.iq_recipes(B), None, 2),
             "shift + conj + gain": (ops.iq_recipes(B), None, 2),
             "everything (mix + noise)": (ops.iq_recipes(B), [src] * B, 3)}
    for name in ("shift + conj + gain", "everything (mix + noise)"):
        r = cases[name][0]
        r["dphi"], r["phi0"], r["gain"], r["flags"] = 0x0A3D70A4, 77, 1.3, 1
    r = cases["everything (mix + noise)"][0]
    r["sigma"], r["seed"], r["dphi2"], r["gain2"], r["off2"] = 0.5, 12345, 0xC0000123, 0.7, 33
    import ctypes as C
    from sy11._lib import call
    for name, (rec, partners, streams) in cases.items():
        rec = rec.copy()
        rec["src2"] = 0 if partners is None else src.data_ptr()
        table = np.concatenate([np.full(B, src.data_ptr(), np.uint64).view(np.uint8), np.array(offs, np.int64).view(np.uint8), rec.view(np.uint8)])
        t = torch.from_numpy(table).to(dev)
        args = (B, L, C.c_void_p(t.data_ptr()), C.c_void_p(t.data_ptr() + 8 * B), C.c_void_p(t.data_ptr() + 16 * B),
                C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        for _ in range(3):
            call("sy11_iq_gather_augment", *args)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):                                    # back-to-back launches between two events: the kernel alone
            call("sy11_iq_gather_augment", *args)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / iters
        lines.append(f"kernel  B={B} L={L}  {name:26s} {us:8.1f} us (mean of {iters} back-to-back launches)  "
                     f"{streams * B * L * 8 / us / 1e3:7.1f} GB/s over {streams} streams of {B * L * 8 / 1e6:.0f} MB")


def loader_rate(ds_dir, data, batch, hyp_kw, budget, iters):
    hyp = SimpleNamespace(**{**IQ_HYP, **hyp_kw, "iq_cache_bytes": budget})
    ds = IQDataset(str(ds_dir), data, imgsz=640, hyp=hyp, mode="train", batch_size=batch, device="cuda")
    dl = IQDataLoader(ds, batch, shuffle=True)
    it = dl._it
    for _ in range(3):
        next(it)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    for _ in range(iters):
        n += next(it)["iq"].shape[0]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ds.cache.close()
    return n / dt, dt / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--captures", type=int, default=8)
    ap.add_argument("--windows", type=int, default=12)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = 1024 + 639 * 256
    lines = [f"iq_loader_micro: batch {a.batch}, 640^2 (L = {L}), {a.captures} captures x {a.windows} windows, {torch.cuda.get_device_name(0)}"]
    kernel_times(a.batch, L, a.iters, lines)
    random.seed(0)
    with tempfile.TemporaryDirectory() as tmp:
        rng = np.random.default_rng(0)
        n = 1024 + (a.windows * 640 - 1) * 256
        for k in range(a.captures):
            x = rng.standard_normal(2 * n, dtype=np.float32)
            x.tofile(Path(tmp) / f"cap{k}.cf32")
            (Path(tmp) / f"cap{k}.txt").write_text(f"0 0.01 {n / 20e6 - 0.01!r} -4e6 -2e6\n1 0.2 0.3 1e6 5e6\n")
        data = {"sample_rate": 20e6, "center_freq": 0.0, "nc": 2}
        for src, budget in (("resident", 8 << 30), ("staged", 0)):
            for aug, kw in (("augmentation off", dict(iq_jitter=0.0)), ("everything on", ALL_ON)):
                rate, ms = loader_rate(tmp, data, a.batch, kw, budget, a.iters)
                lines.append(f"loader  {src:8s} {aug:16s} {rate:9.0f} img/s  ({ms:6.2f} ms per batch of {a.batch}, host recipes + read + launch)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
