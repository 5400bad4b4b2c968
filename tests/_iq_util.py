"""Shared by the IQ dataset tests: four small labelled captures (noise plus chirped bursts of known extent) written to a folder from
a seeded numpy generator, in the accuracy gate's geometry (imgsz 320, n_fft 512, hop 128), with a data YAML."""
import numpy as np

SR, FC, N_FFT, HOP, IMGSZ = 1.0e6, 100.0e6, 512, 128, 320
L = N_FFT + (IMGSZ - 1) * HOP                        # 41 344 samples per window
# name, samples (2 - 3 windows each: exact grid / end-aligned last window / odd length), bursts (cls t0 t1 f_lo f_hi; absolute Hz)
CAPTURES = (
    ("a.npy", N_FFT + (2 * IMGSZ - 1) * HOP, ((0, 0.010, 0.030, FC + 0.10e6, FC + 0.20e6), (1, 0.050, 0.075, FC - 0.30e6, FC - 0.22e6))),
    ("b.cf32", 100000, ((1, 0.020, 0.060, FC - 0.05e6, FC + 0.05e6),)),
    ("c.npy", N_FFT + (3 * IMGSZ - 1) * HOP, ((0, 0.005, 0.020, FC + 0.30e6, FC + 0.38e6), (0, 0.090, 0.115, FC - 0.15e6, FC - 0.05e6),
                                              (1, 0.040, 0.070, FC + 0.02e6, FC + 0.12e6))),
    ("d.cf32", 90001, ()),                           # background only: no sidecar at all
)


def make_capture(n, bursts, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.05
    t = np.arange(n) / SR
    for _, t0, t1, f_lo, f_hi in bursts:
        i0, i1 = int(round(t0 * SR)), min(int(round(t1 * SR)), n)
        tt = t[i0:i1] - t0
        f0, rate = f_lo - FC, (f_hi - f_lo) / (t1 - t0)                       # a chirp that fills the labelled band
        x[i0:i1] += np.exp(2j * np.pi * (f0 * tt + 0.5 * rate * tt * tt))
    return x.astype(np.complex64)


def write_dataset(root, extra_yaml=""):
    """-> (yaml path, [capture arrays]) with train = val = root / "iq"."""
    d = root / "iq"
    d.mkdir(parents=True, exist_ok=True)
    caps = []
    for k, (name, n, bursts) in enumerate(CAPTURES):
        x = make_capture(n, bursts, 100 + k)
        caps.append(x)
        if name.endswith(".npy"):
            np.save(d / name, x)
        else:
            x.view(np.float32).tofile(d / name)
        if bursts:
            (d / name).with_suffix(".txt").write_text("".join(f"{c} {t0!r} {t1!r} {a!r} {b!r}\n" for c, t0, t1, a, b in bursts))
    y = root / "iq.yaml"
    y.write_text(f"path: {root}\ntrain: iq\nval: iq\nkind: iq\nsample_rate: {SR}\ncenter_freq: {FC}\nn_fft: {N_FFT}\nhop: {HOP}\n"
                 f"names:\n  0: chirp_up\n  1: chirp_wide\n{extra_yaml}")
    return y, caps
