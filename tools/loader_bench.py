"""Loader throughput with and without worker processes, alone and feeding a yolo11s f16 training step (files on tmpfs).
   python tools/loader_bench.py [procs ...] [--mixup P] [--no-train] [--n FILES] [--root DIR] [--pkg DIR] [--profile]
   (default procs: 0 4 8).  --mixup P: hyp.mixup of the training dataset.  --no-train: the loader alone, no model.  --root DIR:
   keep / reuse the synthetic dataset there (several runs over the same files).  --pkg DIR: import sy11 from another checkout's
   package directory (A/B of two builds in one session)."""
import sys, tempfile, time
from pathlib import Path
from types import SimpleNamespace
ROOT = Path(__file__).resolve().parents[1]


def _opt(name, default, cast):
    if name in sys.argv:
        i = sys.argv.index(name)
        v = cast(sys.argv[i + 1])
        del sys.argv[i:i + 2]
        return v
    return default


MIXUP, NFILES, DATA_ROOT, PKG = _opt("--mixup", 0.0, float), _opt("--n", 1024, int), _opt("--root", None, str), _opt("--pkg", None, str)
sys.path.insert(0, PKG or str(ROOT / "spectrogram-yolov11_amd"))
import numpy as np
import torch


def main():
    import sy11
    from sy11.data.dataset import DEFAULT_HYP, YOLODataset, build_dataloader
    S, B, n = 640, 64, NFILES
    g = np.random.default_rng(0)
    root = Path(DATA_ROOT) if DATA_ROOT else Path(tempfile.mkdtemp()) / "d"
    if not (root / "images").exists():
        (root / "images").mkdir(parents=True); (root / "labels").mkdir()
        for i in range(n):
            np.save(root / "images" / f"s{i:04d}.npy", g.integers(0, 256, (S, S, 3), dtype=np.uint8))
            rows = np.concatenate((g.integers(0, 2, (4, 1)), g.uniform(0.3, 0.7, (4, 2)), g.uniform(0.05, 0.3, (4, 2))), 1)
            (root / "labels" / f"s{i:04d}.txt").write_text("\n".join(" ".join(f"{v:.6f}" for v in r) for r in rows))
    procs = [int(a) for a in sys.argv[1:] if not a.startswith('-')] or [0, 4, 8]
    train = "--no-train" not in sys.argv
    tag = f"{Path(sy11.__file__).resolve().parents[2].name} mixup {MIXUP:g} "
    if train:
        from sy11.engine.trainer import DetectionTrainer
        from sy11.nn.tasks import DetectionModel
        model = DetectionModel("yolo11s.yaml", nc=2, verbose=False)
        tr = DetectionTrainer(model, batch_size=B, device="cuda", overrides={"amp": True}, graphs=True)
    for p in procs:
        ds = YOLODataset(str(root / "images"), imgsz=S, augment=True, batch_size=B, data={"nc": 2},
                         hyp=SimpleNamespace(**{**DEFAULT_HYP, "mixup": MIXUP}))
        static = torch.empty((B, 3, S, S), device="cuda")
        dl = build_dataloader(ds, B, workers=8, out=static, dtype=torch.float32, procs=p)
        it = iter(dl)
        for _ in range(3):
            next(dl._it)
        torch.cuda.synchronize(); t0 = time.perf_counter(); nb = 0
        import cProfile, pstats, io
        pr = cProfile.Profile()
        if "--profile" in sys.argv: pr.enable()
        for _ in range(2):
            for batch in dl:
                nb += 1
        if "--profile" in sys.argv:
            pr.disable()
            buf = io.StringIO(); pstats.Stats(pr, stream=buf).sort_stats("tottime").print_stats(18)
            print("\n".join(l[:160] for l in buf.getvalue().splitlines() if l.strip())[:4000])
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        alone = nb * B / dt
        if not train:
            print(f"{tag}procs {p}: loader alone {alone:7.0f} img/s ({nb} batches of {B})", flush=True)
            if hasattr(dl, "close"):
                dl.close()
            continue
        dl.out = tr.batch_buffer(S)
        for _ in range(5):
            tr.train_step(next(dl._it))
        torch.cuda.synchronize(); t0 = time.perf_counter(); nb = 0
        for _ in range(3):
            for batch in dl:
                tr.train_step(batch); nb += 1
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        print(f"{tag}procs {p}: loader alone {alone:7.0f} img/s; training from files {nb * B / dt:7.0f} img/s ({dt / nb * 1e3:.1f} ms/step)", flush=True)
        if hasattr(dl, "close"):
            dl.close()


if __name__ == "__main__":
    main()
