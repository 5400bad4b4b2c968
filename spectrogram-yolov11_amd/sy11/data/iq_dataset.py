"""Train and validate from labelled IQ captures (no reference counterpart: the reference's datasets are images).

Data YAML: the usual ``path`` / ``train`` / ``val`` / ``names`` | ``nc`` plus ``kind: iq``, ``sample_rate`` (Hz, required),
``center_freq`` (Hz, default 0) and optionally ``n_fft`` (1024) / ``hop`` (256); ``imgsz`` gives n_frames = n_mel.  ``train`` / ``val`` name
a folder, or a ``.txt`` list, of captures in the formats ``open_iq`` reads.  Each capture has a sidecar ``<stem>.txt`` of rows
``cls t0 t1 f_lo f_hi`` — seconds from the first sample, absolute Hz; a missing or empty sidecar is a background-only capture.

Windows: every capture is cut by ``plan_windows(len, overlap=0)`` (the end-aligned last window included).  ``mode="val"`` serves
exactly that grid; ``mode="train"`` has as many items, item i being grid slot i with its first frame jittered (``iq_augment``).

The house style of the image path, one level earlier: sources live in HBM (``IQSourceCache``), the host draws a recipe of a few
dozen bytes per sample, ONE launch (``ops.iq_gather_augment``) gathers and augments the batch, MixUp included, and the loader emits
``batch["iq"]`` (B, L) complex64 for ``DetectionTrainer.preprocess_batch`` / the validator to turn into images."""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

from .dataset import InfiniteDataLoader
from .iq_augment import IQ_HYP, Geometry, draw_recipe, pack_recipes
from .spectrogram import RAW_IQ_SUFFIXES, open_iq, plan_windows, read_samples

IQ_SUFFIXES = RAW_IQ_SUFFIXES + (".npy",)


def read_iq_sidecar(path, nc=None):
    """``<stem>.txt`` -> (n, 5) float64 rows cls t0 t1 f_lo f_hi.  Missing or empty: no rows.  Raises ValueError naming the file for a
    malformed row, t1 <= t0, f_hi <= f_lo, a class >= nc (or negative / fractional) or a non-finite value."""
    if not os.path.isfile(path):
        return np.zeros((0, 5), np.float64)
    with open(path) as f:
        lines = [x.split() for x in f.read().strip().splitlines() if x.strip()]
    if not lines:
        return np.zeros((0, 5), np.float64)
    try:
        rows = np.array(lines, dtype=np.float64)
    except ValueError:
        raise ValueError(f"{path}: every row must be five numbers `cls t0 t1 f_lo f_hi`") from None
    if rows.ndim != 2 or rows.shape[1] != 5:
        raise ValueError(f"{path}: every row must be five numbers `cls t0 t1 f_lo f_hi`, got {rows.shape[-1]} columns")
    if not np.isfinite(rows).all():
        raise ValueError(f"{path}: non-finite value in a label row")
    if (rows[:, 2] <= rows[:, 1]).any():
        raise ValueError(f"{path}: t1 <= t0 in a label row")
    if (rows[:, 4] <= rows[:, 3]).any():
        raise ValueError(f"{path}: f_hi <= f_lo in a label row")
    if (rows[:, 0] < 0).any() or (rows[:, 0] != np.floor(rows[:, 0])).any() or (nc is not None and (rows[:, 0] >= nc).any()):
        raise ValueError(f"{path}: class {rows[:, 0].max():g} is not an integer in [0, {nc})")
    return rows


def iq_files(path, prefix=""):
    """A folder (searched recursively) or a ``.txt`` list -> sorted capture files.  A folder's ``.txt`` sidecars are not captures."""
    f = []
    for p in path if isinstance(path, (list, tuple)) else [path]:
        p = Path(p)
        if p.is_dir():
            f += [str(x) for x in p.rglob("*") if x.suffix.lower() in IQ_SUFFIXES]
        elif p.is_file():
            parent = str(p.parent) + os.sep
            with open(p) as t:
                f += [x.replace("./", parent, 1) if x.startswith("./") else x for x in t.read().strip().splitlines() if x.strip()]
        else:
            raise FileNotFoundError(f"{prefix}{p} does not exist")
    f = sorted(f)
    if not f:
        raise FileNotFoundError(f"{prefix}no IQ captures ({' / '.join(IQ_SUFFIXES)}) found in {path}")
    return f


class IQSourceCache:
    """Where the kernel's sources live, next to the image path's HBM source cache.  Captures totalling at most ``budget`` bytes are
    uploaded ONCE and the kernel gathers straight from them (no host traffic per step).  Otherwise the windows of a batch are read
    with ``read_samples`` into one of TWO pinned staging buffers by a single background reader thread while the previous step runs
    (numpy's copies release the GIL), the buffer goes host -> device on a side stream guarded by an event, and the pointer table
    points into the device copy.  Both paths feed the same kernel with the same recipes, so they give identical bits."""

    def __init__(self, captures, n_samples, batch_size, device, budget):
        self.captures, self.L, self.device = captures, int(n_samples), torch.device(device)
        total = sum(len(c) for c in captures) * 8
        self.resident = total <= int(budget)
        if self.resident:
            self.dev = [torch.from_numpy(np.array(c, dtype=np.complex64)).to(self.device) for c in captures]
            return
        slots = 2 * int(batch_size)                                            # a window per sample and one per partner
        self.stage = [torch.empty((slots * self.L,), dtype=torch.complex64).pin_memory() for _ in range(2)]
        self.dev = [torch.empty((slots * self.L,), dtype=torch.complex64, device=self.device) for _ in range(2)]
        self.copied, self.used = [None, None], [None, None]                   # per buffer: H2D done; the kernel that read it done
        self.side = torch.cuda.Stream(self.device)
        self.reader = ThreadPoolExecutor(max_workers=1)                        # ONE reader: the disk is the bottleneck, not the CPUs
        self.turn = 0

    def _windows(self, recipes):
        return [(r.a.cap, r.a.first) for r in recipes] + [(r.b.cap, r.b.first) for r in recipes if r.b is not None]

    def _read(self, buf, wins):
        host = self.stage[buf].numpy()
        for j, (cap, first) in enumerate(wins):
            host[j * self.L:(j + 1) * self.L] = read_samples(self.captures[cap], first, first + self.L)

    def prefetch(self, recipes):
        """Start reading a coming batch's windows (staged sources); the ticket goes to ``sources``.  Resident: nothing to do."""
        if self.resident:
            return None
        wins = self._windows(recipes)
        if len(wins) * self.L > self.stage[0].numel():
            raise ValueError(f"IQSourceCache: a batch of {len(recipes)} samples exceeds the staging buffers")
        buf, self.turn = self.turn, self.turn ^ 1
        if self.copied[buf] is not None:
            self.copied[buf].synchronize()                                     # the pinned buffer is free once its last copy is done
        return buf, wins, self.reader.submit(self._read, buf, wins)

    def sources(self, recipes, ticket=None):
        """-> (srcs, offs, partners, partner offsets, done) for ``ops.iq_gather_augment``; call ``done()`` after the launch."""
        if self.resident:
            return ([self.dev[r.a.cap] for r in recipes], [r.a.first for r in recipes],
                    [None if r.b is None else self.dev[r.b.cap] for r in recipes], [0 if r.b is None else r.b.first for r in recipes],
                    lambda: None)
        buf, wins, fut = ticket if ticket is not None else self.prefetch(recipes)
        fut.result()
        main = torch.cuda.current_stream(self.device)
        n = len(wins) * self.L
        if self.used[buf] is not None:
            self.side.wait_event(self.used[buf])                               # the kernel that read this device buffer two batches ago
        with torch.cuda.stream(self.side):
            self.dev[buf][:n].copy_(self.stage[buf][:n], non_blocking=True)
            self.copied[buf] = torch.cuda.Event()
            self.copied[buf].record(self.side)
        main.wait_event(self.copied[buf])
        B, k = len(recipes), len(recipes)
        partners, poffs = [], []
        for r in recipes:
            partners.append(None if r.b is None else self.dev[buf])
            poffs.append(0 if r.b is None else k * self.L)
            k += r.b is not None

        def done():
            self.used[buf] = torch.cuda.Event()
            self.used[buf].record(main)
        return [self.dev[buf]] * B, [j * self.L for j in range(B)], partners, poffs, done

    def close(self):
        if not self.resident:
            self.reader.shutdown(wait=True)


class IQDataset:
    """Windows of labelled IQ captures.  ``__getitem__`` draws a recipe and maps the labels (host, microseconds); ``collate_fn``
    renders the batch with one launch."""

    rect = False

    def __init__(self, path, data, imgsz=640, hyp=None, mode="train", batch_size=16, device="cuda", fraction=1.0, prefix=""):
        if "sample_rate" not in data:
            raise SyntaxError("an IQ dataset needs 'sample_rate:' (Hz) in its data YAML")
        self.data, self.mode, self.augment, self.prefix = data, mode, mode == "train", prefix
        self.hyp = hyp if hyp is not None else SimpleNamespace(**IQ_HYP)
        for k, v in IQ_HYP.items():
            if not hasattr(self.hyp, k):
                setattr(self.hyp, k, v)
        self.imgsz, self.batch_size, self.device = int(imgsz), int(batch_size), torch.device(device)
        self.geometry = g = Geometry(float(data["sample_rate"]), float(data.get("center_freq", 0.0)), int(data.get("n_fft", 1024)),
                                     int(data.get("hop", 256)), self.imgsz, self.imgsz)
        self.files = iq_files(path, prefix)
        if fraction < 1:
            self.files = self.files[: max(round(len(self.files) * fraction), 1)]
        nc = len(data["names"]) if "names" in data else data.get("nc")
        self.captures = [open_iq(f) for f in self.files]
        self.rows = [read_iq_sidecar(str(Path(f).with_suffix(".txt")), nc) for f in self.files]
        self.items, self.last_frame = [], []
        for i, (f, c) in enumerate(zip(self.files, self.captures)):
            try:
                start = plan_windows(len(c), overlap=0, n_fft=g.n_fft, hop=g.hop, n_frames=g.n_frames)
            except ValueError as e:
                raise ValueError(f"{f}: shorter than one window ({e})") from None
            self.items += [(i, int(s)) for s in start]
            self.last_frame.append(int(start[-1]))
        self.cache = None

    def __len__(self):
        return len(self.items)

    def __getitem__(self, index):
        return draw_recipe(self, index)

    def close_mosaic(self, hyp):
        """The last epochs train on single windows, as image MixUp is switched off with the mosaic (dataset.py:197-202)."""
        hyp.iq_mixup = 0.0
        self.hyp = hyp

    def source_cache(self):
        if self.cache is None:
            self.cache = IQSourceCache(self.captures, self.geometry.n_samples, self.batch_size, self.device, self.hyp.iq_cache_bytes)
        return self.cache

    def collate_fn(self, recipes, out=None, dtype=None, ticket=None):
        """[IQRecipe] -> {"iq": (B, L) complex64 on the device, "batch_idx", "cls", "bboxes"} (the label keys as ``YOLODataset.collate_fn``
        emits them).  ``out`` / ``dtype`` belong to the image loaders' interface and do not apply: the image is produced later, from
        ``batch["iq"]``, straight into the graph's static input."""
        from .. import ops as K
        cache = self.source_cache()
        srcs, offs, partners, poffs, done = cache.sources(recipes, ticket)
        rec = pack_recipes(recipes)
        rec["off2"] = poffs
        iq = K.iq_gather_augment(srcs, offs, self.geometry.n_samples, rec, partners)
        done()
        return {"iq": iq, **collate_labels(recipes)}


def collate_labels(recipes):
    lb = [torch.from_numpy(r.labels) for r in recipes]
    return {"batch_idx": torch.cat([torch.full((len(x),), float(i)) for i, x in enumerate(lb)], 0),
            "cls": torch.cat([x[:, 0:1] for x in lb], 0), "bboxes": torch.cat([x[:, 1:5] for x in lb], 0)}


class IQDataLoader(InfiniteDataLoader):
    """``InfiniteDataLoader`` (same sampler: seeded shuffle, strided DDP shard) over an ``IQDataset``.  The recipes stay in the
    training process — the host cost is a few microseconds per sample — and the batch after the one being served is drawn one step
    early so that staged sources are read in the background while the current step runs.  Nothing is drawn across an epoch boundary
    (``close_mosaic`` takes effect with the first batch of its epoch)."""

    def __init__(self, dataset, batch_size, shuffle=True, rank=-1, world_size=1, seed=0):
        super().__init__(dataset, batch_size, shuffle=shuffle, rank=rank, world_size=world_size, seed=seed, prefetch=0)

    def _draw(self, indices):
        recipes = [self.dataset[i] for i in indices]
        return recipes, (self.dataset.source_cache().prefetch(recipes) if self.dataset.device.type == "cuda" else None)

    def _forever(self):
        while True:
            idx = self._epoch_indices()
            batches = [idx[i:i + self.batch_size] for i in range(0, len(idx), self.batch_size)]
            cur = self._draw(batches[0])
            for k in range(len(batches)):
                nxt = self._draw(batches[k + 1]) if k + 1 < len(batches) else None
                yield self.dataset.collate_fn(cur[0], ticket=cur[1])
                cur = nxt
            self.epoch += 1


def build_iq_dataset(cfg, path, batch, data, mode="train", device="cuda"):
    return IQDataset(path, data, imgsz=cfg.imgsz, hyp=cfg, mode=mode, batch_size=batch, device=device,
                     fraction=getattr(cfg, "fraction", 1.0) if mode == "train" else 1.0, prefix=f"{mode}: ")
