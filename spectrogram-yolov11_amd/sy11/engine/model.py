"""The reference's front door (`from ultralytics import YOLO`: engine/model.py Model :23-1150, models/yolo/model.py YOLO
:12-50) for the detection path this build carries: ``YOLO("yolo11s.yaml" | "weights.pt")`` with ``train`` / ``val`` /
``predict`` / ``__call__`` / ``load`` / ``save`` / ``fuse`` / ``info``, wired to the sy11 trainer, validator and
predictor.  Only what those entry points need of the reference's configuration machinery is here: the dataset YAML rules of
``check_det_dataset`` (data/utils.py:300-373: `train` / `val` required, `names` or `nc`, paths relative to `path` or to
the YAML's folder) and the keyword overrides that map onto this build's trainer arguments.  Everything else the
reference's ``Model`` offers (export, tune, track, benchmark, HUB, callbacks) is out of scope."""
from __future__ import annotations

import os

import random
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

from ..nn.tasks import DetectionModel
from .checkpoint import attempt_load_one_weight, save_checkpoint

_TRAIN_KEYS = {"lr0", "momentum", "weight_decay", "nbs", "box", "cls", "dfl", "amp", "optimizer", "warmup_epochs", "warmup_momentum",
               "warmup_bias_lr", "multi_scale", "imgsz", "deterministic"}


def check_det_dataset(data):
    """data/utils.py:300-373 without downloads: a dict or a YAML path -> dict with absolute `train` / `val`, `names`, `nc`."""
    if not isinstance(data, dict):
        import yaml
        yaml_file = Path(data)
        with open(yaml_file, errors="ignore", encoding="utf-8") as f:
            data = yaml.safe_load(f) or {}
        data["yaml_file"] = str(yaml_file)
    data = dict(data)
    for k in ("train", "val"):
        if k not in data:
            if k != "val" or "validation" not in data:
                raise SyntaxError(f"'{k}:' key missing. 'train' and 'val' are required in all data YAMLs.")
            data["val"] = data.pop("validation")
    if "names" not in data and "nc" not in data:
        raise SyntaxError("either 'names' or 'nc' are required in all data YAMLs.")
    if "names" in data and "nc" in data and len(data["names"]) != data["nc"]:
        raise SyntaxError(f"'names' length {len(data['names'])} and 'nc: {data['nc']}' must match.")
    if "names" not in data:
        data["names"] = [f"class_{i}" for i in range(data["nc"])]
    else:
        data["nc"] = len(data["names"])
    if isinstance(data["names"], (list, tuple)):
        data["names"] = dict(enumerate(data["names"]))
    data["names"] = {int(k): str(v) for k, v in data["names"].items()}
    yaml_dir = Path(data["yaml_file"]).resolve().parent if data.get("yaml_file") else Path.cwd()
    root = Path(data.get("path") or yaml_dir)
    if not root.is_absolute():                               # the reference anchors a relative `path` at its global datasets dir;
        root = (yaml_dir / root).resolve()                   # without that setting the YAML's own folder is the only sensible anchor
    data["path"] = root
    for k in ("train", "val", "test"):
        if data.get(k):
            x = data[k]
            data[k] = str((root / x).resolve()) if isinstance(x, str) else [str((root / v).resolve()) for v in x]
    if "kind" in data:                                       # `kind: iq` — labelled IQ captures (sy11/data/iq_dataset.py); no key: images
        if data["kind"] != "iq":
            raise SyntaxError(f"'kind: {data['kind']}' is not a dataset kind (only 'iq'; leave the key out for images)")
        if "sample_rate" not in data:
            raise SyntaxError("'sample_rate:' (Hz) is required in a 'kind: iq' data YAML")
        data["sample_rate"], data["center_freq"] = float(data["sample_rate"]), float(data.get("center_freq", 0.0))
        data["n_fft"], data["hop"] = int(data.get("n_fft", 1024)), int(data.get("hop", 256))
        if not (data["sample_rate"] > 0 and np.isfinite(data["center_freq"])) or data["n_fft"] < 2 or data["hop"] < 1:
            raise SyntaxError("'sample_rate' must be positive, 'center_freq' finite, 'n_fft' >= 2 and 'hop' >= 1")
    return data


def _iq_setup(data, imgsz, overrides, dev):
    """What a `kind: iq` run needs besides the dataset: the producer that turns batch["iq"] into images, after refusing the settings
    that belong to the image path (every image augmentation counts as off for IQ; naming one with a value that would switch it on
    is an error, as `perspective` is for the image transforms)."""
    from ..data.dataset import DEFAULT_HYP
    from ..data.spectrogram import SpectrogramProducer
    bad = sorted(k for k in overrides if (k in DEFAULT_HYP or k in ("rect", "multi_scale")) and overrides[k] and k not in ("mask_ratio", "overlap_mask"))
    if bad:
        raise ValueError(f"{bad} do(es) not apply to a 'kind: iq' dataset (IQ augmentation is iq_shift / iq_conj / iq_gain_db / iq_noise_db / iq_mixup)")
    if not isinstance(imgsz, int):
        raise ValueError("a 'kind: iq' dataset needs a square integer imgsz (n_frames = n_mel = imgsz)")
    return SpectrogramProducer(dev, data["n_fft"], data["hop"], imgsz, imgsz)


class YOLO:
    """models/yolo/model.py:12 / engine/model.py:23 for task="detect"."""

    def __init__(self, model="yolo11n.yaml", task="detect", verbose=False, device="cuda", nc=None):
        if task not in (None, "detect"):
            raise NotImplementedError("sy11 carries the detection task only")
        self.task, self.device = "detect", torch.device(device)
        self.ckpt, self.trainer, self.predictor, self.metrics = None, None, None, None
        self.overrides = {}
        name = str(model)
        if name.endswith((".yaml", ".yml")):
            self.model = DetectionModel(name, nc=nc, verbose=verbose) if nc else DetectionModel(name, verbose=verbose)
            self.cfg = name
        else:
            self.model, self.ckpt = attempt_load_one_weight(name, device=self.device)
            self.cfg = getattr(self.model, "yaml_file", None)
        self.model_name = name

    # ---- bookkeeping of the reference's Model
    @property
    def names(self):
        return getattr(self.model, "names", None)

    def info(self, detailed=False, verbose=True):
        return self.model.info(detailed=detailed, verbose=verbose)

    def fuse(self):
        self.model.fuse()
        return self

    def load(self, weights):
        """engine/model.py:326-350 — take matching weights from a checkpoint / state_dict (class count may differ)."""
        src = attempt_load_one_weight(weights, device=self.device)[0].state_dict() if isinstance(weights, (str, Path)) else weights
        own = self.model.state_dict()
        ok = {k: v for k, v in src.items() if k in own and own[k].shape == v.shape}
        self.model.load_state_dict(ok, strict=False)
        return self

    def save(self, filename="saved_model.pt"):
        save_checkpoint(filename, ema_model=self.model, updates=0)
        return self

    def _nc_model(self, nc, names):
        """engine/trainer.py get_model: the YAML is re-instantiated with the dataset's class count; weights carry over."""
        if getattr(self.model.model[-1], "nc", nc) != nc:
            fresh = DetectionModel(self.cfg or self.model.yaml, nc=nc, verbose=False)
            own = fresh.state_dict()
            fresh.load_state_dict({k: v for k, v in self.model.state_dict().items() if k in own and own[k].shape == v.shape}, strict=False)
            self.model = fresh
        self.model.names = names
        self.model.nc = nc
        return self.model

    # ---- train / val / predict
    def train(self, data, epochs=100, batch=16, imgsz=640, workers=8, seed=0, save_dir=None, close_mosaic=10, patience=100, lrf=0.01,
              cos_lr=False, resume=False, val=True, **overrides):
        """engine/model.py:754-840 -> DetectionTrainer (engine/trainer.py): one process per GPU; under torchrun the RANK /
        WORLD_SIZE of the environment select the shard and switch on the RCCL gradient sum."""
        from ..data.dataset import build_dataloader, build_yolo_dataset
        from . import ddp
        from .trainer import DetectionTrainer
        devices = _device_list(overrides.pop("device", None))
        if len(devices) > 1 and "RANK" not in os.environ:
            # engine/trainer.py:170-207 + utils/dist.py:25-66: `device=[0, 1, ...]` outside a launcher -> one CHILD process per
            # GPU runs this very call; the parent waits and then continues with best.pt, as the reference does
            return self._train_ddp(devices, dict(data=data, epochs=epochs, batch=batch, imgsz=imgsz, workers=workers, seed=seed,
                                                 save_dir=save_dir, close_mosaic=close_mosaic, patience=patience, lrf=lrf, cos_lr=cos_lr,
                                                 resume=resume, val=val, **overrides))
        if len(devices) == 1 and "RANK" not in os.environ:
            self.device = torch.device("cuda", devices[0])
        unknown = set(overrides) - _TRAIN_KEYS - set(_hyp_defaults())
        if unknown:
            raise SyntaxError(f"unknown train arguments {sorted(unknown)} (sy11 carries {sorted(_TRAIN_KEYS | set(_hyp_defaults()))})")
        data = check_det_dataset(data)
        rank, local, world = ddp.setup_process_group()
        dev = torch.device("cuda", local) if self.device.type == "cuda" else self.device
        torch.manual_seed(seed + 1 + rank); random.seed(seed + 1 + rank); np.random.seed(seed + 1 + rank)      # trainer.py:107
        model = self._nc_model(data["nc"], data["names"])
        tr_over = {k: v for k, v in overrides.items() if k in _TRAIN_KEYS}
        tr_over["imgsz"] = imgsz
        iq = data.get("kind") == "iq"
        producer = _iq_setup(data, imgsz, overrides, dev) if iq else None
        self.trainer = DetectionTrainer(model, batch_size=batch, device=dev, overrides=tr_over, world_size=world, producer=producer)
        if iq:                                                                   # recorded in the checkpoint's train_args: `scan` needs
            for k in ("sample_rate", "center_freq", "n_fft", "hop"):             # the same transform the model was trained on
                setattr(self.trainer.args, k, data[k])
        if resume and self.ckpt is not None:
            start = self.trainer.resume_training(self.ckpt)
        else:
            start = 0
        hyp = SimpleNamespace(**{**_hyp_defaults(), **{k: v for k, v in overrides.items() if k in _hyp_defaults()}}, imgsz=imgsz)
        stride = int(max(model.stride))
        if iq:
            from ..data.iq_dataset import build_iq_dataset
            ds = build_iq_dataset(hyp, data["train"], batch, data, mode="train", device=dev)
        else:
            ds = build_yolo_dataset(hyp, data["train"], batch, data, mode="train", stride=stride, device=dev)
        dl = build_dataloader(ds, batch, workers=workers, shuffle=True, rank=rank if world > 1 else -1, world_size=world,
                              out=self.trainer.batch_buffer(imgsz), dtype=torch.float32)
        val_batches = None
        if val and data.get("val"):
            vds = (build_iq_dataset(hyp, data["val"], batch * 2, data, mode="val", device=dev) if iq else
                   build_yolo_dataset(hyp, data["val"], batch * 2, data, mode="val", rect=True, stride=stride, device=dev))
            vdl = build_dataloader(vds, batch * 2, workers=workers, shuffle=False)
            val_batches = lambda: vdl                                                                            # noqa: E731
        save_dir = save_dir or Path("runs") / "detect" / "train"
        hist = self.trainer.fit(dl, epochs, val_batches=val_batches, save_dir=save_dir, close_mosaic=close_mosaic, start_epoch=start,
                                lrf=lrf, cos_lr=cos_lr, patience=patience)
        self.metrics = hist[-1]["metrics"] if hist else None
        if rank in (-1, 0):                                                      # the per-epoch records (what results.csv holds in the
            import json                                                          # reference); a launching parent reads them back
            Path(save_dir).mkdir(parents=True, exist_ok=True)
            (Path(save_dir) / "results.json").write_text(json.dumps(hist, default=str))
        best = Path(save_dir) / "best.pt"
        if rank in (-1, 0) and best.exists():                                    # engine/model.py:833-837: continue with best.pt
            self.model, self.ckpt = attempt_load_one_weight(str(best), device=dev)
        return hist

    def _train_ddp(self, devices, kw):
        """Spawn len(devices) ranks of `YOLO(<same model>).train(<same arguments>)` and wait (sy11.engine.ddp.launch)."""
        import json
        import tempfile
        from . import ddp
        from .. import _lib
        if torch.cuda.is_initialized():
            raise _lib.Sy11Error("train(device=[...]) starts one process per GPU and must do so before THIS process has touched "
                                 "the GPU (construct YOLO(...) from a .yaml, or with device='cpu'); alternatively launch the "
                                 "script with `python -m torch.distributed.run --nproc-per-node N`")
        save_dir = str(kw.get("save_dir") or Path("runs") / "detect" / "train")
        kw = {**kw, "save_dir": save_dir, "data": kw["data"] if isinstance(kw["data"], dict) else str(kw["data"])}
        payload = {"pkg": str(Path(__file__).resolve().parents[2]), "model": self.model_name, "nc": getattr(self.model.model[-1], "nc", None),
                   "kw": kw}
        # guarded: anything that re-imports this file as a module (multiprocessing's spawn bootstrap does) must not train again
        src = ("import json, sys\n"
               "if __name__ == '__main__':\n"
               f"    P = json.loads({json.dumps(json.dumps(payload, default=str))})\n"
               "    sys.path.insert(0, P['pkg'])\n"
               "    from sy11.engine.model import YOLO\n"
               "    m = YOLO(P['model'], nc=P['nc']) if str(P['model']).endswith(('.yaml', '.yml')) else YOLO(P['model'])\n"
               "    m.train(**P['kw'])\n")
        with tempfile.NamedTemporaryFile("w", suffix=".py", prefix="_sy11_ddp_", delete=False) as f:
            f.write(src)
        vis = ",".join(str(d) for d in devices)
        env = {**os.environ, "HIP_VISIBLE_DEVICES": vis, "CUDA_VISIBLE_DEVICES": vis}
        if "SY11_FORCE_DEVICE" in os.environ:                  # rehearsal of N ranks on fewer GPUs (ddp.setup_process_group): the ranks
            env = dict(os.environ)                             # share the forced device, the visibility list is left alone
        try:
            ddp.launch([f.name], len(devices), env=env)
        finally:
            os.unlink(f.name)
        best = Path(save_dir) / "best.pt"
        last = Path(save_dir) / "last.pt"
        ck = best if best.exists() else last
        if ck.exists():
            self.model, self.ckpt = attempt_load_one_weight(str(ck), device="cpu")
        rec = Path(save_dir) / "results.json"
        hist = json.loads(rec.read_text()) if rec.exists() else []               # same return type as the single-process branch
        self.metrics = hist[-1]["metrics"] if hist else None
        return hist

    def val(self, data=None, batch=32, imgsz=640, conf=0.001, iou=0.7, half=False, workers=8, **kw):
        """engine/model.py:623-670 -> DetectionValidator over the rect val loader."""
        from ..data.dataset import build_dataloader, build_yolo_dataset
        from .validator import DetectionValidator
        data = check_det_dataset(data)
        hyp = SimpleNamespace(**_hyp_defaults(), imgsz=imgsz)
        self.model.names = data["names"]
        producer = None
        if data.get("kind") == "iq":
            from ..data.iq_dataset import build_iq_dataset
            producer = _iq_setup(data, imgsz, {}, self.device)
            vds = build_iq_dataset(hyp, data["val"], batch, data, mode="val", device=self.device)
        else:
            vds = build_yolo_dataset(hyp, data["val"], batch, data, mode="val", rect=True, stride=int(max(self.model.stride)), device=self.device)
        vdl = build_dataloader(vds, batch, workers=workers, shuffle=False)
        self.metrics = DetectionValidator(self.model, device=self.device, conf=conf, iou=iou, half=half, producer=producer)(self.model, vdl)
        return self.metrics

    def predict(self, source, conf=0.25, iou=0.7, imgsz=640, max_det=300, classes=None, agnostic_nms=False, half=False, **kw):
        """engine/model.py:500-560 -> DetectionPredictor.  ``source``: an (h, w, 3) BGR uint8 array, a list of them, image / .npy
        file paths, or a (B, 3, H, W) tensor."""
        from ..data.dataset import read_image
        from .predictor import DetectionPredictor
        if self.predictor is None or self.predictor.args["conf"] != conf or self.predictor.args["iou"] != iou or self.predictor.imgsz != ((imgsz, imgsz) if isinstance(imgsz, int) else tuple(imgsz)):
            self.predictor = DetectionPredictor(self.model, device=self.device, conf=conf, iou=iou, max_det=max_det, classes=classes,
                                                agnostic_nms=agnostic_nms, half=half, imgsz=imgsz)
        paths = None
        if isinstance(source, (str, Path)):
            source = [source]
        if isinstance(source, np.ndarray):
            source = [source]
        if isinstance(source, (list, tuple)):
            paths = [str(s) if isinstance(s, (str, Path)) else None for s in source]
            source = [read_image(s) if isinstance(s, (str, Path)) else s for s in source]
        return self.predictor(source, paths=paths)

    __call__ = predict

    def scan(self, source, sample_rate, center_freq=0.0, conf=0.25, iou=0.7, overlap=0.5, batch=64, merge="ios", merge_thres=0.5,
             max_det=300, classes=None, agnostic_nms=False, half=False, stride_frames=None, n_fft=1024, hop=256, imgsz=640,
             resample_to=None, tune_to=None, channels=None, oversample=2, select=None, link=None):
        """Detect over a long IQ capture (no reference counterpart) -> ``ScanResults`` with boxes in strip frames / image rows and
        in seconds / Hz.  ``source``: a 1-D complex64 tensor or ndarray, a ``.npy`` of complex64, or a raw interleaved-float32
        file (``.cf32`` / ``.fc32`` / ``.iq``), opened with ``np.memmap`` and read chunk by chunk.  ``sample_rate`` in Hz,
        ``center_freq`` the RF centre the capture was tuned to.  See ``DetectionPredictor.scan`` for ``overlap`` / ``merge``.
        ``n_fft`` / ``hop`` / ``imgsz`` (n_frames = n_mel) select the transform; a model trained from IQ captures records its own in
        the checkpoint, and a scan with another one warns (its results are those of the transform asked for).
        ``resample_to`` (Hz, or ``"model"`` = the rate, and the centre if there is one, that the checkpoint records) / ``tune_to``
        (Hz): resample and retune the capture on the GPU first, so that a recording taken at another rate or tuning meets the
        transform the model knows (``DetectionPredictor.scan``); boxes stay in seconds of the capture and absolute Hz.
        ``channels`` (K, a ``ChannelPlan`` or ``"model"``) / ``oversample`` / ``select``: split a wideband capture into K bands with
        a polyphase filter bank on the GPU and scan every selected band from one read of the capture; the rows carry their band in
        ``ScanResults.channel`` (``DetectionPredictor.scan``).
        ``link`` = True, or a dict of ``link``'s keywords: link the boxes of one emission into tracks before returning (``link``)."""
        from ..data.spectrogram import SpectrogramProducer, open_iq
        from .predictor import DetectionPredictor, link_keywords, plan_scan_ddc
        trained = (self.ckpt or {}).get("train_args") or {}
        link = link_keywords(link)                            # argument errors come first, before anything touches the device
        if channels is not None:                              # argument errors come first, before anything touches the device
            from ..data.channelize import plan_scan_channels
            channels, select = plan_scan_channels(sample_rate, channels, oversample, select, trained, resample_to, tune_to)
            oversample = channels.oversample
        elif resample_to is not None or tune_to is not None:
            resample_to, tune_to = plan_scan_ddc(sample_rate, center_freq, resample_to, tune_to, trained), None
        if "n_fft" in trained and (trained["n_fft"], trained["hop"], trained.get("imgsz", imgsz)) != (n_fft, hop, imgsz):
            import warnings                                   # the results are those of the transform asked for, as they always were
            warnings.warn(f"scan(n_fft={n_fft}, hop={hop}, imgsz={imgsz}) differs from the transform this model was trained on "
                          f"(n_fft={trained['n_fft']}, hop={trained['hop']}, imgsz={trained.get('imgsz')})", stacklevel=2)
        key = (conf, iou, max_det, classes if classes is None else tuple(classes), agnostic_nms, half, n_fft, hop, imgsz)
        if getattr(self, "_scanner_key", None) != key:
            self._scanner = DetectionPredictor(self.model, device=self.device, conf=conf, iou=iou, max_det=max_det, classes=classes,
                                               agnostic_nms=agnostic_nms, half=half, imgsz=imgsz,
                                               producer=SpectrogramProducer(self.device, n_fft, hop, imgsz, imgsz))
            self._scanner_key = key
        self._scanner.trained = trained
        return self._scanner.scan(open_iq(source), sample_rate, center_freq=center_freq, overlap=overlap, batch=batch, merge=merge,
                                  merge_thres=merge_thres, stride_frames=stride_frames, resample_to=resample_to, tune_to=tune_to,
                                  channels=channels, oversample=oversample, select=select, link=link)

    def link(self, results, gap_t="auto", gap_f="auto", align=0.5, agnostic=False, hop=None):
        """Link the boxes of one emission longer than a window, or wider than a band, into tracks -> the same ``results`` with
        ``results.track`` (the track of every row) and ``results.tracks`` (``sy11.data.link.Tracks``: one union rectangle, class and
        confidence per emission) set; ``extract(source, results.tracks, ...)`` then cuts one clip per emission
        (``DetectionPredictor.link``)."""
        from ..data.link import link_results
        tracks = link_results(results, self.device, gap_t, gap_f, align, agnostic, hop)
        results.track, results.tracks = tracks.track, tracks
        return results

    def extract(self, source, results, sample_rate, center_freq=0.0, rows=None, pad_t=0.0, pad_f=0.1, decimate="auto", chunk_samples=1 << 24):
        """Take every detection of ``results`` (what ``scan`` returned for this capture) out of the recording as baseband IQ ->
        ``sy11.data.extract.Extraction`` (``DetectionPredictor.extract``).  ``source`` as in ``scan``; ``sample_rate`` / ``center_freq`` are
        the capture's own, also after ``scan(resample_to=)`` or ``scan(channels=)``."""
        from ..data.extract import extract_results
        from ..data.spectrogram import open_iq
        return extract_results(open_iq(source), results, sample_rate, center_freq, self.device, rows, pad_t, pad_f, decimate, chunk_samples)

    def measure(self, source, results, sample_rate, center_freq=0.0, rows=None, n_fft=1024, pad_f=0.25, beta=0.99, noise_band=0.8,
                envelope=True, chunk_samples=1 << 24):
        """Measure every detection of ``results`` (what ``scan`` returned for this capture, or its ``tracks``) on the GPU ->
        ``sy11.data.measure.Measurement``: received power, noise density, SNR, the ``beta`` occupied bandwidth, a power-weighted centre
        frequency, the Welch spectrum and, with ``envelope``, the in-box power of every frame (``DetectionPredictor.measure``).
        ``source``, ``results``, ``rows``, ``sample_rate`` and ``center_freq`` as in ``extract``: the rate and centre are the capture's own, also
        after ``scan(resample_to=)`` or ``scan(channels=)``."""
        from ..data.measure import measure_results
        from ..data.spectrogram import open_iq
        return measure_results(open_iq(source), results, sample_rate, center_freq, self.device, rows, n_fft, pad_f, beta, noise_band,
                               envelope, chunk_samples)

    def characterize(self, extraction, n_fft=1024, min_rate=None, line_db=13.0):
        """Characterise every clip of ``extraction`` (what ``extract`` returned) on the GPU -> ``sy11.data.characterize.Characterization``:
        symbol rate, carrier offset at order 2 and 4, the decision between them, the fourth-order cumulant and the spectra of |x|^2, x^2
        and x^4 (``DetectionPredictor.characterize``)."""
        from ..data.characterize import characterize_extraction
        return characterize_extraction(extraction, n_fft, min_rate, line_db)

    def demodulate(self, extraction, characterization=None, *, symbol_rate=None, offset=None, order=None, beta=0.35, span=8, block=32):
        """Demodulate every clip of ``extraction`` on the GPU -> ``sy11.data.demodulate.Demodulation``: the symbol stream, the decisions and the
        error-vector magnitude of every BPSK / four-phase clip, started from ``characterization`` (what ``characterize`` returned) or from
        explicit ``symbol_rate`` / ``offset`` / ``order`` (``DetectionPredictor.demodulate``)."""
        from ..data.demodulate import demodulate_extraction
        return demodulate_extraction(extraction, characterization, symbol_rate=symbol_rate, offset=offset, order=order, beta=beta, span=span,
                                     block=block)

    def demodulate_fsk(self, extraction, *, symbol_rate, offset=0.0, pulse="gauss", bt=0.5, span=2, block=32):
        """Demodulate every frequency-keyed clip (2-FSK, GFSK, GMSK) of ``extraction`` on the GPU -> ``sy11.data.demodulate_fsk.FskDemodulation``: a
        ``Demodulation`` at order 2 with real symbols around +-1, the decisions, the error-vector magnitude, the midpoint of the two tones and their
        deviation, from the caller's ``symbol_rate`` and ``offset`` (``DetectionPredictor.demodulate_fsk``)."""
        from ..data.demodulate_fsk import demodulate_fsk_extraction
        return demodulate_fsk_extraction(extraction, symbol_rate=symbol_rate, offset=offset, pulse=pulse, bt=bt, span=span, block=block)

    def demodulate_ofdm(self, extraction, *, n_fft, cp, carriers, pilots, order=4, offset=0.0, spacing=None, advance=None):
        """Demodulate every cyclic-prefix OFDM clip of ``extraction`` on the GPU -> ``sy11.data.demodulate_ofdm.OfdmDemodulation``: a ``Demodulation`` at the clips' ``order``
        with the data carriers of every OFDM symbol as corrected symbols and decisions, the error-vector magnitude, where the prefix starts and the carrier
        offset, from the caller's layout (``n_fft``, ``cp``, ``carriers``, ``pilots``) (``DetectionPredictor.demodulate_ofdm``)."""
        from ..data.demodulate_ofdm import demodulate_ofdm_extraction
        return demodulate_ofdm_extraction(extraction, n_fft=n_fft, cp=cp, carriers=carriers, pilots=pilots, order=order, offset=offset, spacing=spacing, advance=advance)

    def find_frames(self, demodulation, words, *, payload=0, threshold=0.8, max_errors=None, t0=None):
        """Find the sync ``words`` in every clip of ``demodulation`` on the GPU -> ``sy11.data.frames.Frames``: per frame its clip, word, position, the
        rotation that resolves the demodulator's phase ambiguity, the word's errors and ``payload`` symbols' bits
        (``DetectionPredictor.find_frames``)."""
        from ..data.frames import find_frames
        return find_frames(demodulation, words, payload=payload, threshold=threshold, max_errors=max_errors, t0=t0)

    def equalize(self, frames, demodulation, *, taps=7, reg=1e-3, refine=0):
        """Equalise every frame of ``frames`` (found in ``demodulation``) on the GPU -> ``sy11.data.equalize.Equalized``: per frame the least-squares taps of a symbol-spaced
        FIR trained on its sync word, applied to the symbols the frame owns; ``find_frames`` and ``decode`` take the result in place of the demodulation
        (``DetectionPredictor.equalize``)."""
        from ..data.equalize import equalize_frames
        return equalize_frames(frames, demodulation, taps=taps, reg=reg, refine=refine)

    def decode(self, frames, demodulation, *, n_info, polys=(0o171, 0o133), puncture=None, tail=True, whiten=None, crc=None, soft_scale=32.0):
        """Decode every frame of ``frames`` (found in ``demodulation``) on the GPU -> ``sy11.data.decode.Decoded``: per frame the Viterbi-decoded, de-whitened
        information bits, the channel bit errors against the re-encoded decision and whether the CRC holds (``DetectionPredictor.decode``)."""
        from ..data.decode import decode_frames
        return decode_frames(frames, demodulation, n_info=n_info, polys=polys, puncture=puncture, tail=tail, whiten=whiten, crc=crc, soft_scale=soft_scale)

    def decode_ldpc(self, frames, demodulation, *, code, iterations=20, scale=12, whiten=None, crc=None, soft_scale=16.0):
        """Decode every frame of ``frames`` (found in ``demodulation``) as a codeword of the quasi-cyclic LDPC code ``code`` on the GPU -> ``sy11.data.ldpc.LdpcDecoded``:
        per frame the de-whitened information bits of the layered min-sum decoder, the iterations it ran, whether every check is satisfied, the channel bit
        errors against the decision and whether the CRC holds (``DetectionPredictor.decode_ldpc``)."""
        from ..data.ldpc import decode_ldpc_frames
        return decode_ldpc_frames(frames, demodulation, code=code, iterations=iterations, scale=scale, whiten=whiten, crc=crc, soft_scale=soft_scale)

    def correct(self, decoded, *, code="dvb-204-188", interleave=1, offset=0, crc=None):
        """Correct every frame of ``decoded`` with the Reed-Solomon outer code on the GPU -> ``sy11.data.correct.Corrected``: per frame the information bytes of
        its ``interleave`` de-interleaved codewords, the byte errors corrected in each (-1: beyond the code) and whether the CRC over them holds
        (``DetectionPredictor.correct``)."""
        from ..data.correct import correct_decoded
        return correct_decoded(decoded, code=code, interleave=interleave, offset=offset, crc=crc)


def _device_list(device):
    """`device=0`, `"0,1"`, `[0, 1]`, `"cuda:1"` -> list of GPU indices (utils/torch_utils.py select_device's parsing)."""
    if device is None or device == "" or str(device) == "cpu":
        return []
    from .. import _lib
    try:
        if isinstance(device, (list, tuple)):
            return [int(d) for d in device]
        txt = str(device).lower().replace("cuda:", "").replace("(", "").replace(")", "").replace("[", "").replace("]", "").replace(" ", "")
        if txt == "cuda":
            return [0]
        return [int(d) for d in txt.split(",") if d != ""]
    except (TypeError, ValueError):
        raise _lib.Sy11Error(f"device={device!r}: expected 'cpu', a GPU index, 'cuda:N', '0,1' or a list of indices "
                             f"(the MI355X is the only accelerator this build drives)") from None


def _hyp_defaults():
    from ..data.dataset import DEFAULT_HYP
    from ..data.iq_augment import IQ_HYP
    return {**DEFAULT_HYP, **IQ_HYP}
