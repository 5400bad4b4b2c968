"""GPU: training and validating from IQ captures end to end — the loader's windows against the producer, resident against staged
sources, and `YOLO.train / .val / .scan` on a `kind: iq` data YAML.  Four captures of 2 - 3 windows, 2 classes, the accuracy gate's
geometry (imgsz 320, n_fft 512, hop 128)."""
import math
import random
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from . import _iq_ref as R
from ._iq_util import CAPTURES, FC, HOP, IMGSZ, L, N_FFT, SR, write_dataset

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AUG = dict(iq_shift=0.25, iq_conj=0.5, iq_gain_db=6.0, iq_noise_db=10.0, iq_mixup=0.5)


@pytest.fixture(scope="module")
def dataset_dir(tmp_path_factory):
    root = tmp_path_factory.mktemp("iqds")
    y, caps = write_dataset(root)
    return root, y, caps


def loader(dataset_dir, mode, batch, **kw):
    from sy11.data.dataset import build_dataloader
    from sy11.data.iq_dataset import IQDataLoader, build_iq_dataset
    from sy11.engine.model import _hyp_defaults, check_det_dataset
    data = check_det_dataset(dataset_dir[1])
    hyp = SimpleNamespace(**{**_hyp_defaults(), **kw}, imgsz=IMGSZ)
    ds = build_iq_dataset(hyp, data[mode], batch, data, mode=mode, device=DEV)
    dl = build_dataloader(ds, batch, workers=8, shuffle=False)
    assert isinstance(dl, IQDataLoader)                                       # whatever `workers` says
    return ds, dl


def test_unaugmented_loader_images_equal_the_producer_bit_for_bit(dataset_dir):
    from sy11.data import iq_augment as A
    from sy11.data.spectrogram import SpectrogramProducer
    from sy11.engine.trainer import DetectionTrainer
    from sy11.nn.tasks import DetectionModel
    caps = dataset_dir[2]
    producer = SpectrogramProducer(DEV, N_FFT, HOP, IMGSZ, IMGSZ)
    tr = DetectionTrainer(DetectionModel("yolo11n.yaml", nc=2, verbose=False), batch_size=4, device=DEV, overrides={"imgsz": IMGSZ},
                          producer=producer, graphs=False)
    ds, dl = loader(dataset_dir, "train", 4, iq_jitter=0.0)
    g = A.Geometry(SR, FC, N_FFT, HOP, IMGSZ, IMGSZ)
    seen = 0
    for batch in dl:
        n = batch["iq"].shape[0]
        items = ds.items[seen:seen + n]
        win = np.stack([caps[c][f * HOP:f * HOP + L] for c, f in items])
        assert torch.equal(torch.view_as_real(batch["iq"]).cpu(), torch.view_as_real(torch.from_numpy(win)))
        want_img = producer(torch.from_numpy(win).to(DEV))
        lb = [A.window_labels(ds.rows[c], A.IQSource(c, f * HOP), g) for c, f in items]
        got = tr.preprocess_batch(dict(batch))
        assert got["img"].shape == (n, 3, IMGSZ, IMGSZ) and torch.equal(got["img"], want_img)
        assert torch.equal(batch["cls"], torch.from_numpy(np.concatenate(lb)[:, 0:1]))
        assert torch.equal(batch["bboxes"], torch.from_numpy(np.concatenate(lb)[:, 1:5]))
        assert torch.equal(batch["batch_idx"], torch.cat([torch.full((len(x),), float(i)) for i, x in enumerate(lb)]))
        seen += n
    assert seen == len(ds) == 11
    # the first burst of capture a, window 0, by the restatement's arithmetic: cls 0, 10 - 30 ms, fc + 0.1 .. 0.2 MHz
    c, t0, t1, f_lo, f_hi = CAPTURES[0][2][0]
    x = [R.time_to_col(t, SR, N_FFT, HOP) + 0.5 for t in (t0, t1)]
    y = [R.freq_to_row(f, SR, FC, N_FFT, IMGSZ) + 0.5 for f in (f_lo, f_hi)]
    first = A.window_labels(ds.rows[0], A.IQSource(0, 0), g)[0]
    want = [c, (x[0] + x[1]) / 2 / IMGSZ, (y[0] + y[1]) / 2 / IMGSZ, (x[1] - x[0]) / IMGSZ, (y[1] - y[0]) / IMGSZ]
    assert np.abs(first - np.array(want)).max() <= 2e-7


def test_resident_and_staged_sources_give_identical_bits(dataset_dir):
    outs = []
    for budget in (None, 0):
        random.seed(77)
        kw = dict(AUG) if budget is None else dict(AUG, iq_cache_bytes=0)
        ds, dl = loader(dataset_dir, "train", 4, **kw)
        assert ds.source_cache().resident == (budget is None)
        batches = [b for b in dl] + [b for b in dl]                           # two epochs: both staging buffers are reused
        torch.cuda.synchronize()
        outs.append(batches)
        if budget == 0:
            ds.cache.close()
    assert len(outs[0]) == len(outs[1]) == 6
    for a, b in zip(*outs):
        assert torch.equal(torch.view_as_real(a["iq"]), torch.view_as_real(b["iq"])) and torch.equal(a["bboxes"], b["bboxes"])
        assert torch.isfinite(torch.view_as_real(a["iq"])).all()
    assert not torch.equal(torch.view_as_real(outs[0][0]["iq"]), torch.view_as_real(outs[0][3]["iq"]))   # epochs differ: new draws


def test_yolo_train_val_scan_from_iq_captures(dataset_dir, tmp_path):
    from sy11.engine.model import YOLO
    root, yaml, caps = dataset_dir
    kw = dict(batch=4, imgsz=IMGSZ, workers=0, seed=3, deterministic=True, iq_shift=0.25, iq_conj=0.5, iq_noise_db=10, iq_mixup=0.5)
    torch.manual_seed(0)                                                      # the same initial weights for both runs
    y = YOLO("yolo11n.yaml", device=DEV, nc=2)
    hist = y.train(data=str(yaml), epochs=2, close_mosaic=1, save_dir=tmp_path / "run", **kw)
    assert len(hist) == 2 and all(math.isfinite(v) for h in hist for v in h["train_loss"])
    assert (tmp_path / "run" / "last.pt").exists()
    args = torch.load(tmp_path / "run" / "last.pt", weights_only=False)["train_args"]
    assert (args["sample_rate"], args["center_freq"], args["n_fft"], args["hop"]) == (SR, FC, N_FFT, HOP)
    m = y.val(data=str(yaml), batch=4, imgsz=IMGSZ)
    assert "metrics/mAP50(B)" in m and all(math.isfinite(float(v)) for v in m.values())
    with warnings.catch_warnings(record=True) as caught:                      # the transform the model was trained on: no warning
        warnings.simplefilter("always")
        res = y.scan(str(root / "iq" / "c.npy"), SR, center_freq=FC, conf=0.001, n_fft=N_FFT, hop=HOP, imgsz=IMGSZ)
    assert not [w for w in caught if "trained on" in str(w.message)]
    assert res.start.tolist() == [0, 160, 320, 480, 640] and res.tf.shape == (len(res), 4)
    with pytest.warns(UserWarning, match="trained on"):
        y.scan(torch.from_numpy(np.tile(caps[2], 2)), SR, center_freq=FC)     # the default 1024 / 256 / 640 transform still runs
    # the same seed repeats the run: epoch 0 of a second run has the same mean loss, so the same first step
    torch.manual_seed(0)
    y2 = YOLO("yolo11n.yaml", device=DEV, nc=2)
    hist2 = y2.train(data=str(yaml), epochs=1, close_mosaic=0, save_dir=tmp_path / "run2", val=False, **kw)
    assert hist2[0]["train_loss"] == hist[0]["train_loss"]


def test_image_hyper_parameters_are_refused_for_iq(dataset_dir, tmp_path):
    from sy11.engine.model import YOLO
    y = YOLO("yolo11n.yaml", device=DEV, nc=2)
    for bad in (dict(mosaic=1.0), dict(hsv_h=0.015), dict(multi_scale=True)):
        with pytest.raises(ValueError, match="kind: iq"):
            y.train(data=str(dataset_dir[1]), epochs=1, batch=4, imgsz=IMGSZ, save_dir=tmp_path / "no", **bad)
