"""GPU: MixUp rendered by one fused launch (sy11_image_mixup_warp) through the C-ABI.  Pixels, boxes and classes of every sample
equal the goldens recorded from the REFERENCE's v8_transforms(mixup > 0) + Format run (tests/golden/mixup.npz: reference control
flow and numpy blend, restated cv2 pixels — see oracle/image_ref.py), bit for bit; the blend alone is checked on every byte pair."""
import pickle
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests._golden import load
from tests._mixup_util import CONFIGS, IMGSZ, N_SAMPLES, oracle_render, predict_mixes, run_pipeline

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("name", list(CONFIGS))
def test_fused_render_matches_reference_pipeline(name):
    gold = load("mixup.npz")
    n = mixed = 0
    for k, out in run_pipeline(gold, name, DEV):
        if k is None:
            assert np.array_equal(out, gold[f"{name}.rng_after"])
            continue
        di = out["img"]
        assert (di.partner is not None) == bool(gold[f"{name}.{k}.mixed"])
        got = di.render(chw=True, reverse_c=di.final_reverse_c)
        assert got.is_cuda and got.dtype == torch.uint8
        assert np.array_equal(got.cpu().numpy(), gold[f"{name}.{k}.img"]), f"{name} sample {k}"
        assert np.array_equal(out["bboxes"].numpy(), gold[f"{name}.{k}.bboxes"]) and np.array_equal(out["cls"].numpy(), gold[f"{name}.{k}.cls"])
        # the float form folds preprocess_batch's /255 into the same launch
        slot = torch.empty((3, IMGSZ, IMGSZ), device=DEV)
        di.render(dst=slot, chw=True, reverse_c=di.final_reverse_c)
        assert torch.equal(slot.cpu(), torch.from_numpy(gold[f"{name}.{k}.img"]).float() / 255)
        n += 1
        mixed += di.partner is not None
    assert n == N_SAMPLES and mixed >= 3


def test_blend_alone_on_every_byte_pair():
    """No warp, no HSV, no flip: a[i, j] = i, b[i, j] = j -> all 65 536 (a, b) pairs per launch.  A blend done in float32, or with
    one product contracted into an fma, differs from numpy's two rounded float64 products + rounded sum on some of these."""
    from sy11 import ops as K
    gold = load("mixup.npz")
    rs = [float(gold[f"{n}.{k}.r"]) for n in CONFIGS for k in range(N_SAMPLES) if bool(gold[f"{n}.{k}.mixed"])]
    assert len(rs) == 24
    i, j = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    a = np.ascontiguousarray(np.stack((i, i, i), -1))
    b = np.ascontiguousarray(np.stack((j, j, j), -1))
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    for r in rs + [0.5, 0.0, 1.0]:
        dst = torch.empty((256, 256, 3), dtype=torch.uint8, device=DEV)
        K.image_mixup_warp([(ta, 0, 0, 256, 256, 0, 0)], (256, 256), None, [(tb, 0, 0, 256, 256, 0, 0)], (256, 256), None, r, dst, chw=False)
        want = (a * r + b * (1 - r)).astype(np.uint8)
        assert np.array_equal(dst.cpu().numpy(), want), r


def _count_calls(monkeypatch):
    from sy11 import ops as K
    calls = {"image_mixup_warp": 0, "image_mosaic_warp": 0, "image_letterbox": 0}
    for name in calls:
        def wrapped(*a, _f=getattr(K, name), _n=name, **kw):
            calls[_n] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(K, name, wrapped)
    return calls


def test_full_size_sample_is_one_launch_and_matches_oracle(monkeypatch):
    """BASELINE size: 640 x 640 out of two 1280 x 1280 virtual canvases of four 640 x 640 sources each, rotation + shear, HSV, both
    flips — vs the numpy composition of oracle.image_ref functions, and rendered by exactly ONE image_mixup_warp launch."""
    from sy11.data.augment import DeviceImage, Format, v8_transforms
    from sy11.utils.instance import Instances
    S = 640
    g = np.random.default_rng(12)
    yy, xx = np.mgrid[0:S, 0:S]
    imgs = []
    for i in range(8):                                                   # gradients + noise: interpolation on non-trivial content
        base = np.stack(((xx * (i + 1) + yy) % 256, (yy * 3 + 17 * i) % 256, (xx + 2 * yy) % 256), -1)
        imgs.append(((base + g.integers(0, 96, (S, S, 3))) % 256).astype(np.uint8))
    dev = [torch.from_numpy(im).to(DEV) for im in imgs]

    class DS:
        data, use_keypoints, buffer = {}, False, list(range(8))

        def __len__(self):
            return 8

        def get_image_and_label(self, i):
            return {"im_file": str(i), "ori_shape": (S, S), "resized_shape": (S, S), "img": DeviceImage.wrap(dev[i]),
                    "cls": np.full((1, 1), i % 2, np.float32), "ratio_pad": (1.0, 1.0),
                    "instances": Instances(np.array([[0.5, 0.5, 0.3, 0.3]], np.float32))}

    hyp = SimpleNamespace(hsv_h=0.015, hsv_s=0.7, hsv_v=0.4, degrees=7.0, translate=0.1, scale=0.5, shear=1.0, perspective=0.0, flipud=1.0,
                          fliplr=1.0, bgr=0.0, mosaic=1.0, mixup=1.0, copy_paste=0.0)
    ds = DS()
    tf = v8_transforms(ds, S, hyp)
    tf.append(Format(defer=True))
    random.seed(5); np.random.seed(5)
    calls = _count_calls(monkeypatch)
    out = tf(ds.get_image_and_label(0))
    di = out["img"]
    assert calls == {"image_mixup_warp": 0, "image_mosaic_warp": 0, "image_letterbox": 0}            # the transforms only wrote a recipe
    assert di.partner is not None and len(di.tiles) == 4 and len(di.partner.tiles) == 4 and di.flip_ud and di.flip_lr and di.lut is not None
    assert di.minv is not None and di.partner.minv is not None and di.minv != di.partner.minv
    assert all(tuple(t[0].shape) == (S, S, 3) for t in di.source_tiles())
    got = di.render(chw=True, reverse_c=di.final_reverse_c)
    assert calls == {"image_mixup_warp": 1, "image_mosaic_warp": 0, "image_letterbox": 0}
    want = oracle_render(di)
    assert got.shape == (3, S, S) and np.array_equal(got.cpu().numpy(), want)
    assert len(out["cls"]) == len(out["bboxes"]) and 0 < float(di.mix_r) < 1
    # and the un-mixed recipes differ from the mix (the partner really contributes)
    alone = di.frozen()
    alone.partner, alone.mix_r = None, None
    assert not np.array_equal(alone.render(chw=True, reverse_c=di.final_reverse_c).cpu().numpy(), want)
    assert calls == {"image_mixup_warp": 1, "image_mosaic_warp": 1, "image_letterbox": 0}


def _mix_dataset(root, n, size, device, mixup=1.0):
    from sy11.data.dataset import DEFAULT_HYP, YOLODataset
    from tests.test_augment_gpu import _write_dataset
    if not (root / "images").exists():
        _write_dataset(root, n=n, imgsz=size)
    return YOLODataset(str(root / "images"), imgsz=size, augment=True, batch_size=4, data={"nc": 2}, device=device,
                       hyp=SimpleNamespace(**{**DEFAULT_HYP, "mixup": mixup}))


def test_dataset_batches_render_into_static_input_like_single_samples(tmp_path):
    from sy11.data.dataset import YOLODataset
    ds = _mix_dataset(tmp_path / "d", 10, 64, DEV)
    random.seed(3); np.random.seed(3)
    samples = [ds[i] for i in (0, 3, 4, 7)]                                        # mosaic + mixup from files (png / npy, letterboxed sizes)
    assert all(s["img"].partner is not None for s in samples)
    singles = [s["img"].render(chw=True, reverse_c=s["img"].final_reverse_c, dtype=torch.float32).clone() for s in samples]
    want_u8 = [oracle_render(s["img"]) for s in samples]
    static = torch.zeros((4, 3, 64, 64), device=DEV)                               # stands for a graph's static input
    batch = YOLODataset.collate_fn(samples, out=static, dtype=torch.float32)
    assert batch["img"].data_ptr() == static.data_ptr()
    for b in range(4):
        assert torch.equal(batch["img"][b], singles[b])
        assert torch.equal(batch["img"][b].cpu(), torch.from_numpy(want_u8[b]).float() / 255)
    nl = batch["cls"].shape[0]
    assert batch["bboxes"].shape == (nl, 4) and batch["batch_idx"].shape == (nl,) and nl == sum(len(s["cls"]) for s in samples)


def test_worker_loader_with_mixup_gives_the_in_process_batches(tmp_path):
    """procs=2: worker w prepares batches w, w + 2, ... under seed + w; the same datasets run in-process under those seeds (real
    pixels, no LazyImage nodes) must render the same batches."""
    from sy11.data.dataset import WorkerLoader, YOLODataset
    ds = _mix_dataset(tmp_path / "d", 16, 96, DEV)
    twins = [pickle.loads(pickle.dumps(ds)) for _ in range(2)]
    dl = WorkerLoader(ds, 4, procs=2, shuffle=False, seed=5, dtype=torch.float32)
    try:
        got = [next(dl._it) for _ in range(6)]                                     # 4 batches of one epoch + two of the next
    finally:
        dl.close()
    order = [list(range(k, k + 4)) for k in (0, 4, 8, 12)] + [list(range(0, 4)), list(range(4, 8))]
    want = {}
    for w in range(2):
        seed = 1000003 * (5 + 1) + w
        random.seed(seed); np.random.seed(seed % 2**32); torch.manual_seed(seed)
        for bid in range(w, 6, 2):
            samples = [twins[w][i] for i in order[bid]]
            assert all(s["img"].partner is not None for s in samples)
            want[bid] = YOLODataset.collate_fn(samples, dtype=torch.float32)
    for bid, batch in enumerate(got):
        assert torch.equal(batch["img"], want[bid]["img"]) and batch["img"].dtype == torch.float32 and batch["img"].is_cuda, bid
        for k in ("bboxes", "cls", "batch_idx"):
            assert torch.equal(batch[k], want[bid][k]), (bid, k)
    assert float(got[0]["img"].std()) > 0.05


def test_mixup_warp_rejects_bad_arguments(monkeypatch):
    from sy11 import _lib, ops as K
    src = torch.zeros((8, 8, 3), dtype=torch.uint8, device=DEV)
    dst = torch.full((3, 16, 16), 7, dtype=torch.uint8, device=DEV)
    ok = [(src, 0, 0, 8, 8, 0, 0)]
    big = [(torch.zeros((16, 16, 3), dtype=torch.uint8, device=DEV), 0, 0, 16, 16, 0, 0)]
    M = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    bad = [
        lambda: K.image_mixup_warp(big, (16, 16), None, ok, (8, 8), None, 0.5, dst),                  # recipes of different output size
        lambda: K.image_mixup_warp(ok, (8, 8), None, big, (16, 16), None, 0.5, dst),
        lambda: K.image_mixup_warp(big, (16, 16), None, big, (16, 16), None, 1.5, dst),               # r outside [0, 1]
        lambda: K.image_mixup_warp(big, (16, 16), None, big, (16, 16), None, float("nan"), dst),
        lambda: K.image_mixup_warp(big, (16, 16), None, ok * 5, (16, 16), M, 0.5, dst),               # five tiles on side B
        lambda: K.image_mixup_warp(big, (16, 16), None, [(src, 0, 0, 9, 8, 0, 0)], (16, 16), M, 0.5, dst),   # tile reads outside its source
        lambda: K.image_mixup_warp([(src, 10, 10, 18, 18, 10, 10)], (16, 16), M, big, (16, 16), None, 0.5, dst),   # ... leaves the canvas (side A)
    ]
    for f in bad:
        with pytest.raises(_lib.Sy11Error):
            f()
    torch.cuda.synchronize()
    assert bool((dst == 7).all())                                                                  # nothing was launched
    K.image_mixup_warp(big, (16, 16), None, ok, (16, 16), M, 0.5, dst)                             # the same shapes, valid: 0 * .5 + (0 | 114) * .5
    assert set(dst.unique().tolist()) == {0, 57}


def test_front_door_train_with_mixup(tmp_path, monkeypatch):
    """`YOLO(cfg).train(data=yaml, mixup=0.5, close_mosaic=1, epochs=2)`: the front-door call of tests/test_engine_flow_gpu.py with the
    knob added.  Epoch 0 renders mixed samples (at least a quarter of them, predicted on the CPU from the draws alone), epoch 1
    runs with mosaic closed: MixUp is off, every sample is a plain recipe."""
    from sy11 import YOLO
    from sy11.data.dataset import YOLODataset
    from tests.test_engine_flow_gpu import _dataset
    S, SEED = 96, 0
    _dataset(tmp_path / "ds" / "train", 12, S, 5)
    _dataset(tmp_path / "ds" / "val", 6, S, 6)
    (tmp_path / "ds" / "data.yaml").write_text("path: .\ntrain: train/images\nval: val/images\nnames:\n  0: bright\n  1: dark\n")
    predicted = predict_mixes(str(tmp_path / "ds" / "train" / "images"), S, 6, SEED, dict(mixup=0.5, fliplr=0.0))[0]
    print("epoch 0: predicted mixed samples", predicted, "of 12")
    assert predicted >= 3
    calls = _count_calls(monkeypatch)
    at_close = []
    inner = YOLODataset.close_mosaic

    def closing(self, hyp):
        at_close.append(dict(calls))
        return inner(self, hyp)
    monkeypatch.setattr(YOLODataset, "close_mosaic", closing)
    y = YOLO("yolo11n.yaml", device=DEV)
    hist = y.train(data=str(tmp_path / "ds" / "data.yaml"), epochs=2, batch=6, imgsz=S, workers=0, seed=SEED, save_dir=tmp_path / "run",
                   close_mosaic=1, warmup_epochs=0.5, fliplr=0.0, mixup=0.5)
    assert len(hist) == 2 and all(np.isfinite(h["train_loss"]).all() for h in hist)
    assert len(at_close) == 1                                                    # closed once, before epoch 1
    epoch0 = at_close[0]["image_mixup_warp"]
    print("epoch 0: rendered mixed samples", epoch0, "of 12")
    assert epoch0 >= 3 and epoch0 == predicted                                   # a quarter of epoch 0 at least; the CPU prediction holds
    assert at_close[0]["image_mosaic_warp"] >= 12 - epoch0                       # the other samples of epoch 0 (+ its validation images)
    assert calls["image_mixup_warp"] == epoch0                                   # epoch 1 (and validation): no partner anywhere
    assert calls["image_mosaic_warp"] >= at_close[0]["image_mosaic_warp"] + 12
