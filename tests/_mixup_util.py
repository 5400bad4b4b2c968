"""Shared by the MixUp tests: the product pipeline on the generator's in-memory dataset (tests/golden/mixup.npz, written by
tools/gen_golden_mixup.py), and the numpy execution of a recorded recipe with oracle.image_ref's functions."""
import importlib.util
import random
from pathlib import Path
from types import SimpleNamespace

import numpy as np

from oracle import image_ref as IR
from tests._augment_util import BASE, IMGSZ, FakeDataset  # noqa: F401  (re-exported)

_spec = importlib.util.spec_from_file_location("gen_golden_mixup", Path(__file__).resolve().parents[1] / "tools" / "gen_golden_mixup.py")
_gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_gen)                          # module level only: the config table (the reference is imported in main())
CONFIGS, N_SAMPLES = _gen.CONFIGS, _gen.N_SAMPLES


class LazyFakeDataset(FakeDataset):
    """The same dataset as a loader worker process sees it: images are LazyImage file nodes (a shape, no pixels), so the LetterBox
    of the non-mosaic samples is recorded instead of launched and the whole pipeline runs without a GPU."""

    def get_image_and_label(self, i):
        from sy11.data.recipe import file_image
        out = super().get_image_and_label(i)
        out["img"] = self._di.wrap(file_image(i, self.imgs[i].shape[:2]))
        return out


def run_pipeline(gold, name, device, lazy=False):
    """Yield (k, labels) for the N_SAMPLES samples of config `name`, RNG seeded like the generator; finally (None, rng_after)."""
    from sy11.data.augment import Format, v8_transforms
    hyp = SimpleNamespace(**{**BASE, **CONFIGS[name]})
    ds = (LazyFakeDataset if lazy else FakeDataset)(gold, device)
    tf = v8_transforms(ds, IMGSZ, hyp)
    tf.append(Format(bbox_format="xywh", normalize=True, batch_idx=True, bgr=hyp.bgr, defer=True))
    random.seed(1234)
    np.random.seed(1234)
    for k in range(N_SAMPLES):
        yield k, tf(ds.get_image_and_label(k % len(ds)))
    yield None, np.asarray([random.random(), np.random.uniform()])


def _np(t):
    return t if isinstance(t, np.ndarray) else t.cpu().numpy()


def oracle_geometry(tiles, canvas_hw, minv, out_hw, fill=114):
    """Canvas paste -> cv2.warpAffine fixed-point bilinear (oracle.image_ref.warp_coords), as uint8 HWC."""
    canvas = np.full((*canvas_hw, 3), fill, np.uint8)
    for t, x1, y1, x2, y2, pw, ph in tiles:
        canvas[y1:y2, x1:x2] = _np(t)[y1 - ph:y2 - ph, x1 - pw:x2 - pw]
    if minv is None:
        assert tuple(canvas_hw) == tuple(out_hw)
        return canvas
    sx, sy, fx, fy = IR.warp_coords(minv, out_hw[1], out_hw[0])
    src = canvas.astype(np.int64)

    def tap(xx, yy):
        inside = (xx >= 0) & (xx < canvas.shape[1]) & (yy >= 0) & (yy < canvas.shape[0])
        return np.where(inside[..., None], src[np.clip(yy, 0, canvas.shape[0] - 1), np.clip(xx, 0, canvas.shape[1] - 1)], fill)

    w = [((32 - fy) * (32 - fx) * 32)[..., None], ((32 - fy) * fx * 32)[..., None], (fy * (32 - fx) * 32)[..., None], (fy * fx * 32)[..., None]]
    return ((tap(sx, sy) * w[0] + tap(sx + 1, sy) * w[1] + tap(sx, sy + 1) * w[2] + tap(sx + 1, sy + 1) * w[3] + 16384) >> 15).astype(np.uint8)


def oracle_render(di, reverse_c=None):
    """Execute a DeviceImage recipe (with or without a MixUp partner) in numpy -> uint8 CHW, channel order as Format decided."""
    img = oracle_geometry(di.tiles, di.canvas_hw, di.minv, di.out_hw, di.fill)
    if di.partner is not None:
        p, r = di.partner, di.mix_r
        img2 = oracle_geometry(p.tiles, p.canvas_hw, p.minv, p.out_hw, di.fill)
        img = (img * r + img2 * (1 - r)).astype(np.uint8)                     # MixUp._mix_transform, augment.py:946
    if di.lut is not None:
        hsv = IR.cv2_bgr2hsv_u8(img)
        img = IR.cv2_hsv2bgr_u8(np.stack((di.lut[0][hsv[..., 0]], di.lut[1][hsv[..., 1]], di.lut[2][hsv[..., 2]]), -1))
    if di.flip_ud:
        img = img[::-1]
    if di.flip_lr:
        img = img[:, ::-1]
    chw = img.transpose(2, 0, 1)
    return np.ascontiguousarray(chw[::-1] if (di.final_reverse_c if reverse_c is None else reverse_c) else chw)


def predict_mixes(images_dir, imgsz, batch, seed, hyp_overrides, epochs=1):
    """How many samples of each of the first `epochs` epochs of `YOLO.train(seed=seed, workers=0, **hyp_overrides)` carry a MixUp
    partner, found WITHOUT a GPU: the draws and the sample order need no pixels, so the dataset runs in recipe mode (images are
    LazyImage nodes) on the CPU under the generators train() seeds (seed + 1) and the loader's own permutation generator."""
    import torch
    from sy11.data.dataset import DEFAULT_HYP, InfiniteDataLoader, YOLODataset
    random.seed(seed + 1)
    np.random.seed(seed + 1)
    hyp = SimpleNamespace(**{**DEFAULT_HYP, **hyp_overrides}, imgsz=imgsz)
    ds = YOLODataset(images_dir, imgsz=imgsz, augment=True, batch_size=batch, hyp=hyp, data={"nc": 2}, device="cpu")
    ds.recipe_mode = True
    dl = InfiniteDataLoader(ds, batch, shuffle=True, prefetch=0)
    counts = []
    for _ in range(epochs):
        counts.append(sum(ds[i]["img"].partner is not None for i in dl._epoch_indices()))
    assert torch.initial_seed() is not None
    return counts
